"""Host side of the per-cell histograms of cells larger than the LDS (context option "cell_histogram_windows",
csrc/hmg_histogram_window.hip) and of the group sums on the device (hmg_cell_histogram_groups), without a GPU:
  * hmg_cell_histogram_groups on a host-only grid refuses every bad argument of its own by name -- before it asks for a device
    context, that is before any device work -- and with good arguments says what hmg_cell_histogram says on such a grid;
  * the numpy statement of the group sum (api.histogram_group_sum: per group the cells by ascending cell id, product and sum
    rounded separately) pinned on a hand-written 3-cell case whose bits tell the documented order from the reversed one and from
    a fused multiply-add;
  * driver._large_cells sets and restores all three window options, also when a pass raises.
A context exists only on a device, so the fourth thing -- the option takes 0, 1 and 2, reads back and refuses 3 -- is the one
test of this file that is marked `gpu`."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

L = hmg._lib
OPT = "cell_histogram_windows"


@pytest.fixture(scope="module")
def host(oracle):
    base = oracle.hypercube(2, 1)
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 3)
    assert g.ncells() == 2
    yield g
    g.close()


def call(g, ngroups, groups, weights, counts, volume, grid=True):
    lib = L.load()
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = lib.hmg_cell_histogram_groups(g.h if grid else None, None, None, None, 0, 1, 3, ngroups, p(groups, L.p_i32),
                                       p(weights, L.p_f64), p(counts, L.p_i64), p(volume, L.p_f64))
    return rc, lib.hmg_last_error().decode()


def test_groups_refuse_each_bad_argument_by_name(host):
    g = host
    nb = hmg.histogram_nbins(0, 1, 3)
    groups = np.array([1, -1], dtype=np.int32)
    w = np.array([0.5, 0.25])
    counts = np.zeros((2, nb), dtype=np.int64)
    vol = np.zeros((2, nb))
    who = "hmg_cell_histogram_groups: "
    cases = [((0, groups, w, counts, vol), "ngroups = 0"),
             ((-3, groups, w, counts, vol), "ngroups = -3"),
             ((65536, groups, w, counts, vol), "ngroups = 65536"),
             ((2, groups, w, None, vol), "null counts"),
             ((2, groups, w, counts, None), "weights are given and volume is null"),
             ((2, groups, None, counts, vol), "volume is given and weights are null"),
             ((2, None, w, counts, vol), "null group_of_cell"),
             ((2, np.array([1, 2], dtype=np.int32), w, counts, vol), "group_of_cell[1] = 2 is outside -1 to 1"),
             ((2, np.array([-2, 0], dtype=np.int32), w, counts, vol), "group_of_cell[0] = -2 is outside -1 to 1"),
             ((2, groups, np.array([0.5, np.inf]), counts, vol), "the weight of cell 1 is not finite"),
             ((2, groups, np.array([np.nan, 0.5]), counts, vol), "the weight of cell 0 is not finite")]
    for args, msg in cases:
        rc, err = call(g, *args)
        assert rc != 0 and who + msg in err, (msg, err)
    rc, err = call(g, 2, groups, w, counts, vol, grid=False)
    assert rc != 0 and "null grid" in err
    # good arguments of its own: the pass's first refusal on a host-only grid, with and without weights
    for wv in ((w, vol), (None, None)):
        rc, err = call(g, 2, groups, wv[0], counts, wv[1])
        assert rc != 0 and who in err and "created without a device context" in err, err
    assert (counts == 0).all() and (vol == 0.0).all()                  # nothing was written


def test_python_wrapper_checks_shapes(host):
    with pytest.raises(ValueError, match="labels"):
        hmg.cell_histogram_groups(None, host, np.zeros(3, dtype=np.int64), emin=0, emax=1)
    with pytest.raises(ValueError, match="labels"):
        hmg.cell_histogram_groups(None, host, np.zeros(2), emin=0, emax=1)             # floats
    with pytest.raises(ValueError, match="weights"):
        hmg.cell_histogram_groups(None, host, np.zeros(2, dtype=np.int64), weights=np.ones(3), emin=0, emax=1)
    # no label >= 0: no group, nothing is called
    lab, counts, vol = hmg.cell_histogram_groups(None, host, np.array([-1, -5]), weights=np.ones(2), emin=0, emax=1)
    assert lab.shape == (0,) and counts.shape == (0, 11) == vol.shape
    lab, counts, vol = hmg.cell_histogram_groups(None, host, np.ma.masked_all(2, dtype=np.int64), emin=0, emax=1)
    assert lab.shape == (0,) and counts.shape == (0, 11) and vol is None


def test_group_sum_statement_on_three_cells():
    """weights 0.1, 0.7, 1e-3; column 0 (counts 3, 1, 7): ascending cell order gives ...6e9, the reversed order ...6ea;
    column 2 (counts 1, 3, 1 000 003): separately rounded product and sum give ...8b5, a fused multiply-add ...8b4 (both worked
    out by hand in exact rational arithmetic)."""
    w = np.array([0.1, 0.7, 1e-3])
    counts = np.array([[3, 5, 1], [1, 0, 3], [7, 2, 1000003]], dtype=np.int64)
    one = hmg.api.histogram_group_sum(counts, np.array([0, 0, 0]), 1, w)
    want = [float.fromhex("0x1.01cac083126e9p+0"), float.fromhex("0x1.010624dd2f1aap-1"), float.fromhex("0x1.f519fbe76c8b5p+9")]
    assert one.shape == (1, 3) and one.dtype == np.float64
    assert [x.hex() for x in one[0]] == [x.hex() for x in want]
    assert ((0.0 + 0.1 * 3.0) + 0.7 * 1.0) + 1e-3 * 7.0 == want[0] != ((0.0 + 1e-3 * 7.0) + 0.7 * 1.0) + 0.1 * 3.0
    # two groups, one empty, one cell in none: rows of the cells alone, from 0.0
    two = hmg.api.histogram_group_sum(counts, np.array([2, -1, 0]), 3, w)
    np.testing.assert_array_equal(two[2], 0.0 + w[0] * counts[0].astype(float))
    np.testing.assert_array_equal(two[0], 0.0 + w[2] * counts[2].astype(float))
    np.testing.assert_array_equal(two[1], np.zeros(3))


class FakeContext:
    def __init__(self, **values):
        self.values = dict(values)
        self.log = []

    def counter(self, name):
        return self.values[name]

    def set_option(self, name, value):
        self.log.append((name, value))
        self.values[name] = value


def test_large_cells_restores_all_three_options_when_a_pass_raises():
    names = ("cell_moments_windows", "cell_extrema_windows", OPT)
    ctx = FakeContext(**{names[0]: 0, names[1]: 2, names[2]: 0})
    with pytest.raises(RuntimeError, match="the pass"):
        with driver._large_cells(ctx, True):
            assert [ctx.counter(n) for n in names] == [1, 2, 1]        # at least 1 inside; a caller's 2 stays
            raise RuntimeError("the pass")
    assert [ctx.counter(n) for n in names] == [0, 2, 0]
    ctx = FakeContext(**{n: 0 for n in names})
    with driver._large_cells(ctx, True):
        assert [ctx.counter(n) for n in names] == [1, 1, 1]
    assert [ctx.counter(n) for n in names] == [0, 0, 0]
    ctx.log.clear()
    with driver._large_cells(ctx, False):                              # off: nothing is touched
        pass
    assert ctx.log == []


@pytest.mark.gpu
def test_option_takes_0_1_2_reads_back_and_refuses_3():
    ctx = hmg.Context(0)
    try:
        assert ctx.counter(OPT) == 0 and ctx.counter("cell_histogram_window_launches") == 0
        for value in (1, 2, 0):
            ctx.set_option(OPT, value)
            assert ctx.counter(OPT) == value
            assert ctx.counter("cell_extrema_windows") == 0 and ctx.counter("cell_moments_windows") == 0
        for value in (3, -1):
            with pytest.raises(L.HmgError, match="cell_histogram_windows: 0, 1 or 2"):
                ctx.set_option(OPT, value)
        assert ctx.counter(OPT) == 0
    finally:
        ctx.close()
