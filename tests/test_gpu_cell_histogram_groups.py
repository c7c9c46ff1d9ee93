"""GPU tests of the per-cell histograms summed over groups of cells on the device (hmg_cell_histogram_groups, k_histogram_groups of
csrc/hmg_histogram.hip; api.cell_histogram_groups).

Shapes: the perturbed 2 x 2 x 2 cube on level 3 (48 cells, the LDS kernel), 6 000 cells on level 2 (more cells than resident
workgroups, groups of about 1 500 cells), and the perturbed unit cube on level 7 (6 cells) through the window kernels.  The
vector is random, taken as stored; xi random, the form T.random_spd; the rule 13 octaves below the median of the cells' maxima.
Labels: unsorted and interleaved, three groups (labels 7, 2 and 40, cell after cell) and every fifth cell in no group (label -1);
through the C entry point a fourth, empty group as well.
  * counts EQUAL np.add.at over api.cell_histogram's rows;
  * volume EQUALS, bit for bit, api.histogram_group_sum -- the numpy statement of the documented order (per group the cells by
    ascending cell id, from 0.0, product and sum rounded separately; pinned by tests/test_cell_histogram_window_host.py) -- and
    the bits of a second run and of another context;
  * volume agrees with fields.histogram_volume(labels=...) to 1e-13 of the row's largest entry: that function sums in another
    order (a dot product), so only to rounding;
  * without weights volume is None.
The int64 sums beyond 2^31 cannot be reached at a test's size (DESIGN section 4 says so)."""
import contextlib

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import fields
import _cell_extrema_form as X
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
OPT, XOPT = "cell_histogram_windows", "cell_extrema_windows"
# name: dim, n, level, window option
SHAPES = {"cube": (3, 2, 3, 0), "cube10": (3, 10, 2, 0), "cube7": (3, 1, 7, 1)}
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    assert c.counter(OPT) == 0 and c.counter(XOPT) == 0
    c.close()


@contextlib.contextmanager
def option(ctx, name, value):
    prev = ctx.counter(name)
    ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, prev)


class Shape:
    def __init__(self, O, ctx, name):
        dim, n, level, self.window = SHAPES[name]
        base = X.perturbed_cube(O, dim, n)
        self.mesh = hmg.Mesh(base.nodes, base.elements + 1)
        self.level, self.ne = level, base.nelements()
        self.g = hmg.ImplicitFineGrid(ctx, self.mesh, level)
        rng = np.random.default_rng(900 + level)
        self.v = np.asfortranarray(rng.standard_normal((self.g.nf(level), self.ne)))
        self.xi, self.form = rng.standard_normal(dim), T.random_spd(rng, self.ne, dim)
        self.labels = np.array([7, 2, 40])[(2 * np.arange(self.ne) + 1) % 3]     # 2, 7, 40, 2, ... : no label in one run
        self.labels[::5] = -1
        self.nel = hmg.fine_elements(self.g, level)
        self.vol = fields.cell_volumes(self.mesh)
        self.w = self.vol / float(self.nel)
        self.dv = hmg.DeviceMatrix(self.g, level).from_host(self.v)
        with option(ctx, XOPT, self.window):
            qmax, _, _ = hmg.cell_extrema(self.dv, self.g, self.xi, self.form)
        top = int(np.ceil(np.log2(np.median(qmax))))
        self.kw = dict(emin=top - 13, emax=top, sub_bits=3)
        with option(ctx, OPT, self.window):
            self.rows = hmg.cell_histogram(self.dv, self.g, self.xi, self.form, **self.kw)
        for a in (self.v, self.xi, self.form, self.labels, self.w, self.rows):
            a.setflags(write=False)

    def close(self):
        self.dv.close()
        self.g.close()


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per shape: grid, vector, xi, form, labels, weights and api.cell_histogram's rows -- made once, shared, never changed"""
    def get(name):
        if name not in _cache:
            _cache[name] = Shape(oracle, ctx, name)
        return _cache[name]
    yield get
    for s in _cache.values():
        s.close()
    _cache.clear()


def group_ids(labels):
    lab = np.unique(labels[labels >= 0])
    return lab, np.where(labels >= 0, np.searchsorted(lab, labels), -1)


@pytest.mark.parametrize("name", list(SHAPES))
def test_groups_against_the_rows_and_the_statement(ctx, shapes, name):
    s = shapes(name)
    want_labels, gid = group_ids(s.labels)
    assert list(want_labels) == [2, 7, 40] and (gid == -1).sum() >= s.ne // 5
    want_counts = np.zeros((3, s.rows.shape[1]), dtype=np.int64)
    np.add.at(want_counts, gid[gid >= 0], s.rows[gid >= 0])
    want_volume = hmg.api.histogram_group_sum(s.rows, gid, 3, s.w)
    with option(ctx, OPT, s.window):
        l0, w0 = ctx.counter("cell_histogram_launches"), ctx.counter("cell_histogram_window_launches")
        labels, counts, volume = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, **s.kw)
        assert ctx.counter("cell_histogram_launches") == l0 + 1
        assert ctx.counter("cell_histogram_window_launches") == w0 + s.window
        assert ctx.counter("cell_histogram_groups_kernel_ns") > 0 and ctx.counter("cell_histogram_kernel_ns") > 0
        np.testing.assert_array_equal(labels, want_labels)
        assert counts.shape == want_counts.shape and counts.dtype == np.int64
        assert volume.shape == want_volume.shape and volume.dtype == np.float64
        np.testing.assert_array_equal(counts, want_counts)
        assert (counts.sum(axis=1) == np.bincount(gid[gid >= 0], minlength=3) * s.nel).all()
        assert (counts[:, 1:-2] > 0).sum() > 12                        # (the rule resolves something)
        diff = int((volume != want_volume).sum())
        print(f"{name}: {diff} of {volume.size} volumes differ from the statement in the documented order")
        assert volume.tobytes() == want_volume.tobytes()
        # another order of summation: to rounding
        byl = fields.histogram_volume(s.rows, s.vol, s.nel, labels=s.labels)
        for k, lab in enumerate(labels):
            err = np.abs(volume[k] - byl[int(lab)]).max() / np.abs(byl[int(lab)]).max()
            print(f"{name}: label {lab}: {err:.2e} from fields.histogram_volume")
            assert err <= 1e-13
        # a second run: the same bits, nothing allocated; without weights: the same counts, no volume
        a0 = ctx.counter("device_allocs")
        _, c2, v2 = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, **s.kw)
        assert ctx.counter("device_allocs") == a0
        assert c2.tobytes() == counts.tobytes() and v2.tobytes() == volume.tobytes()
        l3, c3, v3 = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, **s.kw)
        assert v3 is None
        np.testing.assert_array_equal(l3, labels)
        np.testing.assert_array_equal(c3, counts)


@pytest.mark.parametrize("name", ["cube", "cube7"])
def test_another_context_gives_the_same_bits(ctx, shapes, name):
    s = shapes(name)
    with option(ctx, OPT, s.window):
        _, counts, volume = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, **s.kw)
    other = hmg.Context(0)
    try:
        other.set_option(OPT, s.window)
        g = hmg.ImplicitFineGrid(other, s.mesh, s.level)
        dv = hmg.DeviceMatrix(g, s.level).from_host(s.v)
        _, c2, v2 = hmg.cell_histogram_groups(dv, g, s.labels, s.xi, s.form, s.w, **s.kw)
        assert c2.tobytes() == counts.tobytes() and v2.tobytes() == volume.tobytes()
        dv.close()
        g.close()
    finally:
        other.close()


def test_an_empty_group_and_masked_labels(ctx, shapes):
    """the C entry point with four groups of which one has no cell: its rows are zeros, the others as before; a masked label is a
    cell in no group, as a negative one"""
    s = shapes("cube")
    L = hmg._lib
    lib = L.load()
    _, gid3 = group_ids(s.labels)
    gid = np.where(gid3 >= 2, 3, gid3).astype(np.int32)                # groups 0, 1, 3; group 2 is empty
    nb = s.rows.shape[1]
    counts, volume = np.full((4, nb), -1, dtype=np.int64), np.full((4, nb), np.nan)
    packed = hmg.api._packed_form(s.form, s.ne, 3)
    xi = np.ascontiguousarray(s.xi)
    w = np.ascontiguousarray(s.w)
    L.check(lib.hmg_cell_histogram_groups(s.g.h, s.dv.h, xi.ctypes.data_as(L.p_f64), packed.ctypes.data_as(L.p_f64), s.kw["emin"],
                                          s.kw["emax"], s.kw["sub_bits"], 4, gid.ctypes.data_as(L.p_i32), w.ctypes.data_as(L.p_f64),
                                          counts.ctypes.data_as(L.p_i64), volume.ctypes.data_as(L.p_f64)))
    assert (counts[2] == 0).all() and (volume[2] == 0.0).all() and not np.signbit(volume[2]).any()
    _, c3, v3 = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, **s.kw)
    np.testing.assert_array_equal(counts[[0, 1, 3]], c3)
    assert volume[[0, 1, 3]].tobytes() == v3.tobytes()
    assert volume.tobytes() == hmg.api.histogram_group_sum(s.rows, gid, 4, s.w).tobytes()
    # masked labels
    masked = np.ma.masked_array(np.where(s.labels < 0, 7, s.labels), mask=s.labels < 0)
    lm, cm, vm = hmg.cell_histogram_groups(s.dv, s.g, masked, s.xi, s.form, s.w, **s.kw)
    np.testing.assert_array_equal(lm, [2, 7, 40])
    assert cm.tobytes() == c3.tobytes() and vm.tobytes() == v3.tobytes()


def test_refusals_launch_nothing_and_the_context_goes_on(ctx, shapes):
    s = shapes("cube")
    L = hmg._lib
    l0 = ctx.counter("cell_histogram_launches")
    bad = np.array(s.w)
    bad[3] = np.nan
    with pytest.raises(L.HmgError, match="hmg_cell_histogram_groups: the weight of cell 3 is not finite"):
        hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, bad, **s.kw)
    # what the pass itself refuses carries this call's name: a rule with too many bins, a level that needs the window option
    with pytest.raises(L.HmgError, match="hmg_cell_histogram_groups: 1056 regular bins"):
        hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, emin=0, emax=33, sub_bits=5)
    big = shapes("cube7")
    with pytest.raises(L.HmgError, match="hmg_cell_histogram_groups: one cell of level 7 .*does not fit the LDS") as err:
        hmg.cell_histogram_groups(big.dv, big.g, big.labels, big.xi, big.form, big.w, **big.kw)
    assert OPT in str(err.value)
    assert ctx.counter("cell_histogram_launches") == l0
    _, counts, _ = hmg.cell_histogram_groups(s.dv, s.g, s.labels, s.xi, s.form, s.w, **s.kw)
    assert counts.sum() == (s.labels >= 0).sum() * s.nel
    assert ctx.counter("cell_histogram_launches") == l0 + 1
