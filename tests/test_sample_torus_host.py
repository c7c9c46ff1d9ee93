"""Host side of sampling on a periodic grid (include/hmg.h: hmg_grid_set_periodic_sampling, then hmg_grid_locate), without a GPU,
on host-only grids, against the numpy statement of tests/_sample_torus_form.py: interior points by construction (cells that wrap
included) at _sample_form's bounds; the same points moved by whole periods, and the same torus with its node representatives moved
by whole periods, bit for bit; every fine node and every coarse face, the faces across the seam included, by the lowest-cell rule;
the bin lists against a brute-force search; NaN and inf; the switch and its refusals; and an ordinary grid's locate against the
bits the commit before this feature gave (tests/golden/ordinary_locate_parent.npz)."""
import ctypes
import os

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L

import _periodic_form as P
import _sample_torus_form as T

F = T.F
CASES = [(name, level) for name in sorted(T.CASES) for level in T.CASES[name][2]]
REFUSAL = "periodic grids are not served (point location on a torus is not built)"      # today's message, to the letter
_grids = {}
_fine = {}


@pytest.fixture(scope="module")
def host():
    def get(name, shift=False):
        if (name, shift) not in _grids:
            g = hmg.ImplicitFineGrid(None, T.mesh(name, shift), T.CASES[name][1])
            g.set_periodic_sampling(True)
            _grids[(name, shift)] = g
        return _grids[(name, shift)]
    yield get
    for g in _grids.values():
        g.close()
    _grids.clear()
    _fine.clear()


def fine(g, name, level):
    if (name, level) not in _fine:
        _fine[(name, level)] = T.TorusFineMesh(g, level)
    return _fine[(name, level)]


def same(a, b):
    return all(p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == "f") for p, q in zip(a, b))


@pytest.mark.parametrize("name,level", CASES)
def test_locate_against_the_statement(host, name, level):
    g = host(name)
    fm0 = fine(g, name, level)
    d = fm0.dim
    pts = fm0.interior_points(400, seed=100 + level)
    fm = fm0.scope(pts["x"])
    box = ((pts["x"] < 0) | (pts["x"] >= fm.period)).any(axis=1)
    assert box.any() and (~box).any()                           # cells that wrap put points past the box
    cell, nodes, w, gw = hmg.locate(g, level, pts["x"])
    assert np.array_equal(cell, pts["cell"])
    o_lib, o_ref = np.argsort(nodes, axis=1), np.argsort(pts["nodes"], axis=1)
    assert np.array_equal(np.take_along_axis(nodes, o_lib, 1), np.take_along_axis(pts["nodes"], o_ref, 1))
    err_w = np.abs(np.take_along_axis(w, o_lib, 1) - np.take_along_axis(pts["weights"], o_ref, 1)).max()
    g_lib = np.take_along_axis(gw, o_lib[:, :, None], 1)
    err_g = np.abs(g_lib - np.take_along_axis(pts["grads"], o_ref[:, :, None], 1)).max()
    print(f"{name} level {level}: weights {err_w:.3e} (bound {fm.T_w():.3e}), gweights {err_g:.3e} (bound {fm.T_gradient(1.0):.3e})")
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() <= 4 * F.EPS
    assert err_w <= fm.T_w()
    assert err_g <= fm.T_gradient(1.0)
    assert w.shape == (400, d + 1) and gw.shape == (400, d + 1, d)


@pytest.mark.parametrize("name,level", CASES)
def test_whole_periods_and_moved_representatives_change_no_bit(host, name, level):
    g = host(name)
    fm = fine(g, name, level)
    x = T.quantized(fm.interior_points(400, seed=200 + level)["x"])
    here = hmg.locate(g, level, x)
    assert np.array_equal(here[0], fm.interior_points(400, seed=200 + level)["cell"])
    # the same points whole periods away: cell, nodes and weights (and the gradient weights, which belong to the element)
    xs = T.whole_period_shifts(x, fm.period, seed=300 + level)
    assert (np.abs(xs - x).max(axis=0) >= 2 * fm.period).all()
    assert same(hmg.locate(g, level, xs), here)
    # the same torus with its node representatives moved by whole periods: the box is the period's, not the nodes'
    gs = host(name, shift=True)
    assert not np.array_equal(gs.base.nodes, g.base.nodes)
    assert np.array_equal(P.keys(gs.base.nodes, fm.period, 1, P.DEN), P.keys(g.base.nodes, fm.period, 1, P.DEN))
    assert same(hmg.locate(gs, level, x), here)
    assert same(hmg.locate(gs, level, xs), here)


@pytest.mark.parametrize("name,level", [("torus2", 3), ("torus3", 3)])
def test_every_fine_node_goes_to_the_lowest_cell(host, name, level):
    g = host(name)
    fm = fine(g, name, level)
    x, lowest = fm.node_points()
    cell, nodes, w, gw = hmg.locate(g, level, x)
    assert np.array_equal(cell, lowest)                         # the lowest cell that has a node there modulo the period
    assert (np.abs(w.max(axis=1) - 1.0) <= fm.T_w()).all() and (w >= 0).all() and np.isfinite(gw).all()
    top = np.take_along_axis(nodes, w.argmax(axis=1)[:, None], 1)[:, 0]
    ids, n = P.fine_ids(g, level, P.DEN)                         # (nf, ne): torus fine node behind (hierarchical node, cell)
    asked = ids.T.ravel()                                        # x is cell-major
    assert np.array_equal(ids[top, cell], asked)                 # the vertex that carries the point is that torus node
    assert np.unique(asked).size == n


@pytest.mark.parametrize("name,level", [("torus2", 3), ("torus3", 1)])
def test_coarse_faces_go_to_the_lower_cell(host, name, level):
    g = host(name)
    fm = fine(g, name, level)
    x, want = fm.coarse_face_points(6, seed=9)
    own = np.tile(np.repeat(np.arange(fm.ne), 6), fm.dim + 1)
    assert (want < own).any() and (want == own).any()            # asked from both sides
    cell = hmg.locate(g, level, x)[0]
    assert np.array_equal(cell, want)
    # across the seam: the cell that wins stores that face whole periods away from where the point was formed
    far = np.abs(fm.Xc[want].mean(axis=1) - fm.Xc[own].mean(axis=1)).max(axis=1) > 0.5 * fm.period.min()
    assert far.any()


@pytest.mark.parametrize("name,seed", [("torus2", 1), ("torus3", 1)])
def test_the_lists_are_never_short(host, name, seed):
    """10^5 random points over four periods per axis against a brute-force search of all cells by the minimal image.  The
    condition on the seed: no point within 1e-9 of any face plane of any cell, in barycentric terms."""
    g = host(name)
    fm = fine(g, name, 1)
    x = np.ascontiguousarray((np.random.default_rng(seed).random((100000, fm.dim)) * 4.0 - 1.5) * fm.period)
    want, margin = fm.brute_force_cells(x)
    assert margin >= 1e-9, margin
    for gg in (g, host(name, shift=True)):
        cell = hmg.locate(gg, 1, x)[0]
        assert (cell >= 0).all()
        assert np.array_equal(cell, want)
    assert np.unique(want).size == fm.ne


def test_nan_and_inf(host):
    for name in sorted(T.CASES):
        g = host(name)
        d = g.base.dim
        bad = np.full((4, d), 0.25)
        bad[0, 0] = np.nan
        bad[1, -1] = np.inf
        bad[2, 0] = -np.inf
        bad[3, :] = np.nan
        cell, nodes, w, gw = hmg.locate(g, 2, bad)
        assert (cell == -1).all() and (nodes == -1).all() and np.isnan(w).all() and np.isnan(gw).all()
        assert (hmg.locate(g, 2, np.full((1, d), 0.25))[0] >= 0).all()
        assert (hmg.locate(g, 2, np.full((1, d), -1e6))[0] >= 0).all()      # no finite point is outside


def test_the_switch():
    lib = L.load()
    g = hmg.ImplicitFineGrid(None, T.mesh("torus2"), 2)
    o = hmg.ImplicitFineGrid(None, hmg.Mesh(g.base.nodes, g.base.elements[:1]), 2)          # one cell, not periodic
    try:
        x = np.array([[0.3, 0.2]])
        cell = np.zeros(1, dtype=np.int32)
        val = np.zeros(1)
        px, pc, pv = x.ctypes.data_as(L.p_f64), cell.ctypes.data_as(L.p_i32), val.ctypes.data_as(L.p_f64)
        calls = {"hmg_grid_locate": lambda: lib.hmg_grid_locate(g.h, 2, 1, px, pc, None, None, None),
                 "hmg_sample": lambda: lib.hmg_sample(g.h, 2, None, None, 1, px, pv, None, None),
                 "hmg_sample_raster": lambda: lib.hmg_sample_raster(g.h, 2, None, None, px, px, px, 1, 1, pv, None, None)}

        def refused_as_today():
            for name, call in calls.items():
                assert call() != 0
                assert lib.hmg_last_error().decode() == f"{name}: {REFUSAL}"

        assert g.periodic_sampling() is False                    # off by default
        builds = hmg.locator_counter("sample_locator_builds")
        refused_as_today()
        g.set_periodic_sampling(True)
        assert g.periodic_sampling() is True
        assert hmg.locator_counter("sample_locator_builds") == builds          # the switch builds nothing
        first = hmg.locate(g, 2, x)
        assert first[0][0] >= 0 and hmg.locator_counter("sample_locator_builds") == builds + 1
        hmg.locate(g, 2, x)
        assert hmg.locator_counter("sample_locator_builds") == builds + 1
        # the device calls on a grid without a context say so, as on any grid
        assert calls["hmg_sample"]() != 0 and "without a device context" in lib.hmg_last_error().decode()
        assert calls["hmg_sample_raster"]() != 0 and "without a device context" in lib.hmg_last_error().decode()
        g.set_periodic_sampling(False)
        assert g.periodic_sampling() is False
        refused_as_today()
        g.set_periodic_sampling(True)                            # toggling drops the locator
        assert same(hmg.locate(g, 2, x), first) and hmg.locator_counter("sample_locator_builds") == builds + 2
        # values other than 0 and 1, a null result, a null grid
        for bad in (2, -1):
            assert lib.hmg_grid_set_periodic_sampling(g.h, bad) != 0
            assert "hmg_grid_set_periodic_sampling" in lib.hmg_last_error().decode()
        assert g.periodic_sampling() is True
        assert lib.hmg_grid_periodic_sampling(g.h, None) != 0 and "hmg_grid_periodic_sampling" in lib.hmg_last_error().decode()
        on = ctypes.c_int(7)
        assert lib.hmg_grid_set_periodic_sampling(None, 1) != 0 and lib.hmg_grid_periodic_sampling(None, ctypes.byref(on)) != 0
        # an ordinary grid: refused with the call's name, and its flag reads 0
        for v in (0, 1):
            assert lib.hmg_grid_set_periodic_sampling(o.h, v) != 0
            msg = lib.hmg_last_error().decode()
            assert "hmg_grid_set_periodic_sampling" in msg and "not periodic" in msg, msg
        with pytest.raises(L.HmgError, match="hmg_grid_set_periodic_sampling"):
            o.set_periodic_sampling(True)
        assert o.periodic_sampling() is False
        assert hmg.locate(o, 2, g.base.nodes[g.base.elements[0] - 1].mean(axis=0)[None, :])[0][0] == 0
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("name", ["tri", "tet"])
def test_an_ordinary_grid_keeps_its_bits(name):
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordinary_locate_parent.npz"))
    got = T.ordinary_locate(name)
    assert (got["cell"] >= 0).any() and (got["cell"] < 0).any()
    for key, val in got.items():
        ref = gold[f"{name}_{key}"]
        assert val.dtype == ref.dtype and val.shape == ref.shape
        assert np.array_equal(val, ref, equal_nan=val.dtype.kind == "f"), key
