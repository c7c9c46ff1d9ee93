"""GPU tests of the per-cell extrema over the fine elements (hmg_cell_extrema, csrc/hmg_extrema.hip) against the CPU statement of
tests/_cell_extrema_form.py (pinned by tests/test_cell_extrema_statement.py).

Shapes: the perturbed 2 x 2 x 2 cube (48 cells, no two congruent) on levels 2 (5 of the 6 simplex shapes), 3, 4 (one wave), 5 (256
threads) and 6 (512 threads, LDS above 48 KB); the perturbed 2 x 2 square (8 cells) on levels 2, 5 and 8; 6 000 cells on level 2,
more than the resident workgroups, so that the cell loop runs; a shrunk grid.
Bounds: maxima and minima within 1e-11 of the largest statement maximum over the cells (the project's bound for the apply; a
minimum may be near zero, so it is measured against the maximum too); counts EQUAL to the statement's, each threshold the midpoint
of the widest gap near the 10 %, 50 %, 90 % and 99 % quantiles of the statement's element values, after an assertion on the
statement alone that no element lies within 1e-9 of the largest value of a threshold."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver, fields
import _cell_extrema_form as X
import _cell_moments_form as F
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
MARGIN = 1e-9


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


MESHES = {"cube": (3, 2, 6), "square": (2, 2, 8), "cube10": (3, 10, 2)}
CASES = [("cube", 2), ("cube", 3), ("cube", 4), ("cube", 5), ("cube", 6), ("square", 2), ("square", 5), ("square", 8)]
_cache = {}


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per mesh: oracle mesh and implicit grid, device grid; per (mesh, level): a consistent random vector, xi, an SPD form and
    the statement's element gradients -- computed once, shared, never changed"""
    def get(name, level):
        O = oracle
        if name not in _cache:
            dim, n, grids = MESHES[name]
            base = X.perturbed_cube(O, dim, n)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            rng = np.random.default_rng(300 + level)
            v = F.consistent_random(O, implicit, level, rng)
            xi = rng.standard_normal(base.dim)
            form = T.random_spd(rng, base.nelements(), base.dim)
            grad = X.element_gradients(O, implicit, level, v)
            for a in (v, xi, form, grad):
                a.setflags(write=False)
            _cache[(name, level)] = (v, xi, form, grad)
        return (base, implicit, g) + _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def check(got, q, thr, what):
    """got = (qmax, qmin, counts) of the device against the statement's element values q and thresholds thr"""
    wmax, wmin, wcounts = X.extrema(q, thr)
    scale = np.abs(wmax).max()
    if len(thr):
        mg = X.margin(q, thr)
        print(f"{what}: no element within {mg:.2e} of a threshold (relative to the largest value)")
        assert mg > MARGIN                                             # (on the statement alone)
    qmax, qmin, counts = got
    e1, e2 = np.abs(qmax - wmax).max() / scale, np.abs(qmin - wmin).max() / scale
    print(f"{what}: max {e1:.2e} min {e2:.2e} of the largest maximum {scale:.3e}; counts differ in "
          f"{int((counts != wcounts).sum())} of {counts.size}")
    assert qmax.shape == wmax.shape and qmin.shape == wmin.shape and counts.shape == wcounts.shape
    assert e1 <= TOL and e2 <= TOL
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(counts, wcounts)


@pytest.mark.parametrize("name,level", CASES)
def test_device_against_the_statement(shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    q = X.element_values(grad, xi, form)
    thr = X.gap_thresholds(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    got = hmg.cell_extrema(dv, g, xi, form, thr)
    check(got, q, thr, f"{name} level {level}")
    assert q.shape[1] == hmg.fine_elements(g, level)
    # the same bits in a second run
    again = hmg.cell_extrema(dv, g, xi, form, thr)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 3), ("square", 5)])
@pytest.mark.parametrize("variant", ["indefinite", "no_form", "no_xi", "diagonal", "nthr0", "nthr8"])
def test_forms_and_threshold_counts(shapes, name, level, variant):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    d = base.dim
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    if variant == "indefinite":
        Q = form - np.einsum("ekk->e", form)[:, None, None] / d * np.eye(d)[None]
        Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
        q = X.element_values(grad, xi, Q)
        assert q.min() < 0.0 < q.max()
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, xi, Q, thr), q, thr, f"{name} level {level} indefinite form")
    elif variant == "no_form":
        q = X.element_values(grad, xi, None)
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, xi, None, thr), q, thr, f"{name} level {level} form None")
    elif variant == "no_xi":
        q = X.element_values(grad, None, form)
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, None, form, thr), q, thr, f"{name} level {level} xi None")
    elif variant == "diagonal":
        diag = np.ascontiguousarray(form[:, np.arange(d), np.arange(d)])
        Q = np.zeros_like(form)
        Q[:, np.arange(d), np.arange(d)] = diag
        q = X.element_values(grad, xi, Q)
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, xi, diag, thr), q, thr, f"{name} level {level} diagonal form")
    elif variant == "nthr0":
        q = X.element_values(grad, xi, form)
        got = hmg.cell_extrema(dv, g, xi, form)
        assert got[2].shape == (base.nelements(), 0)
        check(got, q, [], f"{name} level {level} no thresholds")
    else:
        q = X.element_values(grad, xi, form)
        thr = X.gap_thresholds(q, quantiles=(0.02, 0.10, 0.30, 0.50, 0.70, 0.90, 0.97, 0.995))
        assert thr.shape == (8,)
        check(hmg.cell_extrema(dv, g, xi, form, thr), q, thr, f"{name} level {level} eight thresholds")
    dv.close()


def test_more_cells_than_resident_workgroups(shapes):
    base, implicit, g, v, xi, form, grad = shapes("cube10", 2)
    assert base.nelements() == 6000 > 16 * 256
    q = X.element_values(grad, xi, form)
    thr = X.gap_thresholds(q)
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    check(hmg.cell_extrema(dv, g, xi, form, thr), q, thr, "6000 cells level 2")
    dv.close()


def test_shrunk_grid(oracle, ctx):
    O = oracle
    base = X.perturbed_cube(O, 3, 2)
    level = 3
    implicit = O.ImplicitFineGrid.create(base, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    rng = np.random.default_rng(11)
    v = F.consistent_random(O, implicit, level, rng)
    xi, form = rng.standard_normal(3), T.random_spd(rng, 48, 3)
    q = X.element_values(X.element_gradients(O, implicit, level, v), xi, form)
    thr = X.gap_thresholds(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    full = hmg.cell_extrema(dv, g, xi, form, thr)
    g.shrink(47, base.nodes.shape[0])
    assert g.ncells() == 47
    part = hmg.cell_extrema(dv, g, xi, form[:47], thr)
    for a, b in zip(full, part):
        assert b.shape[0] == 47
        np.testing.assert_array_equal(b, a[:47])                       # the extrema do not see the boundary
    check(part, q[:47], thr, "47 of 48 cells")
    dv.close()
    g.close()


@pytest.mark.parametrize("name,level", [("cube", 2), ("cube", 4), ("cube", 6), ("square", 5), ("square", 8)])
def test_linear_field_and_far_thresholds(oracle, shapes, name, level):
    base, implicit, g, _, xi, form, _ = shapes(name, level)
    gvec = np.array([0.7, -1.3, 0.45])[:base.dim]
    dv = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(oracle, implicit, level, gvec))
    want = np.einsum("k,ekl,l->e", xi + gvec, form, xi + gvec)
    qmax, qmin, counts = hmg.cell_extrema(dv, g, xi, form, [0.5 * want.min(), 2.0 * want.max()])
    e1, e2 = np.abs(qmax - want).max() / want.max(), np.abs(qmin - want).max() / want.max()
    print(f"{name} level {level}: linear field, max {e1:.2e} min {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    # a threshold below the minimum counts every fine element, one above the maximum none
    assert (counts[:, 0] == hmg.fine_elements(g, level)).all()
    assert (counts[:, 1] == 0).all()
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 4), ("cube", 6), ("square", 8)])
def test_the_mean_lies_between_the_extrema(shapes, name, level):
    """against cell_moments on the device: qmin <= sigma_c : G_u(c) / |c| <= qmax"""
    base, implicit, g, v, xi, form, _ = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    qmax, qmin, _ = hmg.cell_extrema(dv, g, xi, form)
    _, gram = hmg.cell_moments(dv, g, xi)
    mean = np.einsum("ekl,ekl->e", form, gram) / fields.cell_volumes(hmg.Mesh(base.nodes, base.elements + 1))
    slack = 1e-10 * np.abs(mean)
    print(f"{name} level {level}: min/mean {np.max(qmin / mean):.3f}, max/mean {np.min(qmax / mean):.3f}")
    assert (qmin <= mean + slack).all() and (mean <= qmax + slack).all()
    dv.close()


def test_allocations_settle(shapes, ctx):
    """the first call on a level uploads its element mask and makes the pool blocks; a second call allocates nothing"""
    base, implicit, g, v, xi, form, _ = shapes("cube", 4)
    dv = hmg.DeviceMatrix(g, 4).from_host(v)
    hmg.cell_extrema(dv, g, xi, form, [1.0, 2.0])
    n0 = ctx.counter("device_allocs")
    hmg.cell_extrema(dv, g, xi, form, [1.0, 2.0])
    assert ctx.counter("device_allocs") == n0
    assert ctx.counter("cell_extrema_kernel_ns") > 0
    dv.close()


# ---- refusals ----

@pytest.mark.parametrize("windows", [0, 1])
def test_level7_is_refused_whatever_the_window_option_says(oracle, ctx, windows):
    base = oracle.hypercube(3, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 7)
    dv = hmg.DeviceMatrix(g, 7)
    prev = ctx.counter("cell_moments_windows")
    ctx.set_option("cell_moments_windows", windows)
    try:
        with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: one cell of level 7 .*does not fit the LDS"):
            hmg.cell_extrema(dv, g)
    finally:
        ctx.set_option("cell_moments_windows", prev)
    # ... and a level that is served goes on working on the same grid
    d2 = hmg.DeviceMatrix(g, 2).from_host(F.linear_interpolant(oracle, oracle.ImplicitFineGrid.create(base, 2), 2, np.ones(3)))
    qmax, qmin, _ = hmg.cell_extrema(d2, g)
    assert np.abs(qmax - 3.0).max() <= 3.0 * TOL and np.abs(qmin - 3.0).max() <= 3.0 * TOL
    for o in (dv, d2, g):
        o.close()


def test_2d_level9_is_refused(oracle, ctx):
    base = oracle.hypercube(2, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 9)
    dv = hmg.DeviceMatrix(g, 9)
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: one cell of level 9 .*does not fit the LDS"):
        hmg.cell_extrema(dv, g)
    dv.close()
    g.close()


def test_bad_arguments_are_refused(oracle, shapes, ctx):
    base, implicit, g, v, xi, form, _ = shapes("cube", 2)
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    # a host-only grid
    gh = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: .*without a device context"):
        hmg.cell_extrema(dv, gh)
    gh.close()
    # a vector of another grid
    g2 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: .*another grid"):
        hmg.cell_extrema(dv, g2)
    g2.close()
    # nine thresholds, a NaN threshold, a NaN in the form
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: 9 thresholds"):
        hmg.cell_extrema(dv, g, thresholds=np.arange(9.0))
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: threshold 1 is not finite"):
        hmg.cell_extrema(dv, g, thresholds=[1.0, np.nan])
    bad = form.copy()
    bad[5, 1, 1] = np.inf
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: the form of cell 5 is not finite"):
        hmg.cell_extrema(dv, g, form=bad)
    # null thresholds with nthr > 0, null vector: the C entry point itself
    L = hmg._lib
    out = np.zeros((g.ncells(), 3))
    assert L.load().hmg_cell_extrema(g.h, dv.h, None, None, 1, None, out.ctypes.data_as(L.p_f64)) != 0
    assert "hmg_cell_extrema: null thresholds" in L.load().hmg_last_error().decode()
    assert L.load().hmg_cell_extrema(g.h, None, None, None, 0, None, out.ctypes.data_as(L.p_f64)) != 0
    assert "hmg_cell_extrema: null vector" in L.load().hmg_last_error().decode()
    # ... and the next call succeeds
    check(hmg.cell_extrema(dv, g, xi, form), X.element_values(shapes("cube", 2)[6], xi, form), [], "after the refusals")
    dv.close()


# ---- the Dirichlet driver ----

def test_driver_uniform_medium(ctx):
    xi = np.array([0.6, 0.8])
    r = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, ctx=ctx, sigma_grid=np.full((3, 3, 2), 3.0), extrema=True,
                                        thresholds=[0.5, 2.0], fields=True)
    print("uniform medium: concentration", r["concentration"].min(), r["concentration"].max())
    assert np.abs(r["concentration"] - 1.0).max() <= 1e-10
    np.testing.assert_allclose(r["exceedance"][:, 0], r["volumes"], rtol=1e-14)     # above half the mean: the whole volume
    assert (r["exceedance"][:, 1] == 0.0).all()                                      # above twice the mean: nothing


def test_driver_checkerboard(ctx):
    xi = np.array([0.6, 0.8])
    kw = dict(ctx=ctx, seed=2, values=(1.0, 9.0))
    plain = driver.dirichlet_homogenization(2, hmg.Tri64, 3, xi, fields=True, **kw)
    r = driver.dirichlet_homogenization(2, hmg.Tri64, 3, xi, fields=True, extrema=True, thresholds=[1.0, 4.0], **kw)
    new = {"peak_energy_density", "min_energy_density", "concentration", "exceedance"}
    assert set(r) == set(plain) | new and not (set(plain) & new)
    for k in plain:                                                   # the dict without `extrema` is unchanged
        if k != "base":
            np.testing.assert_array_equal(np.asarray(plain[k]), np.asarray(r[k]))
    ne = r["volumes"].shape[0]
    assert r["peak_energy_density"].shape == (ne,) and r["exceedance"].shape == (ne, 2)
    dens = r["energy"] / r["volumes"]
    slack = 1e-10 * dens
    assert (r["peak_energy_density"] + slack >= dens).all() and (dens + slack >= r["min_energy_density"]).all()
    np.testing.assert_allclose(r["concentration"], r["peak_energy_density"] / r["energy_form"], rtol=1e-14)
    assert (r["exceedance"] >= 0.0).all() and (r["exceedance"] <= r["volumes"][:, None] * (1 + 1e-14)).all()
    assert (r["exceedance"][:, 1] <= r["exceedance"][:, 0]).all()
    print("checkerboard: concentration up to", r["concentration"].max(), "exceedance", r["exceedance"].sum(axis=0) / r["volume"])
    without = driver.dirichlet_homogenization(2, hmg.Tri64, 3, xi, extrema=True, **kw)
    assert "exceedance" not in without and "peak_energy_density" in without
