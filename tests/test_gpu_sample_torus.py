"""Sampling on a periodic grid on the device (include/hmg.h: hmg_grid_set_periodic_sampling, then hmg_sample and
hmg_sample_raster; k_sample_torus) against the host's hmg_grid_locate and the numpy statement of tests/_sample_torus_form.py:
the device's cell on every point set of the host tests, values and gradients of a vector laid out by position, xi . x at the
caller's point periods away, rasters over several periods against point lists and against themselves one period on, the periodic
tensor driver's slices on a laminate, and allocations.  Bounds: the formulas of _sample_form.py with X grown to the points asked."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver, fields

import _sample_torus_form as T

F = T.F
pytestmark = pytest.mark.gpu

LEVELS = {"torus2": 9, "torus3": 7}
_grids = {}
_fine = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    for g in _grids.values():
        g.close()
    _grids.clear()
    _fine.clear()
    c.close()


@pytest.fixture(scope="module")
def grid(ctx):
    def get(name):
        if name not in _grids:
            g = hmg.ImplicitFineGrid(ctx, T.mesh(name), LEVELS[name])
            g.set_periodic_sampling(True)
            _grids[name] = g
        return _grids[name]
    return get


def fine(g, name, level):
    if (name, level) not in _fine:
        _fine[(name, level)] = T.TorusFineMesh(g, level, explicit=not (name == "torus3" and level >= 6))
    return _fine[(name, level)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- 1. one text: the device's cell is the host's on every point set of the host tests ------------------------------------------
@pytest.mark.parametrize("name", ["torus2", "torus3"])
def test_the_device_finds_the_hosts_cell(grid, name):
    g = grid(name)
    level = 3
    fm = fine(g, name, level)
    d = fm.dim
    inner = T.quantized(fm.interior_points(400, seed=200 + level)["x"])
    bad = np.full((3, d), 0.25)
    bad[0, 0], bad[1, -1], bad[2, 0] = np.nan, np.inf, -np.inf
    sets = {"interior": fm.interior_points(400, seed=100 + level)["x"],
            "periods away": T.whole_period_shifts(inner, fm.period, seed=300 + level),
            "fine nodes": fm.node_points()[0],
            "coarse faces": fm.coarse_face_points(6, seed=9)[0],
            "random": np.ascontiguousarray((np.random.default_rng(1).random((100000, d)) * 4.0 - 1.5) * fm.period),
            "not finite": bad}
    v = hmg.DeviceMatrix(g, level)
    try:
        for what, x in sets.items():
            cell = hmg.locate(g, level, x)[0]
            s = hmg.sample(v, g, x, value=False, gradient=False)
            assert same(s["cell"], cell), what
            assert (cell >= 0).all() or what == "not finite"
        assert (hmg.sample(v, g, bad)["cell"] == -1).all() and np.isnan(hmg.sample(v, g, bad)["value"]).all()
        assert np.isnan(hmg.sample(v, g, bad)["gradient"]).all()
    finally:
        v.close()


# ---- 2. values and gradients of a vector laid out by position -------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("torus2", 1), ("torus2", 5), ("torus2", 9), ("torus3", 1), ("torus3", 4), ("torus3", 6),
                                        ("torus3", 7)])
def test_values_and_gradients_against_the_statement(grid, name, level):
    g = grid(name)
    fm0 = fine(g, name, level)
    d = fm0.dim
    xh = fm0.nodal_vector(seed=40 + level)                       # one normal value per torus fine node: the copies agree
    vmax = float(np.abs(xh).max())
    pts = fm0.interior_points(400, seed=100 + level)
    k = np.random.default_rng(50 + level).integers(-3, 4, size=pts["x"].shape).astype(np.float64)
    x = np.ascontiguousarray(np.concatenate([pts["x"], pts["x"] + k * fm0.period]))       # ... and whole periods away
    fm = fm0.scope(x)
    vals = np.tile(xh[pts["nodes"], pts["cell"][:, None]], (2, 1))                        # (n, d + 1)
    ref_v = (np.tile(pts["weights"], (2, 1)) * vals).sum(axis=1)
    ref_g = np.einsum("nk,nkc->nc", vals, np.tile(pts["grads"], (2, 1, 1)))
    xi = np.array([0.3, -1.7, 0.9][:d])
    v = hmg.DeviceMatrix(g, level)
    try:
        v.from_host(xh)
        for use_xi in (None, xi):
            s = hmg.sample(v, g, x, xi=use_xi)
            assert np.array_equal(s["cell"], np.tile(pts["cell"], 2))
            want_v = ref_v if use_xi is None else ref_v + x @ xi
            want_g = ref_g if use_xi is None else ref_g + xi
            err_v, err_g = np.abs(s["value"] - want_v).max(), np.abs(s["gradient"] - want_g).max()
            print(f"{name} level {level} xi {use_xi is not None}: value {err_v:.3e} (bound {fm.T_value(vmax, use_xi):.3e}), "
                  f"gradient {err_g:.3e} (bound {fm.T_gradient(vmax, use_xi):.3e})")
            assert err_v <= fm.T_value(vmax, use_xi)
            assert err_g <= fm.T_gradient(vmax, use_xi)
    finally:
        v.close()


# ---- 3. v = 0: xi . x of the caller's point, periods away -----------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("torus2", 4), ("torus3", 3)])
def test_xi_dot_x_is_taken_at_the_callers_point(grid, name, level):
    g = grid(name)
    fm = fine(g, name, level)
    d = fm.dim
    x0 = fm.interior_points(400, seed=7)["x"]
    k = np.random.default_rng(8).integers(-3, 4, size=x0.shape).astype(np.float64)
    x = np.ascontiguousarray(x0 + k * fm.period)
    assert (np.abs(k).max(axis=0) == 3).all()
    xi = np.array([0.3, -1.7, 0.9][:d])
    v = hmg.DeviceMatrix(g, level)                               # zeros
    try:
        s = hmg.sample(v, g, x, xi=xi)
        X = fm.scope(x).X
        err = np.abs(s["value"] - x @ xi).max()
        print(f"{name}: |value - xi . x| {err:.3e} (bound {8 * F.EPS * np.abs(xi).sum() * X:.3e})")
        assert err <= 8 * F.EPS * np.abs(xi).sum() * X
        assert np.array_equal(s["gradient"], np.broadcast_to(xi, x.shape))
        assert np.array_equal(s["cell"], fm.interior_points(400, seed=7)["cell"])
    finally:
        v.close()


# ---- 4. rasters over several periods ---------------------------------------------------------------------------------------------
# dyadic origins and steps: the device's fmas are exact, and so is numpy's origin + a du + b dv.  The periods: torus2 (8, 3 / 2),
# torus3 (6, 3 / 2, 3).  The first raster of each spans 2.5 periods both ways and crosses the seam; 64 (2D: 64 and 48) pixels on
# is a whole number of periods on.
RASTERS = {
    "torus2": (5, [((-3.0 + 1 / 64, -0.5 + 1 / 128), (1 / 8, 0.0), (0.0, 1 / 32), 160, 120, (64, 48)),       # axis-aligned
                   ((-1.0, 0.25 + 1 / 64), (1 / 16, 0.0), (0.0, 1 / 32), 300, 1, None),
                   ((7.5, -1.0), (1 / 16, 1 / 128), (1 / 64, 1 / 32), 1, 300, None),
                   ((-0.5 + 1 / 64, 1.0), (1 / 4, 0.0), (0.0, 1 / 8), 5, 40, None)]),
    "torus3": (4, [((-2.0 + 1 / 64, -0.25, 1 / 128), (3 / 32, 3 / 128, 0.0), (0.0, 3 / 128, 3 / 64), 160, 160, (64, 64)),   # oblique
                   ((-1.0, 0.25, 2.75 + 1 / 64), (1 / 16, 0.0, 1 / 256), (0.0, 1 / 64, 0.0), 300, 1, None),
                   ((5.5, -1.0, 0.5), (1 / 64, 0.0, 0.0), (1 / 128, 1 / 64, 1 / 32), 1, 300, None),
                   ((-0.5 + 1 / 64, 1.0, -0.25), (1 / 4, 0.0, 1 / 64), (0.0, 1 / 8, 0.0), 5, 40, None)]),
}


@pytest.mark.parametrize("name", sorted(RASTERS))
def test_rasters_tile_and_equal_the_point_list(grid, name):
    g = grid(name)
    level, rasters = RASTERS[name]
    fm = fine(g, name, level)
    d = fm.dim
    v = hmg.DeviceMatrix(g, level)
    try:
        xh = fm.nodal_vector(seed=6)
        v.from_host(xh)
        vmax = float(np.abs(xh).max())
        xi = np.array([1.0, -2.0, 0.5][:d])
        for origin, du, dv, nu, nv, period_in_pixels in rasters:
            a = np.arange(nu, dtype=np.float64)[None, :, None]
            b = np.arange(nv, dtype=np.float64)[:, None, None]
            x = (np.asarray(origin) + a * np.asarray(du) + b * np.asarray(dv)).reshape(-1, d)
            for use_xi in (xi, None):
                r = hmg.sample_raster(v, g, origin, du, dv, nu, nv, xi=use_xi)
                p = hmg.sample(v, g, x, xi=use_xi)
                assert r["value"].shape == (nv, nu) and r["gradient"].shape == (nv, nu, d) and r["cell"].shape == (nv, nu)
                assert same(r["value"].ravel(), p["value"]) and same(r["cell"].ravel(), p["cell"])
                assert same(r["gradient"].reshape(-1, d), p["gradient"])
                assert (r["cell"] >= 0).all() and np.isfinite(r["value"]).all() and np.isfinite(r["gradient"]).all()
                r2 = hmg.sample_raster(v, g, origin, du, dv, nu, nv, xi=use_xi, gradient=False)
                assert "gradient" not in r2 and same(r2["value"], r["value"]) and same(r2["cell"], r["cell"])
            if period_in_pixels is None:
                continue
            pa, pb = period_in_pixels
            span = (nu - 1) * np.abs(du) + (nv - 1) * np.abs(dv)
            assert (span[:2] >= 2.4 * fm.period[:2]).all()
            assert ((x.min(axis=0) < 0) & (x.max(axis=0) > fm.period))[:2].all()         # across the seam, both sides
            whole = (pa * np.asarray(du)) / fm.period, (pb * np.asarray(dv)) / fm.period
            assert all(np.array_equal(w, np.rint(w)) and np.abs(w).max() == 1 for w in whole)
            # r is the last pass, xi = None: v repeats, to the bit; with xi the value grows by xi . (the shift) and the gradient repeats
            for key in ("value", "gradient", "cell"):
                assert same(r[key][:, pa:], r[key][:, :-pa]), key
                assert same(r[key][pb:, :], r[key][:-pb, :]), key
            rx = hmg.sample_raster(v, g, origin, du, dv, nu, nv, xi=xi)
            assert same(rx["gradient"][:, pa:], rx["gradient"][:, :-pa]) and same(rx["cell"], r["cell"])
            # (two values of at most 7 fmas each, every partial sum within max|v| + |xi|_1 X, and the two subtractions here)
            grow = rx["value"][:, pa:] - rx["value"][:, :-pa] - float(xi @ (pa * np.asarray(du)))
            assert np.abs(grow).max() <= 8 * F.EPS * (vmax + np.abs(xi).sum() * fm.scope(x).X)
            assert np.unique(r["cell"]).size > fm.ne // 2
    finally:
        v.close()


# ---- 5. the periodic tensor driver's slices on a laminate ------------------------------------------------------------------------
@pytest.mark.parametrize("n,eltype,refinements", [(4, hmg.Tri64, 3), (3, hmg.Tet64, 2)])
def test_driver_slices_on_a_laminate(ctx, tmp_path, n, eltype, refinements):
    """Layers along axis 0 with isotropic sigma_i: the correctors are P1-exact, grad u_0 = sigma_harm / sigma(cell) e_0 and
    grad u_1 = e_1, also on slices that cross the seam and lie periods away."""
    d = 2 if eltype == hmg.Tri64 else 3
    layer = np.array([1.0, 9.0, 3.0, 5.0][:n])
    sg = np.broadcast_to(layer.reshape((n,) + (1,) * d), (n,) * d + (d,)).copy()
    harm = n / np.sum(1.0 / layer)
    step = 1 / 32
    if d == 2:
        slices = [((-0.75 * n + 1 / 128, -0.25 + 1 / 256), (2.5 * n / 80, 0.0), (0.0, step), 80, 40),
                  ((n - 0.5, 2.0 * n + 1 / 64), (1 / 64, 1 / 256), (-1 / 256, 1 / 64), 64, 64)]
    else:
        slices = [((-0.75 * n + 1 / 128, -0.25 + 1 / 256, 0.5 * n + 1 / 512), (2.5 * n / 80, 0.0, 0.0), (0.0, step, 0.0), 80, 40),
                  ((n - 0.5, 2.0 * n + 1 / 64, -1.0), (1 / 64, 1 / 256, 0.0), (-1 / 256, 1 / 64, 1 / 32), 64, 64)]
    kw = dict(refinements=refinements, ctx=ctx, sigma_grid=sg, tolerance=1e-12)
    out = driver.periodic_homogenization_tensor(n, eltype, slices=slices, save=str(tmp_path / "run"), **kw)
    plain = driver.periodic_homogenization_tensor(n, eltype, **kw)
    assert "slices" not in plain and np.array_equal(out["tensor"], plain["tensor"])       # unchanged by slices=
    assert abs(out["tensor"][0, 0] - harm) <= 1e-8
    assert len(out["slices"]) == 2 and all(len(per_k) == d for per_k in out["slices"])
    per_cube = (2 if d == 2 else 6) * n ** (d - 1)                # cells per layer: cube q = cell // (2 or 6), layer = q // n^(d-1)
    for i, per_k in enumerate(out["slices"]):
        for k, s in enumerate(per_k):
            assert set(s) == {"value", "gradient", "cell", "flux", "energy_density"}
            assert (tmp_path / f"run_slice{i}_u{k + 1}.vts").exists()
            assert (s["cell"] >= 0).all()
        sigma = layer[per_k[0]["cell"] // per_cube]
        assert np.unique(per_k[0]["cell"] // per_cube).size == (n if i == 0 else 2)       # every layer; the two at the seam
        want0 = np.zeros(per_k[0]["gradient"].shape)
        want0[..., 0] = harm / sigma
        e0, e1 = np.abs(per_k[0]["gradient"] - want0).max(), np.abs(per_k[1]["gradient"] - np.eye(d)[1]).max()
        print(f"n {n} d {d} slice {i}: |grad u_0 - harm / sigma e_0| {e0:.3e}, |grad u_1 - e_1| {e1:.3e}")
        assert e0 <= 1e-8 and e1 <= 1e-8
        # the flux of u_0 is the constant sigma_harm e_0, and fields' helpers take the result as it is
        flux = fields.sample_flux(np.repeat(sg.reshape(-1, d), per_cube // n ** (d - 1), axis=0), per_k[0]["cell"], per_k[0]["gradient"])
        assert np.array_equal(flux, per_k[0]["flux"]) and np.abs(flux[..., 0] - harm).max() <= 1e-8 * layer.max()


# ---- 6. allocations --------------------------------------------------------------------------------------------------------------
def test_allocations_and_launch_counts(ctx):
    g = hmg.ImplicitFineGrid(ctx, T.mesh("torus3"), 3)
    v = hmg.DeviceMatrix(g, 3).rand(2)
    try:
        g.set_periodic_sampling(True)
        x = np.ascontiguousarray((np.random.default_rng(2).random((300, 3)) * 4.0 - 1.5) * np.asarray(g.base.period))
        ctx.sync()
        a0, n0 = ctx.counter("device_allocs"), ctx.counter("sample_launches")
        first = hmg.sample(v, g, x)
        a1 = ctx.counter("device_allocs")
        assert a1 > a0 and ctx.counter("sample_launches") == n0 + 1                # locator, lattice table, one pool block
        again = hmg.sample(v, g, x)
        assert ctx.counter("device_allocs") == a1 and ctx.counter("sample_launches") == n0 + 2
        assert all(same(again[key], first[key]) for key in first)
        r = hmg.sample_raster(v, g, (0.1, 0.2, 0.3), (1 / 8, 0, 0), (0, 1 / 8, 0), 20, 15)
        assert ctx.counter("device_allocs") == a1 and ctx.counter("sample_launches") == n0 + 3
        assert (r["cell"] >= 0).all() and ctx.counter("sample_kernel_ns") > 0 and ctx.counter("sample_download_ns") > 0
        # a line profile through several periods (fields.line_points)
        line = fields.line_points(-1.5 * np.asarray(g.base.period), 2.5 * np.asarray(g.base.period), 257)
        assert (hmg.sample(v, g, line)["cell"] >= 0).all()
    finally:
        v.close()
        g.close()
