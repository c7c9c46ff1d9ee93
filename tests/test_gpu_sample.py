"""Point sampling on the device (include/hmg.h: hmg_sample, hmg_sample_raster) against the host's hmg_grid_locate and the numpy
statement of tests/_sample_form.py: a random vector at points that are interior by construction, affine data at interior points
and at every kind of tie, launch tails, rasters against point lists bit for bit, the zero-weight rule, allocations and the pending
r-update, the guard of the raw column pointer, and the driver's slices.  Bounds: the formulas of _sample_form.py."""
import ctypes

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import driver

import _sample_form as F

pytestmark = pytest.mark.gpu

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
def grid(ctx, oracle):
    def get(name):
        if name not in _grids:
            _grids[name] = hmg.ImplicitFineGrid(ctx, F.base_mesh(oracle, name), F.GRID_LEVELS[name])
        return _grids[name]
    return get


def fine(g, name, level):
    if (name, level) not in _fine:
        _fine[(name, level)] = F.FineMesh(g, level)
    return _fine[(name, level)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- 1. random vector: the device against the host's locate ---------------------------------------------------------------------
@pytest.mark.parametrize("name,level", F.LOCATE_CASES)
def test_random_vector_against_host_locate(grid, name, level):
    g = grid(name)
    fm = fine(g, name, level)
    d = fm.dim
    v = hmg.DeviceMatrix(g, level).rand(40 + level)
    try:
        xh = v.to_host()
        vmax = float(np.abs(xh).max())
        pts = fm.interior_points(200, seed=100 + level)
        x = pts["x"]
        cell, nodes, w, gw = hmg.locate(g, level, x)
        assert np.array_equal(cell, pts["cell"])
        vals = xh[nodes, cell[:, None]]                                        # (n, d + 1)
        ref_v = (w * vals).sum(axis=1)
        ref_g = np.einsum("nk,nkc->nc", vals, gw)
        xi = np.array([0.3, -1.7, 0.9][:d])
        for use_xi in (None, xi):
            s = hmg.sample(v, g, x, xi=use_xi)
            assert np.array_equal(s["cell"], cell) and s["cell"].dtype == np.int32
            want_v = ref_v if use_xi is None else ref_v + x @ xi
            want_g = ref_g if use_xi is None else ref_g + xi
            err_v, err_g = np.abs(s["value"] - want_v).max(), np.abs(s["gradient"] - want_g).max()
            print(f"{name} level {level} xi {use_xi is not None}: value {err_v:.3e} (bound {fm.T_value(vmax, use_xi):.3e}), "
                  f"gradient {err_g:.3e} (bound {fm.T_gradient(vmax, use_xi):.3e})")
            assert err_v <= fm.T_value(vmax, use_xi)
            assert err_g <= fm.T_gradient(vmax, use_xi)
            # each output left out in turn: the others keep their bits
            for off in ("value", "gradient", "cell"):
                t = hmg.sample(v, g, x, xi=use_xi, **{off: False})
                assert off not in t and set(t) == {"value", "gradient", "cell"} - {off}
                for key in t:
                    assert same(t[key], s[key]), (off, key)
    finally:
        v.close()


# ---- 2. affine exactness, whatever the tie rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", F.AFFINE_CASES)
def test_affine_data_is_reproduced_everywhere(grid, name, level):
    g = grid(name)
    fm = fine(g, name, level)
    d = fm.dim
    alpha, beta = 0.7, np.array([1.3, -0.4, 2.1][:d])
    v = hmg.DeviceMatrix(g, level)
    try:
        xh = fm.affine_vector(alpha, beta)
        v.from_host(xh)
        vmax = float(np.abs(xh).max())
        x = np.concatenate([fm.interior_points(200, seed=7)["x"], fm.nodes, fm.edge_midpoints(20000, seed=8),
                            fm.coarse_face_points(g, 20, seed=9)])
        s = hmg.sample(v, g, x)
        assert (s["cell"] >= 0).all()                                          # the closed domain: every point is found
        err_v = np.abs(s["value"] - (alpha + x @ beta)).max()
        err_g = np.abs(s["gradient"] - beta).max()
        print(f"{name} level {level}: {x.shape[0]} points, value {err_v:.3e} (bound {fm.T_affine(alpha, beta):.3e}), "
              f"gradient {err_g:.3e} (bound {fm.T_gradient(vmax):.3e})")
        assert err_v <= fm.T_affine(alpha, beta)
        assert err_g <= fm.T_gradient(vmax)
    finally:
        v.close()


# ---- 3. launch tails ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("cube3x2", 4), ("square4", 5)])
def test_launch_tails(grid, name, level):
    g = grid(name)
    fm = fine(g, name, level)
    v = hmg.DeviceMatrix(g, level).rand(5)
    try:
        x = fm.interior_points(1000, seed=3)["x"]
        x[17] = fm.nodes.max(axis=0) + 1.0                                      # one point outside, in the first wave
        xi = np.full(fm.dim, 0.5)
        full = hmg.sample(v, g, x, xi=xi)
        assert full["cell"][17] == -1 and np.isnan(full["value"][17]) and np.isnan(full["gradient"][17]).all()
        for n in (1, 63, 64, 65, 257, 1000):
            part = hmg.sample(v, g, x[:n], xi=xi)
            for key in ("value", "gradient", "cell"):
                assert same(part[key], full[key][:n]), (n, key)
    finally:
        v.close()


# ---- 4. rasters: bitwise the point list ------------------------------------------------------------------------------------------
RASTERS = {   # dyadic origin and steps: the fmas of the device are exact, and so is numpy's origin + a du + b dv
    "cube3x2": (3, [((1.5, 1.25, 2.0625), (1 / 64, 0.0, 0.0), (0.0, 1 / 64, 0.0), 1, 1),
                    ((0.75, 0.875, 1.25), (1 / 32, 1 / 64, 0.0), (0.0, 1 / 64, 1 / 2), 65, 3),           # an oblique plane
                    ((0.875, 1.0, 0.9375), (1 / 16, 1 / 32, 1 / 64), (-1 / 64, 1 / 16, 1 / 16), 33, 33),
                    # thinner than a 16 x 16 tile one way: lines both ways (256 x 1 and 1 x 256 tiles), 8 x 32 and 4 x 64 tiles
                    ((0.75, 1.5, 1.5), (1 / 64, 0.0, 0.0), (0.0, 1 / 64, 0.0), 300, 1),
                    ((1.5, 0.75, 1.5), (1 / 64, 0.0, 0.0), (0.0, 1 / 64, 1 / 128), 1, 300),
                    ((0.875, 0.9375, 1.25), (1 / 4, 0.0, 1 / 64), (0.0, 1 / 8, 0.0), 5, 40),
                    ((0.9375, 0.875, 1.25), (1 / 8, 0.0, 0.0), (0.0, 1 / 4, 1 / 64), 70, 3)]),
    "square4": (4, [((2.5, 3.125), (1 / 64, 0.0), (0.0, 1 / 64), 1, 1),
                    ((0.75, 0.875), (5 / 64, 1 / 64), (-1 / 8, 3 / 2), 65, 3),
                    ((0.5, 0.75), (5 / 32, 1 / 64), (-1 / 64, 5 / 32), 33, 33),
                    ((0.5, 2.0), (1 / 32, 0.0), (0.0, 1 / 32), 300, 1),
                    ((2.0, 0.5), (1 / 32, 0.0), (1 / 64, 1 / 32), 1, 300),
                    ((0.875, 0.9375), (1 / 4, 0.0), (0.0, 1 / 8), 5, 40),
                    ((0.9375, 0.875), (1 / 8, 0.0), (0.0, 1 / 4), 70, 3)]),
}


@pytest.mark.parametrize("name", sorted(RASTERS))
def test_raster_equals_the_point_list(grid, name):
    g = grid(name)
    level, rasters = RASTERS[name]
    d = g.base.dim
    v = hmg.DeviceMatrix(g, level).rand(6)
    try:
        xi = np.array([1.0, -2.0, 0.5][:d])
        for origin, du, dv, nu, nv in rasters:
            r = hmg.sample_raster(v, g, origin, du, dv, nu, nv, xi=xi)
            a = np.arange(nu, dtype=np.float64)[None, :, None]
            b = np.arange(nv, dtype=np.float64)[:, None, None]
            x = (np.asarray(origin) + a * np.asarray(du) + b * np.asarray(dv)).reshape(-1, d)
            p = hmg.sample(v, g, x, xi=xi)
            assert r["value"].shape == (nv, nu) and r["gradient"].shape == (nv, nu, d) and r["cell"].shape == (nv, nu)
            assert same(r["value"].ravel(), p["value"]) and same(r["cell"].ravel(), p["cell"])
            assert same(r["gradient"].reshape(-1, d), p["gradient"])
            out = r["cell"] < 0
            assert np.isnan(r["value"][out]).all() and np.isnan(r["gradient"][out]).all()
            assert np.isfinite(r["value"][~out]).all() and np.isfinite(r["gradient"][~out]).all()
            if nu * nv > 1:
                assert out.any() and (~out).any()                               # partly hanging over the domain
            lo, hi = g.base.nodes.min(axis=0), g.base.nodes.max(axis=0)
            inside = ((x >= lo) & (x <= hi)).all(axis=1)                        # the domain is the box
            assert np.array_equal(~out.ravel(), inside)
            r2 = hmg.sample_raster(v, g, origin, du, dv, nu, nv, xi=xi, gradient=False)
            assert "gradient" not in r2 and same(r2["value"], r["value"]) and same(r2["cell"], r["cell"])
    finally:
        v.close()


# ---- 5. a vertex without a weight is not read -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("cube3x2", 3), ("square4", 3)])
def test_zero_weight_vertex_is_not_read(grid, name, level):
    g = grid(name)
    fm = fine(g, name, level)
    d = fm.dim
    v = hmg.DeviceMatrix(g, level).rand(9)
    try:
        xh = v.to_host()
        cell = 0                                                                # (it wins every tie on its surface)
        interior = np.flatnonzero(g.table_i32("slot_cls", level)[g.table_i32("hier2slot", level)] == 0)
        h = int(interior[len(interior) // 2])                                   # a node inside the cell: one copy
        xh[h, cell] = np.nan
        v.from_host(xh)
        bad = cell * fm.nf + h
        els = fm.cells[(fm.cells == bad).any(axis=1)]                           # the elements around the node
        assert len(els) >= 2 * d
        wts = np.array([0.5, 0.25, 0.25] if d == 3 else [0.75, 0.25])           # dyadic: the node's weight is exactly 0
        opposite = np.array([wts @ fm.nodes[e[e != bad]] for e in els])
        inside = np.array([fm.nodes[e].mean(axis=0) for e in els])
        for grad in (False, True):
            s = hmg.sample(v, g, opposite, gradient=grad)
            assert (s["cell"] == cell).all() and np.isfinite(s["value"]).all()
            s = hmg.sample(v, g, inside, gradient=grad)
            assert (s["cell"] == cell).all() and np.isnan(s["value"]).all()
        assert np.isnan(hmg.sample(v, g, inside)["gradient"]).all()
    finally:
        v.close()


# ---- 6. memory and the pending r-update -----------------------------------------------------------------------------------------
class Problem:
    def __init__(self, ctx, levels=4):
        self.levels = levels
        self.base, self.cond, self.g, self.op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, levels, seed=17, lam=0.8)
        self.bl = hmg.BaseLevel(self.g)
        self.ops = [self.op] * levels

    def start(self):
        st = [hmg.LevelState(self.g, i + 1) for i in range(self.levels)]
        st[-1].x.rand(3)
        st[-1].b.rand(4)
        hmg.broadcast_interfaces(st[-1].x, self.g, self.levels)
        hmg.apply_constraint(st[-1].x, self.levels, self.g)
        return st

    def cycles(self, st, n):
        for _ in range(n):
            hmg.vcycle(self.g, self.bl, self.ops, st, self.levels, 3, 2)


def _close(st):
    for s in st:
        s.close()


def test_allocations_and_pending_r(ctx):
    P = Problem(ctx)
    try:
        rng = np.random.default_rng(2)
        x = rng.random((300, 3)) * 2.2 - 1.1                                    # the domain is [-1, 1]^3: some points outside
        st = P.start()
        P.cycles(st, 2)
        ctx.sync()
        a0 = ctx.counter("device_allocs")
        first = hmg.sample(st[-1].x, P.g, x)
        a1 = ctx.counter("device_allocs")
        assert a1 > a0                                                          # locator, lattice table, one pool block
        assert (first["cell"] >= 0).any() and (first["cell"] < 0).any()
        for _ in range(5):
            again = hmg.sample(st[-1].x, P.g, x)
            assert all(same(again[k], first[k]) for k in first)
        assert ctx.counter("device_allocs") == a1
        P.cycles(st, 1)
        ctx.sync()
        assert ctx.counter("device_allocs") == a1
        assert ctx.counter("sample_kernel_ns") > 0 and ctx.counter("sample_download_ns") > 0
        _close(st)

        # sampling x leaves an open record alone
        st = P.start()
        P.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == 1
        m0 = ctx.counter("r_materialized")
        hmg.sample(st[-1].x, P.g, x)
        assert ctx.counter("r_materialized") == m0
        _close(st)

        # sampling r settles it: the bits of a twin run without the record
        got = []
        try:
            for lazy in (0, 1):
                ctx.set_option("lazy_r", lazy)
                st = P.start()
                P.cycles(st, 2)
                assert ctx.counter("lazy_r_form") == lazy
                m0 = ctx.counter("r_materialized")
                got.append(hmg.sample(st[-1].r, P.g, x, xi=np.array([0.1, 0.2, 0.3])))
                assert ctx.counter("r_materialized") == m0 + lazy
                _close(st)
        finally:
            ctx.set_option("lazy_r", 1)
        assert np.isfinite(got[0]["value"][got[0]["cell"] >= 0]).all()
        for key in got[0]:
            assert same(got[0][key], got[1][key]), key
    finally:
        P.g.close()


# ---- 7. the raw column pointer is checked before anything is launched -----------------------------------------------------------
def test_pointer_guard(grid, ctx):
    lib = L.load()
    g = grid("cube3x2")
    v2, v4 = hmg.DeviceMatrix(g, 2), hmg.DeviceMatrix(g, 4)
    try:
        x = np.array([[1.5, 1.5, 1.5]])
        val = np.zeros(1)
        px, pv = x.ctypes.data_as(L.p_f64), val.ctypes.data_as(L.p_f64)
        hmg.sample(v4, g, x)
        n0 = ctx.counter("sample_launches")
        assert n0 >= 1
        host = np.zeros(g.ld(4) * g.ncells())
        cases = [(4, v2.device_ptr(), "bytes"),                                  # a level-2 vector handed in as level 4
                 (4, v4.device_ptr() + 8 * (g.ld(4) * g.ncells() // 2), "bytes"),  # into the middle of a vector
                 (4, 0, "null"), (4, host.ctypes.data, "device memory")]
        for level, ptr, word in cases:
            rc = lib.hmg_sample(g.h, level, ctypes.c_void_p(ptr), None, 1, px, pv, None, None)
            assert rc != 0
            msg = lib.hmg_last_error().decode()
            assert "hmg_sample" in msg and word in msg, msg
            rc = lib.hmg_sample_raster(g.h, level, ctypes.c_void_p(ptr), None, px, px, px, 1, 1, pv, None, None)
            assert rc != 0 and "hmg_sample_raster" in lib.hmg_last_error().decode()
        # the other refusals of the device calls
        ok = ctypes.c_void_p(v4.device_ptr())
        assert lib.hmg_sample(g.h, 4, ok, None, 1, px, None, None, None) != 0 and "output" in lib.hmg_last_error().decode()
        assert lib.hmg_sample(g.h, 4, ok, None, 1, None, pv, None, None) != 0 and "null points" in lib.hmg_last_error().decode()
        assert lib.hmg_sample(g.h, 4, ok, None, 2 ** 31, px, pv, None, None) != 0 and "2^31" in lib.hmg_last_error().decode()
        assert lib.hmg_sample_raster(g.h, 4, ok, None, px, px, px, 65536, 32768, pv, None, None) != 0
        assert "2^31" in lib.hmg_last_error().decode()
        assert lib.hmg_sample_raster(g.h, 4, ok, None, None, px, px, 1, 1, pv, None, None) != 0 and "null origin" in lib.hmg_last_error().decode()
        val[0] = 5.0
        assert lib.hmg_sample(g.h, 4, ok, None, 0, None, pv, None, None) == 0 and val[0] == 5.0
        assert lib.hmg_sample_raster(g.h, 4, ok, None, px, px, px, 0, 7, pv, None, None) == 0 and val[0] == 5.0
        assert ctx.counter("sample_launches") == n0                              # nothing was launched
    finally:
        v2.close()
        v4.close()


# ---- 8. the driver's slices ------------------------------------------------------------------------------------------------------
def test_driver_slices(ctx, tmp_path):
    xi = np.array([0.6, 0.0, 0.8])
    sl = ((1.0 + 1 / 128, 1.0 + 1 / 128, 1.4), (1 / 32, 0.0, 0.0), (0.0, 1 / 32, 0.0), 64, 64)       # z = 1.4, inside [1, 3]^3
    out = driver.dirichlet_homogenization(2, hmg.Tet64, refinements=2, xi=xi, ctx=ctx, slices=[sl], fields=True, extrema=True,
                                          save=str(tmp_path / "run"))
    assert (tmp_path / "run_slice0.vts").exists()
    s = out["slices"][0]
    assert set(s) == {"value", "gradient", "cell", "flux", "energy_density"}
    assert s["energy_density"].shape == (64, 64) and s["flux"].shape == (64, 64, 3) and (s["cell"] >= 0).all()
    cells, counts = np.unique(s["cell"], return_counts=True)
    c = int(cells[np.argmax(counts)])
    avg = float(s["energy_density"][s["cell"] == c].mean())
    lo, hi = out["min_energy_density"][c], out["peak_energy_density"][c]
    print(f"cell {c}: {counts.max()} pixels, energy density {lo:.6e} <= {avg:.6e} <= {hi:.6e}")
    assert lo < hi and lo * (1 - 1e-12) <= avg <= hi * (1 + 1e-12)
    # a uniform medium: the loads cancel, v = 0 and every pixel's gradient is xi
    out = driver.dirichlet_homogenization(2, hmg.Tet64, refinements=2, xi=xi, ctx=ctx, slices=[sl], values=(1.0, 1.0))
    assert out["cycles"] == 0
    g = out["slices"][0]["gradient"]
    assert np.abs(g - xi).max() <= 4 * F.EPS * np.abs(xi).max()            # the gradient bound with max|v| = 0
    assert "slices" not in driver.dirichlet_homogenization(2, hmg.Tri64, refinements=1, ctx=ctx)
