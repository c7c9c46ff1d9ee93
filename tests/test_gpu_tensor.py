"""
The full homogenized tensor from one run: the two pair forms of the driver integrals (hmg_integrate modes 3 and 4,
api.integrate_pair_mass / integrate_pair_load) against numpy on the oracle's tables, and driver.checkerboard_homogenization_tensor
against its CPU statement (tests/_tensor_form.py, held against the scalar oracle driver by tests/test_tensor_statement.py) and
against the scalar device driver.

Bounds: the integrals 1e-11 max(|want|, 1), the bound of the existing integral tests (test_gpu_parity.py); identities between
modes on the device 1e-11 of the sum of the terms' magnitudes; tensor entries 1e-8, the |delta sigma| bound of BASELINE.md.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Pairing:
    """A mesh on oracle and device with seeded consistent v, w, a seeded load s and b = rhs_a.xi.grad(v) on the device."""

    def __init__(self, O, ctx, dim, n, levels, perturb, seed, ordered=True):
        self.O, self.levels = O, levels
        m = O.hypercube(dim, n, origin=(-n / 2.0,) * dim)
        if ordered:
            m = O.order_nodes_and_elements_by_magnitude(m)
        rng = np.random.default_rng(seed)
        if perturb:
            m.nodes = m.nodes + perturb * (rng.random(m.nodes.shape) - 0.5)
        self.mesh = m
        self.sig = rng.choice([1.0, 9.0], size=(m.nelements(), dim))
        self.impl = O.ImplicitFineGrid.create(m, levels)
        self.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(m))
        self.mass = O.mass_matrix(self.impl.reference.levels[-1])
        self.det = O.cell_geometry(m)[2]
        self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), levels)
        self.A = hmg.L2PlusDivAGrad(self.g, 0.7, self.sig)
        shape = (self.impl.nf(levels), m.nelements())
        self.v, self.w = (self.consistent(rng.standard_normal(shape)) for _ in range(2))
        self.s = np.asfortranarray(rng.standard_normal(shape))
        self.dv, self.dw, self.ds = (hmg.DeviceMatrix(self.g, levels).from_host(a) for a in (self.v, self.w, self.s))
        self.xi = rng.standard_normal(dim)
        self.db = hmg.DeviceMatrix(self.g, levels)
        hmg.rhs_axi_grad_v(self.db, self.g, self.xi)

    def consistent(self, a):
        a = np.asfortranarray(a)
        self.O.broadcast_interfaces(a, self.impl, self.levels)
        self.O.apply_constraint(a, self.levels, self.cons, self.impl)
        return a

    def want_mass(self, v, w, nsub):
        """Mq(v; w) = sum_c |J_c| sum_i w_i (M v)_i"""
        run = np.einsum("ie,ie->e", w[:, :nsub], self.mass @ v[:, :nsub])
        return float(np.sum(run * self.det[:nsub]))

    def want_load(self, v, s, nsub):
        """Lq(v; s) = sum_c |J_c| sum_i v_i s_i"""
        run = np.einsum("ie,ie->e", v[:, :nsub], s[:, :nsub])
        return float(np.sum(run * self.det[:nsub]))

    def prefixes(self):
        ne = self.mesh.nelements()
        mid = (ne // 2) | 1
        return sorted({0, 1, min(mid, ne), ne})

    def close(self):
        for a in (self.dv, self.dw, self.ds, self.db):
            a.close()
        self.g.close()


def _check_pairing(p, ctx):
    g = p.g
    for nsub in p.prefixes():
        a = p.want_mass(p.v, p.w, nsub)
        got = hmg.integrate_pair_mass(p.dv, p.dw, g, nsub)
        print(f"level {p.levels} nsub {nsub}: Mq(v; w) {got:.15e} want {a:.15e} diff {got - a:.2e}")
        assert abs(got - a) <= TOL * max(abs(a), 1.0), (nsub, got, a)
        a = p.want_mass(p.v, p.v, nsub)
        got = hmg.integrate_pair_mass(p.dv, p.dv, g, nsub)                   # the second vector may be v
        assert abs(got - a) <= TOL * max(abs(a), 1.0), (nsub, got, a)
        a = p.want_load(p.v, p.s, nsub)
        got = hmg.integrate_pair_load(p.dv, p.ds, g, nsub)
        print(f"level {p.levels} nsub {nsub}: Lq(v; s) {got:.15e} want {a:.15e} diff {got - a:.2e}")
        assert abs(got - a) <= TOL * max(abs(a), 1.0), (nsub, got, a)
        if nsub == 0:
            assert hmg.integrate_pair_mass(p.dv, p.dw, g, 0) == 0.0 and hmg.integrate_pair_load(p.dv, p.ds, g, 0) == 0.0
        # identities between the modes, on the device
        m0 = hmg.integrate_first_term(p.dv, g, nsub, p.xi, b=p.db)
        m4, m3vv = hmg.integrate_pair_load(p.dv, p.db, g, nsub), hmg.integrate_pair_mass(p.dv, p.dv, g, nsub)
        assert abs(m0 - (m4 + m3vv)) <= TOL * (abs(m4) + abs(m3vv)), (nsub, m0, m4, m3vv)
        m1 = hmg.integrate_terms(p.dv, p.dw, g, nsub)
        m3vw, m3wv = hmg.integrate_pair_mass(p.dv, p.dw, g, nsub), hmg.integrate_pair_mass(p.dw, p.dv, g, nsub)
        assert abs(m1 - (m3vv + m3vw)) <= TOL * (abs(m3vv) + abs(m3vw)), (nsub, m1, m3vv, m3vw)
        assert abs(m3vw - m3wv) <= TOL * (abs(m3vw) + abs(m3wv)), (nsub, m3vw, m3wv)           # M is symmetric
    # two calls: identical bits; no allocation
    ne = p.mesh.nelements()
    ctx.sync()
    allocs = ctx.counter("device_allocs")
    first = [hmg.integrate_pair_mass(p.dv, p.dw, g, ne), hmg.integrate_pair_load(p.dv, p.ds, g, ne),
             hmg.integrate_pair_mass(p.dv, p.dw, g, p.prefixes()[-2]), hmg.integrate_pair_load(p.dv, p.ds, g, p.prefixes()[-2])]
    again = [hmg.integrate_pair_mass(p.dv, p.dw, g, ne), hmg.integrate_pair_load(p.dv, p.ds, g, ne),
             hmg.integrate_pair_mass(p.dv, p.dw, g, p.prefixes()[-2]), hmg.integrate_pair_load(p.dv, p.ds, g, p.prefixes()[-2])]
    assert first == again
    assert ctx.counter("device_allocs") == allocs


# meshes of the sizes tests/test_gpu_parity.py, test_gpu_parity_l6.py and test_gpu_tri_deep.py use for these levels; a perturbed
# mesh has one coefficient row per cell (more than one cell class), an unperturbed one a handful
@pytest.mark.parametrize("levels,n,perturb,ordered", [(2, 4, 0.2, True), (3, 4, 0.2, True), (4, 4, 0.0, True), (4, 4, 0.2, True),
                                                      (5, 4, 0.2, True), (6, 2, 0.0, True), (6, 2, 0.1, True),
                                                      (7, 1, 0.1, False)])
def test_pair_integrals_match_numpy_3d(oracle, ctx, levels, n, perturb, ordered):
    """Every kernel family that carries the integral form in 3D: levels 2-4 (64 / 192 threads), 5 and 6 (register-blocked
    interior and class-wise surface), 7 (cells larger than the LDS: the rolling-window slab kernel)."""
    p = Pairing(oracle, ctx, 3, n, levels, perturb, 100 + levels, ordered)
    _check_pairing(p, ctx)
    p.close()


@pytest.mark.parametrize("levels,n,perturb", [(3, 6, 0.2), (8, 2, 0.1), (9, 4, 0.2)])
def test_pair_integrals_match_numpy_2d(oracle, ctx, levels, n, perturb):
    """Triangles: level 3 (odd Nf = 15: columns that are not 16-byte aligned), 8 (the largest cell that fits the LDS), 9 (row-band
    kernel)."""
    n0 = ctx.counter("rows_launches")
    p = Pairing(oracle, ctx, 2, n, levels, perturb, 200 + levels)
    assert p.g.ld(levels) % 2 == 1 or levels != 3
    _check_pairing(p, ctx)
    assert (ctx.counter("rows_launches") > n0) == (levels >= 9)
    p.close()


def test_pair_integral_errors_and_prefix_after_a_shrink(oracle, ctx):
    """Mode 5 is an error, so are vectors of different levels and a prefix beyond the grid; after a shrink the limit is the new cell
    count and the values are those of the shrunk mesh's prefix."""
    import ctypes
    from homogenization_jl_amd import _lib as L
    p = Pairing(oracle, ctx, 3, 6, 3, 0.0, 7)
    ne = p.mesh.nelements()
    out = ctypes.c_double()
    assert L.load().hmg_integrate(p.g.h, 5, p.dv.h, p.dw.h, ne, None, ctypes.byref(out)) != 0
    with pytest.raises(HmgError, match="mode must be"):
        hmg.api._integrate(p.g, 5, p.dv, p.dw, ne, None)
    low = hmg.DeviceMatrix(p.g, 2)
    for fn in (hmg.integrate_pair_mass, hmg.integrate_pair_load):
        with pytest.raises(HmgError):
            fn(p.dv, low, p.g, ne)
        with pytest.raises(HmgError, match="subset out of range"):
            fn(p.dv, p.dw, p.g, ne + 1)
    with pytest.raises(HmgError, match="second vector"):
        hmg.api._integrate(p.g, 3, p.dv, None, ne, None)
    O = oracle
    ne2, nn2 = O.find_elements_in_radius(p.mesh, 2), O.find_nodes_in_radius(p.mesh, 2)
    assert 0 < ne2 < ne
    p.g.shrink(ne2, nn2)
    for fn in (hmg.integrate_pair_mass, hmg.integrate_pair_load):
        with pytest.raises(HmgError, match="subset out of range"):
            fn(p.dv, p.dw, p.g, ne2 + 1)
    a = p.want_mass(p.v, p.w, ne2)
    assert abs(hmg.integrate_pair_mass(p.dv, p.dw, p.g, ne2) - a) <= TOL * max(abs(a), 1.0)
    a = p.want_load(p.v, p.s, ne2)
    assert abs(hmg.integrate_pair_load(p.dv, p.ds, p.g, ne2) - a) <= TOL * max(abs(a), 1.0)
    low.close()
    p.close()


# ---- the tensor driver ----------------------------------------------------------------------------------------------------
_NF = {2: [3, 6, 15, 45, 153, 561], 3: [4, 10, 35, 165, 969, 6545]}


def _inputs(dim, n, refinements, seed):
    """The field and the initial guess in the oracle driver's order of draws (default_rng(seed): sigma first, then x0)."""
    rng = np.random.default_rng(seed)
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sgrid = np.where(rng.random((width,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    x0 = rng.random((_NF[dim][refinements], (2 if dim == 2 else 6) * width ** dim))
    return sgrid, x0


@pytest.mark.parametrize("dim,n,tol,steps", [(2, 5, 1e-12, {0, 1}), (3, 0, 1e-13, {0})])
def test_tensor_driver_matches_the_cpu_statement(ctx, dim, n, tol, steps):
    """The two cases of tests/test_tensor_statement.py (the 2D one includes a domain shrink), the same sigma_grid and x0."""
    from _tensor_form import checkerboard_homogenization_tensor as cpu_tensor
    sgrid, x0 = _inputs(dim, n, 1, 3)
    want, hist_c = cpu_tensor(n=n, dim=dim, refinements=1, tolerance=tol, sigma_grid=sgrid, x0=x0)
    t = {}
    got, hist_d = driver.checkerboard_homogenization_tensor(n, hmg.Tri64 if dim == 2 else hmg.Tet64, refinements=1, tolerance=tol,
                                                            sigma_grid=sgrid, x0=x0, ctx=ctx, timings=t)
    print("device\n", got, "\ncpu statement\n", want, "\nlargest difference", np.abs(got - want).max())
    assert got.shape == (dim, dim) and np.array_equal(got, got.T)
    assert {h[0] for h in hist_d} == steps
    assert {(h[0], h[1]) for h in hist_d} == {(k, d) for k in steps for d in range(dim)}
    assert np.abs(got - want).max() <= 1e-8, (got, want)
    assert t["inexact_vcycles"] == 0 and t["directions"] == dim and t["pair_integrals_s"] > 0 and t["vcycles"] == len(hist_d)


def _polarised_on_device(ctx, n, el, dim, **kw):
    from _tensor_form import polarised
    return polarised(lambda xi: driver.checkerboard_homogenization(n, el, xi=xi, ctx=ctx, **kw)[0], dim)


@pytest.mark.parametrize("dim,n,refinements", [(2, 5, 2), (3, 0, 2)])
def test_tensor_driver_matches_the_scalar_device_driver(ctx, dim, n, refinements):
    """Sigma_ii against the scalar driver with xi = e_i, xi' Sigma xi against its default xi; accelerate=True gives the same
    tensor; every (k, direction) is in the history; no inexact level-1 solve."""
    el = hmg.Tri64 if dim == 2 else hmg.Tet64
    kw = dict(refinements=refinements, tolerance=1e-12, seed=5)
    t = {}
    S, hist = driver.checkerboard_homogenization_tensor(n, el, ctx=ctx, timings=t, **kw)
    outer = {h[0] for h in hist}
    assert {(h[0], h[1]) for h in hist} == {(k, d) for k in outer for d in range(dim)}
    assert t["inexact_vcycles"] == 0 and t["outer_steps"] == len(outer)
    if dim == 2:
        assert outer == {0, 1}
    for i in range(dim):
        want, hist_s = driver.checkerboard_homogenization(n, el, xi=np.eye(dim)[i], ctx=ctx, **kw)
        print(f"Sigma_{i}{i} {S[i, i]:.15f} scalar {want:.15f} diff {S[i, i] - want:.2e}")
        assert abs(S[i, i] - want) <= 1e-8, (i, S[i, i], want)
        assert {h[0] for h in hist_s} == outer
    xi = driver.random_unit_vec(dim)
    want, _ = driver.checkerboard_homogenization(n, el, ctx=ctx, **kw)
    got = float(xi @ S @ xi)
    print(f"xi' Sigma xi {got:.15f} scalar {want:.15f} diff {got - want:.2e}")
    assert abs(got - want) <= 1e-8, (got, want)
    ta = {}
    Sa, hist_a = driver.checkerboard_homogenization_tensor(n, el, ctx=ctx, accelerate=True, timings=ta, **kw)
    print("accelerated - plain: largest difference", np.abs(Sa - S).max(), "cycles", len(hist_a), "against", len(hist))
    assert np.abs(Sa - S).max() <= 1e-8, (Sa, S)
    assert ta["inexact_vcycles"] == 0


@pytest.mark.parametrize("refinements", [4, 5])
def test_tensor_driver_on_the_level_5_and_6_kernels(ctx, refinements):
    """3D, n = 0 (10^3 cubes), finest level 5 / 6: all six entries against the polarisation of six scalar device runs."""
    kw = dict(refinements=refinements, tolerance=1e-12, seed=2)
    t = {}
    S, hist = driver.checkerboard_homogenization_tensor(0, hmg.Tet64, ctx=ctx, timings=t, **kw)
    want = _polarised_on_device(ctx, 0, hmg.Tet64, 3, **kw)
    print("tensor\n", S, "\npolarised\n", want, "\nlargest difference", np.abs(S - want).max())
    assert np.abs(S - want).max() <= 1e-8, (S, want)
    assert {(h[0], h[1]) for h in hist} == {(0, d) for d in range(3)}
    assert t["inexact_vcycles"] == 0


def test_scalar_driver_is_unchanged_by_a_tensor_run(ctx):
    """The scalar driver with fixed inputs returns the same bits before and after a tensor run in the same context."""
    kw = dict(refinements=2, tolerance=1e-6, seed=9, ctx=ctx)
    before = driver.checkerboard_homogenization(5, hmg.Tri64, **kw)
    driver.checkerboard_homogenization_tensor(5, hmg.Tri64, **kw)
    after = driver.checkerboard_homogenization(5, hmg.Tri64, **kw)
    assert before[0] == after[0]
    assert before[1] == after[1]


def test_tensor_driver_save_writes_one_file_per_step_and_direction(ctx, tmp_path):
    from homogenization_jl_amd import vtk
    S0, h0 = driver.checkerboard_homogenization_tensor(1, hmg.Tri64, refinements=2, tolerance=1e-3, ctx=ctx)
    S1, h1 = driver.checkerboard_homogenization_tensor(1, hmg.Tri64, refinements=2, tolerance=1e-3, ctx=ctx,
                                                       save=(2, str(tmp_path)))
    assert np.array_equal(S0, S1) and h0 == h1
    for k, d in {(h[0], h[1]) for h in h1}:
        out = vtk.read_vtu(str(tmp_path / f"ahom_{k}_{d}.vtu"))
        assert np.isfinite(out["point_data"]["v"]).all()
