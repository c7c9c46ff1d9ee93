"""
2D grids of 9 to 11 levels (cells of 33 153 / 131 841 / 525 825 nodes, larger than the LDS) on the device against the CPU oracle:
the row-band apply of hmg_apply_rows.hip in every form the library sends it, the transfers, interface sums, smoother, V-cycle,
driver integrals and the driver itself.  Tri64 checkerboards of 8 to 32 cells (200 for the driver).
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

pytestmark = pytest.mark.gpu

TOL = 1e-11
EXACT_OPTIONS = ("lean_post", "lazy_post", "lazy_top", "lazy_dead", "fold_x", "swap_rp", "fold_prolong", "prolong_in_image", "fold_faces",
                 "fold_restrict", "zero_entry", "cell_order")


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Case:
    def __init__(self, O, ctx, n, levels, lam=0.7, seed=0, perturb=0.2):
        self.O, self.levels, self.lam = O, levels, lam
        m = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, n, origin=(-n / 2.0,) * 2))
        rng = np.random.default_rng(seed)
        m.nodes = m.nodes + perturb * (rng.random(m.nodes.shape) - 0.5)
        self.mesh = m
        self.sig = rng.choice([1.0, 9.0], size=(m.nelements(), 2))
        self.impl = O.ImplicitFineGrid.create(m, levels)
        self.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(m))
        self.ops = {}
        self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), levels)
        self.A = hmg.L2PlusDivAGrad(self.g, lam, self.sig)
        self.rng = rng

    def op(self, lev):
        if lev not in self.ops:
            O, l = self.O, self.impl.reference.levels[lev - 1]
            self.ops[lev] = O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), self.cons, self.lam, self.sig)
        return self.ops[lev]

    def all_ops(self):
        return [self.op(l) for l in range(1, self.levels + 1)]

    def rand(self, level):
        return np.asfortranarray(self.rng.standard_normal((self.impl.nf(level), self.mesh.nelements())))

    def dev(self, level, a):
        return hmg.DeviceMatrix(self.g, level).from_host(a)

    def state(self, lev):
        O = self.O
        st = O.LevelState.create(self.mesh.nelements(), self.impl.nf(lev))
        st.x[...] = self.rand(lev)
        O.broadcast_interfaces(st.x, self.impl, lev)
        O.apply_constraint(st.x, lev, self.cons, self.impl)
        st.b[...] = self.rand(lev)
        return st


@pytest.fixture(scope="module")
def cases(oracle, ctx):
    # 32 cells at level 9, 18 at level 10, 8 at level 11
    return {9: Case(oracle, ctx, 4, 9, seed=9), 10: Case(oracle, ctx, 3, 10, seed=10), 11: Case(oracle, ctx, 2, 11, seed=11)}


@pytest.mark.parametrize("levels", [9, 10, 11])
def test_apply_residual_constraint(cases, ctx, levels):
    """mul!, local_residual!, apply_constraint! on the finest level through the row-band kernel (counter "rows_launches")."""
    c = cases[levels]
    O, lev = c.O, levels
    x, y = c.rand(lev), c.rand(lev)
    want = y.copy(order="F")
    O.mul(-1.3, c.mesh, c.op(lev), x, want)
    dx, dy = c.dev(lev, x), c.dev(lev, y)
    n0 = ctx.counter("rows_launches")
    hmg.mul(-1.3, c.g, c.A, dx, dy)
    assert ctx.counter("rows_launches") == n0 + 1
    assert relerr(dy.to_host(), want) <= TOL
    st = O.LevelState.create(c.mesh.nelements(), c.impl.nf(lev))
    st.x[...] = c.rand(lev); st.b[...] = c.rand(lev)
    O.local_residual(c.impl, c.op(lev), st, lev)
    dst = hmg.LevelState(c.g, lev)
    dst.x.from_host(st.x); dst.b.from_host(st.b)
    hmg.local_residual(c.g, c.A, dst, lev)
    got = dst.r.to_host()
    assert relerr(got, st.r) <= TOL
    np.testing.assert_array_equal(got == 0.0, st.r == 0.0)              # same Dirichlet zero pattern
    a = c.rand(lev)
    want = a.copy(order="F"); O.apply_constraint(want, lev, c.cons, c.impl)
    d = c.dev(lev, a); hmg.apply_constraint(d, lev, c.g)
    np.testing.assert_array_equal(d.to_host(), want)


def test_level8_apply_keeps_its_kernel(cases, ctx):
    """A level-8 cell fits the LDS: its apply does not take the row-band kernel."""
    c = cases[9]
    x, y = c.rand(8), c.rand(8)
    want = y.copy(order="F")
    c.O.mul(0.9, c.mesh, c.op(8), x, want)
    dy = c.dev(8, y)
    n0 = ctx.counter("rows_launches")
    hmg.mul(0.9, c.g, c.A, c.dev(8, x), dy)
    assert ctx.counter("rows_launches") == n0
    assert relerr(dy.to_host(), want) <= TOL


def test_apply_is_deterministic(cases):
    c = cases[10]
    x, y = c.rand(10), c.rand(10)
    outs = []
    for _ in range(2):
        dy = c.dev(10, y)
        hmg.mul(1.0, c.g, c.A, c.dev(10, x), dy)
        outs.append(dy.to_host())
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("levels", [9, 10, 11])
def test_transfer_interfaces_duplicates(cases, levels):
    """restrict_to! (1e-14), interpolate_and_sum_to!, broadcast_interfaces!, zero_out_all_but_one! (bit-exact)."""
    c = cases[levels]
    O, lev = c.O, levels
    P = c.impl.reference.interops[lev - 2]
    xf, xc = c.rand(lev), c.rand(lev - 1)
    want = xf.copy(order="F"); O.interpolate_and_sum_to(want, P, xc)
    df, dc = c.dev(lev, xf), c.dev(lev - 1, xc)
    hmg.interpolate_and_sum_to(df, c.g, dc)
    np.testing.assert_array_equal(df.to_host(), want)
    wantb = np.zeros_like(xc, order="F"); O.restrict_to(wantb, P, xf)
    db = hmg.DeviceMatrix(c.g, lev - 1)
    hmg.restrict_to(db, c.g, c.dev(lev, xf))
    assert relerr(db.to_host(), wantb) <= 1e-14
    a = c.rand(lev)
    want = a.copy(order="F"); O.broadcast_interfaces(want, c.impl, lev)
    d = c.dev(lev, a); hmg.broadcast_interfaces(d, c.g, lev)
    np.testing.assert_array_equal(d.to_host(), want)
    want2 = want.copy(order="F"); O.zero_out_all_but_one(want2, c.impl, lev)
    n_unique = hmg.norm_unique(d)
    assert abs(n_unique - np.linalg.norm(want2)) <= 1e-13 * np.linalg.norm(want2)
    hmg.zero_out_all_but_one(d, c.g, lev)
    np.testing.assert_array_equal(d.to_host(), want2)


@pytest.mark.parametrize("fused", [1, 0])
def test_smoothing_steps(oracle, ctx, cases, fused):
    """smoothing_steps! on level 10, fused CG pass and one kernel per statement: x, r, p, Ap <= 1e-10."""
    if fused:
        c = cases[10]
    else:
        ctx.set_option("fuse_cg", 0)              # read when a grid is created
        try:
            c = Case(oracle, ctx, 2, 10, seed=17)
        finally:
            ctx.set_option("fuse_cg", 1)
    lev = 10
    st = c.state(lev)
    dst = hmg.LevelState(c.g, lev)
    dst.x.from_host(st.x); dst.b.from_host(st.b)
    c.O.smoothing_steps(3, c.impl, c.op(lev), st, lev)
    hmg.smoothing_steps(3, c.g, c.A, dst, lev)
    assert relerr(dst.x.to_host(), st.x) <= 1e-10
    assert relerr(dst.r.to_host(), st.r) <= 1e-10
    assert relerr(dst.p.to_host(), st.p) <= 1e-10
    assert relerr(dst.Ap.to_host(), st.Ap) <= 1e-10


@pytest.mark.parametrize("levels", [9, 10, 11])
def test_vcycle_matches_oracle(cases, levels):
    """One vcycle! from the finest level: x <= 1e-9, r <= 1e-8."""
    c = cases[levels]
    O = c.O
    sts = [O.LevelState.create(c.mesh.nelements(), c.impl.nf(i + 1)) for i in range(levels)]
    top = c.state(levels)
    sts[-1] = top
    dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
    dsts[-1].x.from_host(top.x); dsts[-1].b.from_host(top.b)
    O.vcycle(c.impl, O.make_base_level(c.mesh, c.sig, c.lam), c.all_ops(), sts, levels, 3)
    hmg.vcycle(c.g, hmg.BaseLevel(c.g), [c.A] * levels, dsts, levels, 3)
    assert relerr(dsts[-1].x.to_host(), sts[-1].x) <= 1e-9
    assert relerr(dsts[-1].r.to_host(), sts[-1].r) <= 1e-8
    for s in dsts:
        s.close()


def test_exact_savings_are_exact_level10(ctx):
    """Every exact saving of hmg_vcycle on and off on a 10-level 2D grid: x and r after two V-cycles are the same bits."""
    levels = 10
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tri64, 4, levels, seed=11)     # 32 triangles
    res = []
    try:
        for on in (1, 0):
            for o in EXACT_OPTIONS:
                ctx.set_option(o, on)
            ctx.set_option("lazy_top", 2 if on else 0)
            st = [hmg.LevelState(g, i + 1) for i in range(levels)]
            st[-1].x.rand(3); st[-1].b.rand(4)
            hmg.broadcast_interfaces(st[-1].x, g, levels)
            hmg.apply_constraint(st[-1].x, levels, g)
            bl = hmg.BaseLevel(g)
            for _ in range(2):
                hmg.vcycle(g, bl, [op] * levels, st, levels, 3)
            res.append((st[-1].x.to_host(), st[-1].r.to_host(), hmg.norm_unique(st[-1].r)))
            for s in st:
                s.close()
    finally:
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 1)
        ctx.set_option("lazy_top", 2)
        g.close()
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_driver_integrals_and_rhs_level10(cases):
    """hmg_integrate modes 0 / 1 / 2, next_rhs! and rhs_a xi grad v! on level 10."""
    c = cases[10]
    O, lev = c.O, 10
    xi = np.array([0.6, -0.8])
    mass = O.mass_matrix(c.impl.reference.levels[-1])
    dphis = O.partial_derivatives_functionals(c.impl.reference.levels[-1])
    want = np.zeros((c.impl.nf(lev), c.mesh.nelements()), order="F")
    O.rhs_axi_grad_v(want, dphis, c.impl, c.sig, xi)
    db = hmg.DeviceMatrix(c.g, lev)
    hmg.rhs_axi_grad_v(db, c.g, xi)
    assert relerr(db.to_host(), want) <= 1e-12
    v, w = c.rand(lev), c.rand(lev)
    dv, dw = c.dev(lev, v), c.dev(lev, w)
    for nsub in (7, c.mesh.nelements()):
        a = O.integrate_first_term(v, dphis, c.impl, nsub, mass, c.sig, xi)
        assert abs(hmg.integrate_first_term(dv, c.g, nsub, xi, b=db) - a) <= 1e-11 * max(abs(a), 1.0)
        b = O.integrate_terms(v, w, c.impl, nsub, mass)
        assert abs(hmg.integrate_terms(dv, dw, c.g, nsub) - b) <= 1e-11 * max(abs(b), 1.0)
        ar = O.integrate_area(mass, c.impl, nsub)
        assert abs(hmg.integrate_area(dv, c.g, nsub) - ar) <= 1e-12 * max(ar, 1.0)
    want2 = np.zeros_like(v, order="F")
    O.next_rhs(want2, v, c.impl, mass, c.lam)
    hmg.next_rhs(db, dv, c.g)
    assert relerr(db.to_host(), want2) <= 1e-12


def test_checkerboard_homogenization_refinements8(oracle):
    """checkerboard_homogenization(0, Tri64, refinements=8): 200 triangles, 9 levels, against the oracle with the same field and x0."""
    n, refinements = 0, 8
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sgrid = driver.generate_conductivity(2, width, 41)
    m = 2 ** refinements
    x0 = hmg.host_random(((m + 1) * (m + 2) // 2, 2 * width ** 2), 141)
    want, hist_o = oracle.checkerboard_homogenization(n=n, dim=2, refinements=refinements, tolerance=1e-3, sigma_grid=sgrid, x0=x0)
    ctx = hmg.Context(0)
    try:
        got, hist_d = driver.checkerboard_homogenization(n, hmg.Tri64, refinements=refinements, tolerance=1e-3, ctx=ctx,
                                                         sigma_grid=sgrid, x0=x0)
        assert ctx.counter("rows_launches") > 0
    finally:
        ctx.close()
    assert [h[:2] for h in hist_d] == [h[:2] for h in hist_o]            # same V-cycles per outer step
    assert abs(got - want) <= 1e-8
