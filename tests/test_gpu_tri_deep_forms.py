"""
2D grids of 9 to 11 levels (the row-band apply of hmg_apply_rows.hip) in every form smooth_form() sends: the smoother with
1, 2 and 3 steps, fused and one kernel per statement; both halves of a V-cycle level with the exact savings on and off (one-step
smoothers: the dead step is step 0; one pending x-update in the local residual); whole V-cycles with other step counts, which
give the levels below the finest their roles (pre-smoother on a zero initial guess, post-smoother that keeps x only); a shrunk
grid whose level vectors keep their storage.  Against the CPU oracle on the perturbed Tri64 lattices of test_gpu_tri_deep.py.

The oracle's vcycle does not forward `steps` to the coarser levels (as the reference does not): vcycle_steps below restates its
recursion with a steps_coarse argument, and the first test holds the restatement against O.vcycle bit for bit.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from test_gpu_tri_deep import EXACT_OPTIONS, Case, relerr

gpu = pytest.mark.gpu

OPTS = ("swap_rp", "fold_x", "fold_prolong", "lazy_dead", "lean_post", "prolong_in_image", "fold_restrict")   # test_gpu_parity_l6.py
STEP_PAIRS = [(3, 2), (1, 1), (2, 3), (4, 1)]          # (steps on the finest level, steps on every level below)


def vcycle_steps(O, implicit, base, ops, levels, k, steps, steps_coarse):
    """O.vcycle (src/multigrid.jl:73-119) with `steps_coarse` CG steps on the levels below k instead of the default 2."""
    if k == 1:
        O.vcycle(implicit, base, ops, levels, 1)                         # the base solve
        return
    curr, nxt = levels[k - 1], levels[k - 2]
    P = implicit.reference.interops[k - 2]
    O.smoothing_steps(steps, implicit, ops[k - 1], curr, k)
    O.local_residual(implicit, ops[k - 1], curr, k)
    O.restrict_to(nxt.b, P, curr.r)
    nxt.x.fill(0.0)
    vcycle_steps(O, implicit, base, ops, levels, k - 1, steps_coarse, steps_coarse)
    O.interpolate_and_sum_to(curr.x, P, nxt.x)
    O.smoothing_steps(steps, implicit, ops[k - 1], curr, k)


def test_restated_recursion_is_the_oracles(oracle):
    """vcycle_steps with steps_coarse = 2 against O.vcycle on a 4-level grid: every vector of every level after two cycles, the same
    bits (CPU only; on one thread: the oracle's threaded dot products do not add their partial sums in a fixed order, so two runs
    of O.vcycle itself differ in the last bits otherwise)."""
    O, levels = oracle, 4
    threads = O.NTHREADS[0]
    O.NTHREADS[0] = 1
    try:
        res, x0 = _both_recursions(O, levels)
    finally:
        O.NTHREADS[0] = threads
    assert np.abs(res[0][-1].x - x0).max() > 0
    for a, b in zip(*res):
        for name in ("x", "b", "r", "p", "Ap"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def _both_recursions(O, levels):
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, 3, origin=(-1.5, -1.5)))
    rng = np.random.default_rng(2)
    m.nodes = m.nodes + 0.2 * (rng.random(m.nodes.shape) - 0.5)
    sig = rng.choice([1.0, 9.0], size=(m.nelements(), 2))
    impl = O.ImplicitFineGrid.create(m, levels)
    cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(m))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, 0.7, sig) for l in impl.reference.levels]
    x0 = np.asfortranarray(rng.standard_normal((impl.nf(levels), m.nelements())))
    O.broadcast_interfaces(x0, impl, levels)
    O.apply_constraint(x0, levels, cons, impl)
    b0 = np.asfortranarray(rng.standard_normal(x0.shape))
    res = []
    for restated in (False, True):
        sts = [O.LevelState.create(m.nelements(), impl.nf(i + 1)) for i in range(levels)]
        sts[-1].x[...] = x0; sts[-1].b[...] = b0
        base = O.make_base_level(m, sig, 0.7)
        for _ in range(2):
            if restated:
                vcycle_steps(O, impl, base, ops, sts, levels, 3, 2)
            else:
                O.vcycle(impl, base, ops, sts, levels, 3)
        res.append(sts)
    return res, x0


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class FormCase(Case):
    """Case with one fixed initial state per level, the oracle's side of every step count computed once, and a second device grid
    without the fused CG pass (option fuse_cg is read when a grid is created)."""

    def __init__(self, O, ctx, n, levels, seed):
        super().__init__(O, ctx, n, levels, seed=seed)
        self.ctx = ctx
        st = self.state(levels)
        self.x0, self.b0 = st.x.copy(order="F"), st.b.copy(order="F")
        xc = self.rand(levels - 1)                                      # a consistent coarse correction
        O.broadcast_interfaces(xc, self.impl, levels - 1)
        O.apply_constraint(xc, levels - 1, self.cons, self.impl)
        self.xc = xc
        self._down, self._up, self._plain = {}, {}, None

    def fresh(self):
        st = self.O.LevelState.create(self.mesh.nelements(), self.impl.nf(self.levels))
        st.x[...] = self.x0; st.b[...] = self.b0
        return st

    def unfused(self):
        if self._plain is None:
            self.ctx.set_option("fuse_cg", 0)
            try:
                g = hmg.ImplicitFineGrid(self.ctx, hmg.Mesh(self.mesh.nodes, self.mesh.elements + 1), self.levels)
            finally:
                self.ctx.set_option("fuse_cg", 1)
            self._plain = (g, hmg.L2PlusDivAGrad(g, self.lam, self.sig))
        return self._plain

    def down(self, steps):
        """smoothing_steps! from (x0, b0): the smoother's state; then local_residual! and restrict_to!."""
        if steps not in self._down:
            O, lev = self.O, self.levels
            st = self.fresh()
            O.smoothing_steps(steps, self.impl, self.op(lev), st, lev)
            smoothed = {n: getattr(st, n).copy(order="F") for n in ("x", "r", "p", "Ap")}
            O.local_residual(self.impl, self.op(lev), st, lev)
            nb = np.zeros((self.impl.nf(lev - 1), self.mesh.nelements()), order="F")
            O.restrict_to(nb, self.impl.reference.interops[lev - 2], st.r)
            self._down[steps] = (smoothed, st.r, nb)
        return self._down[steps]

    def up(self, steps):
        """interpolate_and_sum_to!(x0, P, xc), smoothing_steps!."""
        if steps not in self._up:
            O, lev = self.O, self.levels
            st = self.fresh()
            O.interpolate_and_sum_to(st.x, self.impl.reference.interops[lev - 2], self.xc)
            O.smoothing_steps(steps, self.impl, self.op(lev), st, lev)
            self._up[steps] = st
        return self._up[steps]


@pytest.fixture(scope="module")
def cases(oracle, ctx):
    # 32 cells at level 9, 18 at level 10, 8 at level 11
    return {9: FormCase(oracle, ctx, 4, 9, 19), 10: FormCase(oracle, ctx, 3, 10, 20), 11: FormCase(oracle, ctx, 2, 11, 21)}


@gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("levels", [9, 10, 11])
def test_smoothing_steps(cases, ctx, levels, steps, fused):
    """smoothing_steps! called on the finest level, fused CG pass and one kernel per statement: x, r, p, Ap <= 1e-10."""
    c = cases[levels]
    g, A = (c.g, c.A) if fused else c.unfused()
    want = c.down(steps)[0]
    dst = hmg.LevelState(g, levels)
    try:
        dst.x.from_host(c.x0); dst.b.from_host(c.b0)
        n0 = ctx.counter("rows_launches")
        hmg.smoothing_steps(steps, g, A, dst, levels)
        assert ctx.counter("rows_launches") >= n0 + steps + 1
        errs = {n: relerr(getattr(dst, n).to_host(), want[n]) for n in ("x", "r", "p", "Ap")}
        print(f"smoothing_steps L={levels} steps={steps} fused={fused}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
        for n, e in errs.items():
            assert e <= 1e-10, (n, e)
    finally:
        dst.close()


@gpu
@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("levels", [9, 10, 11])
def test_vcycle_down_leg(cases, ctx, levels, steps, plain):
    """hmg.vcycle_down on the finest level (smoothing_steps!, local_residual!, restrict_to!, fill!(next.x, 0)), exact savings on
    (plain = 0: what hmg_vcycle runs -- steps >= 2: the dead step writes nothing and the residual applies two pending x-updates;
    steps = 1: the dead step is step 0, one pending update) and off: x, the cell-local r and the coarse right-hand side <= 1e-10,
    the coarse x all zeros, the row-band kernel at work."""
    c = cases[levels]
    smoothed, r_local, nb = c.down(steps)
    for o in OPTS:
        ctx.set_option(o, 0 if plain else 1)
    states = [None] * levels
    try:
        states[levels - 2], states[levels - 1] = hmg.LevelState(c.g, levels - 1), hmg.LevelState(c.g, levels)
        states[-1].x.from_host(c.x0); states[-1].b.from_host(c.b0)
        states[-2].x.from_host(c.rand(levels - 1))                       # must come back as zeros
        n0 = ctx.counter("rows_launches")
        hmg.vcycle_down(c.g, [c.A] * levels, states, levels, steps)
        assert ctx.counter("rows_launches") >= n0 + steps + 1
        errs = (relerr(states[-1].x.to_host(), smoothed["x"]), relerr(states[-1].r.to_host(), r_local),
                relerr(states[-2].b.to_host(), nb))
        print(f"vcycle_down L={levels} steps={steps} plain={plain}: x {errs[0]:.3e} r {errs[1]:.3e} b_coarse {errs[2]:.3e}")
        assert max(errs) <= 1e-10, errs
        assert not states[-2].x.to_host().any()
    finally:
        for o in OPTS:
            ctx.set_option(o, 1)
        for s in states:
            if s is not None:
                s.close()


@gpu
@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("levels", [9, 10, 11])
def test_vcycle_up_leg(cases, ctx, levels, steps, plain):
    """hmg.vcycle_up on the finest level (interpolate_and_sum_to!, smoothing_steps!) with a consistent coarse correction, exact
    savings on and off: x and r <= 1e-10; p and Ap too with the savings off (with them on the last p-update is dropped)."""
    c = cases[levels]
    want = c.up(steps)
    for o in OPTS:
        ctx.set_option(o, 0 if plain else 1)
    states = [None] * levels
    try:
        states[levels - 2], states[levels - 1] = hmg.LevelState(c.g, levels - 1), hmg.LevelState(c.g, levels)
        states[-1].x.from_host(c.x0); states[-1].b.from_host(c.b0)
        states[-2].x.from_host(c.xc)
        n0 = ctx.counter("rows_launches")
        hmg.vcycle_up(c.g, [c.A] * levels, states, levels, steps)
        assert ctx.counter("rows_launches") >= n0 + steps + 1
        names = ("x", "r", "p", "Ap") if plain else ("x", "r")
        errs = {n: relerr(getattr(states[-1], n).to_host(), getattr(want, n)) for n in names}
        print(f"vcycle_up L={levels} steps={steps} plain={plain}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
        for n, e in errs.items():
            assert e <= 1e-10, (n, e)
    finally:
        for o in OPTS:
            ctx.set_option(o, 1)
        for s in states:
            if s is not None:
                s.close()


@gpu
@pytest.mark.parametrize("levels,steps,steps_coarse", [(11,) + p for p in STEP_PAIRS] + [(10, 1, 1), (10, 2, 3)])
def test_vcycle_step_pairs(cases, levels, steps, steps_coarse):
    """Whole V-cycles with other step counts: the levels below the finest that go through the row-band kernel (9 and 10 of 11,
    9 of 10) are pre-smoothed from a zero initial guess and post-smoothed for x alone, forms only hmg_vcycle sends.  One and
    two cycles against the oracle's recursion with `steps_coarse` steps below the finest level: x <= 1e-9, r <= 1e-8."""
    c = cases[levels]
    O = c.O
    sts = [O.LevelState.create(c.mesh.nelements(), c.impl.nf(i + 1)) for i in range(levels)]
    sts[-1] = c.fresh()
    dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
    try:
        dsts[-1].x.from_host(c.x0); dsts[-1].b.from_host(c.b0)
        base, dbase = O.make_base_level(c.mesh, c.sig, c.lam), hmg.BaseLevel(c.g)
        for cyc in range(2):
            vcycle_steps(O, c.impl, base, c.all_ops(), sts, levels, steps, steps_coarse)
            hmg.vcycle(c.g, dbase, [c.A] * levels, dsts, levels, steps, steps_coarse)
            ex, er = relerr(dsts[-1].x.to_host(), sts[-1].x), relerr(dsts[-1].r.to_host(), sts[-1].r)
            print(f"vcycle L={levels} steps={steps}/{steps_coarse} cycle {cyc}: x {ex:.3e} r {er:.3e}")
            assert ex <= 1e-9, (cyc, ex)
            assert er <= 1e-8, (cyc, er)
    finally:
        for s in dsts:
            s.close()


@gpu
@pytest.mark.parametrize("steps,steps_coarse", STEP_PAIRS)
def test_exact_savings_are_exact_level10_step_pairs(ctx, steps, steps_coarse):
    """test_gpu_tri_deep.test_exact_savings_are_exact_level10 for every step pair: all exact savings of hmg_vcycle on and off on
    the 10-level checkerboard, x, r and norm_unique(r) after two V-cycles are the same bits."""
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
                hmg.vcycle(g, bl, [op] * levels, st, levels, steps, steps_coarse)
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


@gpu
def test_shrink_then_vcycle_level9(oracle, ctx):
    """test_gpu_parity.test_shrink_then_vcycle at 9 levels: the 32-cell grid shrunk to the cells / nodes within radius 1 (the
    8 triangles around the origin and their 9 nodes; radii taken on the lattice before its nodes are perturbed, which keeps the
    prefixes nested), level vectors created BEFORE the shrink.  One V-cycle against the oracle on the sub-mesh: x <= 1e-9,
    r <= 1e-8; the wide prolongation and the wide norm, which take the cell count from the shrunk mesh, bit for bit and
    restrict_to! to 1e-14."""
    O, levels = oracle, 9
    flat = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, 4, origin=(-2.0, -2.0)))
    ne, nn = O.find_elements_in_radius(flat, 1), O.find_nodes_in_radius(flat, 1)
    assert 8 <= ne <= 24 and nn >= 9
    c = Case(O, ctx, 4, levels, seed=29)
    np.testing.assert_array_equal(c.mesh.elements, flat.elements)
    assert c.mesh.elements[:ne].max() < nn
    sub = O.Mesh(c.mesh.nodes[:nn], np.ascontiguousarray(c.mesh.elements[:ne]))
    sig = np.ascontiguousarray(c.sig[:ne])
    impl = O.ImplicitFineGrid.create(sub, levels)
    cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(sub))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, c.lam, sig) for l in impl.reference.levels]
    x_full, b_full = c.rand(levels), c.rand(levels)
    f_full, c_full = c.rand(levels), c.rand(levels - 1)
    dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
    df, dc, dcb = c.dev(levels, f_full), c.dev(levels - 1, c_full), hmg.DeviceMatrix(c.g, levels - 1)
    dsts[-1].x.from_host(x_full); dsts[-1].b.from_host(b_full)
    c.g.shrink(ne, nn)
    assert c.g.ncells() == ne
    # transfers and the unique-copy norm on the shrunk grid (a vector of the shrunk grid is the prefix of its columns)
    P = impl.reference.interops[levels - 2]
    wantb = np.zeros((impl.nf(levels - 1), ne), order="F")
    O.restrict_to(wantb, P, np.asfortranarray(f_full[:, :ne]))
    hmg.restrict_to(dcb, c.g, df)
    assert relerr(dcb.to_host(), wantb) <= 1e-14
    wantf = np.asfortranarray(f_full[:, :ne]); O.interpolate_and_sum_to(wantf, P, np.asfortranarray(c_full[:, :ne]))
    hmg.interpolate_and_sum_to(df, c.g, dc)
    np.testing.assert_array_equal(df.to_host(), wantf)
    O.broadcast_interfaces(wantf, impl, levels)
    hmg.broadcast_interfaces(df, c.g, levels)
    np.testing.assert_array_equal(df.to_host(), wantf)
    uniq = wantf.copy(order="F"); O.zero_out_all_but_one(uniq, impl, levels)
    assert abs(hmg.norm_unique(df) - np.linalg.norm(uniq)) <= 1e-13 * np.linalg.norm(uniq)
    hmg.zero_out_all_but_one(df, c.g, levels)
    np.testing.assert_array_equal(df.to_host(), uniq)
    # one V-cycle
    hmg.broadcast_interfaces(dsts[-1].x, c.g, levels)
    hmg.apply_constraint(dsts[-1].x, levels, c.g)
    sts = [O.LevelState.create(ne, impl.nf(i + 1)) for i in range(levels)]
    sts[-1].x[...] = x_full[:, :ne]; sts[-1].b[...] = b_full[:, :ne]
    O.broadcast_interfaces(sts[-1].x, impl, levels)
    O.apply_constraint(sts[-1].x, levels, cons, impl)
    O.vcycle(impl, O.make_base_level(sub, sig, c.lam), ops, sts, levels, 3)
    n0 = ctx.counter("rows_launches")
    hmg.vcycle(c.g, hmg.BaseLevel(c.g), [c.A] * levels, dsts, levels, 3)
    assert ctx.counter("rows_launches") > n0
    ex = relerr(dsts[-1].x.to_host(), sts[-1].x)
    er = relerr(dsts[-1].r.to_host(), sts[-1].r)
    print(f"shrink L=9 {ne} of {c.mesh.nelements()} cells: x {ex:.3e} r {er:.3e}")
    assert ex <= 1e-9
    assert er <= 1e-8
