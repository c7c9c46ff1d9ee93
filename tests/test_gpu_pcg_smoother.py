"""
The Jacobi-preconditioned CG smoother on the device (include/hmg.h: hmg_grid_set_smoother, csrc/hmg_pcg.hip, smooth_pcg() in
csrc/hmg_smooth.cpp, api.set_smoother / smoother_diag, the drivers' `smoother="jacobi"`) against its two CPU statements
(tests/_pcg_smoother_form.py): the inverse diagonal, the smoother by itself, the V-cycle, the flexible CG around it, lifetimes
and the drivers.  Tolerances are those the CG smoother is held to: dinv 1e-11 of the level's largest entry (the apply
tolerance), x, r, p of a smoother 1e-10 (tests/test_gpu_parity.py), x 1e-9 and r 1e-8 after V-cycles, alpha and beta 1e-8.
Partitioned grids: tests/test_gpu_pcg_smoother_dist.py.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

from _fcg_form import fcg_local, local_problem
from _pcg_smoother_form import (JacobiGlobalForm, JacobiOracle, convergence_case, inverse_diagonal, inverse_diagonals,
                                residual_history, smoothing_steps_jacobi, vcycle_jacobi)

pytestmark = pytest.mark.gpu

EXACT_OPTIONS = ("lean_post", "lazy_post", "lazy_top", "lazy_dead", "fold_x", "swap_rp", "fold_prolong", "prolong_in_image", "fold_faces",
                 "fold_restrict", "zero_entry", "cell_order")


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Problem:
    """Oracle-side objects of one mesh (operators and inverse diagonals level by level, on demand) and device grids of it."""

    def __init__(self, O, mesh, levels, lam, seed, values=(1.0, 9.0), sig=None):
        self.O, self.mesh, self.levels, self.lam = O, mesh, levels, lam
        self.rng = np.random.default_rng(seed)
        self.sig = self.rng.choice(list(values), size=(mesh.nelements(), mesh.dim)) if sig is None else sig
        self.impl = O.ImplicitFineGrid.create(mesh, levels)
        self.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(mesh))
        self._ops, self._dinv = {}, {}

    def op(self, lev):
        if lev not in self._ops:
            O, l = self.O, self.impl.reference.levels[lev - 1]
            self._ops[lev] = O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), self.cons, self.lam, self.sig)
        return self._ops[lev]

    def ops(self):
        return [self.op(l) for l in range(1, self.levels + 1)]

    def dinv(self, lev):
        if lev not in self._dinv:
            self._dinv[lev] = inverse_diagonal(self.O, self.impl, self.op(lev), lev)
        return self._dinv[lev]

    def dinvs(self):
        return [None] + [self.dinv(l) for l in range(2, self.levels + 1)]

    def device(self, ctx, fused=1, kind="jacobi"):
        ctx.set_option("fuse_cg", fused)                      # (read when a grid is created)
        try:
            g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.mesh.nodes, self.mesh.elements + 1), self.levels)
        finally:
            ctx.set_option("fuse_cg", 1)
        g.set_smoother(kind)
        return g, hmg.L2PlusDivAGrad(g, self.lam, self.sig)

    def state(self, lev):
        O = self.O
        st = O.LevelState.create(self.mesh.nelements(), self.impl.nf(lev))
        st.x[...] = self.rng.standard_normal(st.x.shape)
        O.broadcast_interfaces(st.x, self.impl, lev)
        O.apply_constraint(st.x, lev, self.cons, self.impl)
        st.b[...] = self.rng.standard_normal(st.x.shape)
        return st


def _cube(O, dim, n, perturb=0.0, seed=0, ordered=True):
    m = O.hypercube(dim, n, origin=(-n / 2.0,) * dim)
    if ordered:
        m = O.order_nodes_and_elements_by_magnitude(m)
    if perturb:
        m.nodes = m.nodes + perturb * (np.random.default_rng(seed).random(m.nodes.shape) - 0.5)
    return m


@pytest.fixture(scope="module")
def level7(oracle):
    """6 cells of 47 905 nodes, as test_level7_cells_larger_than_lds builds them"""
    return Problem(oracle, _cube(oracle, 3, 1, perturb=0.1, seed=13, ordered=False), 7, 0.9, 13)


@pytest.fixture(scope="module")
def level9(oracle):
    """32 triangles of 33 153 nodes, the smallest mesh of tests/test_gpu_tri_deep.py"""
    return Problem(oracle, _cube(oracle, 2, 4, perturb=0.2, seed=9), 9, 0.7, 9)


def _check_dinv(p, g, levels_checked):
    for lev in levels_checked:
        got = hmg.smoother_diag(g, lev).to_host()
        want = p.dinv(lev)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"level {lev}: dinv {err:.2e} (largest entry {np.abs(want).max():.3e})")
        assert err <= 1e-11, (lev, err)
        np.testing.assert_array_equal(got == 0.0, want == 0.0)        # zeros exactly where the constraint puts them
        assert (want == 0.0).any() and np.isfinite(got).all()


@pytest.mark.parametrize("name,dim,n,levels,lam,perturb", [("3d-width1", 3, 1, 6, 0.7, 0.0), ("3d-width1-lam0", 3, 1, 6, 0.0, 0.0),
                                                          ("3d-width2", 3, 2, 5, 0.0, 0.2), ("2d", 2, 4, 5, 0.7, 0.2),
                                                          ("2d-lam0", 2, 4, 5, 0.0, 0.0),
                                                          ("3d-1296-distinct-rows", 3, 6, 3, 0.7, 0.2)])
def test_inverse_diagonal_matches_the_cell_local_construction(oracle, ctx, name, dim, n, levels, lam, perturb):
    """hmg_grid_smoother_diag on every level >= 2 against the diagonal built from the oracle's operator tables, contrast 100.
    The last case has more distinct coefficient rows (1296 perturbed cells) than the class-weight cache takes."""
    p = Problem(oracle, _cube(oracle, dim, n, perturb=perturb, seed=3), levels, lam, 3, values=(1.0, 100.0))
    g, A = p.device(ctx)
    assert g.smoother() == "jacobi"
    _check_dinv(p, g, range(2, levels + 1))
    g.close()


def test_inverse_diagonal_level7(ctx, level7):
    g, A = level7.device(ctx)
    _check_dinv(level7, g, [7])
    g.close()


def test_inverse_diagonal_2d_level9(ctx, level9):
    g, A = level9.device(ctx)
    _check_dinv(level9, g, [9])
    g.close()


def _check_smoother(p, ctx, fused, levels_checked, shrink=None):
    O = p.O
    g, A = p.device(ctx, fused=fused)
    if shrink:
        g.shrink(*shrink)
    for lev in levels_checked:
        n = g.ld(lev) * g.ncells()
        for steps in (1, 2, 3):
            st = p.state(lev)
            dst = hmg.LevelState(g, lev)
            dst.x.from_host(st.x)
            dst.b.from_host(st.b)
            smoothing_steps_jacobi(O, steps, p.impl, p.op(lev), st, lev, p.dinv(lev))
            hmg.smoothing_steps(steps, g, A, dst, lev)
            ex, er, ep = relerr(dst.x.to_host(), st.x), relerr(dst.r.to_host(), st.r), relerr(dst.p.to_host(), st.p)
            print(f"level {lev} ({n} entries), {steps} steps, fuse_cg {fused}: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
            assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (lev, steps, ex, er, ep)
            dst.close()
    g.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_smoother_3d_levels_2_to_6(oracle, ctx, fused):
    """hmg_smooth with 1, 2 and 3 steps against the cell-local statement on every level of a 2 x 2 x 2 grid of 6 levels: the
    packed, pipelined, one-wave and register-blocked applies; Nf = 35, 165, 969, 6545 are odd, no length is a multiple of 512."""
    p = Problem(oracle, _cube(oracle, 3, 2, perturb=0.2, seed=21), 6, 0.7, 21, values=(1.0, 100.0))
    _check_smoother(p, ctx, fused, [2, 3, 4, 5, 6])


@pytest.mark.parametrize("fused", [1, 0])
def test_smoother_on_a_shrunk_grid_with_an_odd_number_of_entries(oracle, ctx, fused):
    """47 of 48 cells kept: 35 x 47 and 165 x 47 entries are odd, so flat pairs straddle columns and the tail entry runs."""
    O = oracle
    full = _cube(O, 3, 2, seed=22)
    sig = np.random.default_rng(22).choice([1.0, 100.0], size=(48, 3))
    sub = O.Mesh(full.nodes.copy(), np.ascontiguousarray(full.elements[:47]))
    p = Problem(O, sub, 4, 0.7, 22, sig=np.ascontiguousarray(sig[:47]))
    p_full = Problem(O, full, 4, 0.7, 22, sig=sig)
    p.device = p_full.device                                  # the device grid is created on all 48 cells, then shrunk
    assert (35 * 47) % 2 == 1 and (165 * 47) % 2 == 1
    _check_smoother(p, ctx, fused, [3, 4], shrink=(47, full.nnodes()))


@pytest.mark.parametrize("fused", [1, 0])
def test_smoother_level7(ctx, level7, fused):
    n0 = ctx.counter("slab2_launches")
    _check_smoother(level7, ctx, fused, [7])
    assert ctx.counter("slab2_launches") > n0


@pytest.mark.parametrize("fused", [1, 0])
def test_smoother_2d_level9(ctx, level9, fused):
    n0 = ctx.counter("rows_launches")
    _check_smoother(level9, ctx, fused, [9])
    assert ctx.counter("rows_launches") > n0


@pytest.mark.parametrize("dim,n,grids,contrast", [(3, 2, 4, 100), (3, 2, 5, 9), (2, 4, 5, 9)])
def test_vcycle_matches_both_statements(oracle, ctx, dim, n, grids, contrast):
    """One to three hmg_vcycle's of three smoothing steps against the global form (assembled matrices) and the cell-local one."""
    O, lam, steps = oracle, 1.0, 3
    rng = np.random.default_rng(23)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, float(contrast))
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    top = states[-1]
    top.x[...] = rng.random(top.x.shape)
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    O.local_rhs(top.b, implicit)
    G = JacobiGlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    gx, gb = G.gather(top.x, grids - 1), G.gather_sum(top.b, grids - 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids)
    g.set_smoother("jacobi")
    A = hmg.L2PlusDivAGrad(g, lam, cond)
    sts = [hmg.LevelState(g, i + 1) for i in range(grids)]
    sts[-1].x.from_host(top.x)
    sts[-1].b.from_host(top.b)
    bl = hmg.BaseLevel(g)
    base_level = O.make_base_level(base, cond, lam)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    for cycle in range(3):
        hmg.vcycle(g, bl, [A] * grids, sts, grids, steps)
        gx, gr = G.vcycle(grids - 1, gx, gb, steps)
        vcycle_jacobi(O, implicit, base_level, ops, states, grids, steps, dinvs)
        dx, dr = sts[-1].x.to_host(), sts[-1].r.to_host()
        eg = np.abs(G.gather(dx, grids - 1) - gx).max() / np.abs(gx).max()
        egr = np.abs(G.gather(dr, grids - 1) - gr).max() / np.abs(gr).max()
        el, elr = relerr(dx, top.x), relerr(dr, top.r)
        print(f"cycle {cycle + 1}: global x {eg:.2e} r {egr:.2e}  cell-local x {el:.2e} r {elr:.2e}")
        assert eg <= 1e-9 and egr <= 1e-8 and el <= 1e-9 and elr <= 1e-8, (cycle, eg, egr, el, elr)
    for s in sts:
        s.close()
    g.close()


def _run_vcycles(ctx, g, op, levels, cycles, steps=3, split=False):
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(3)
    st[-1].b.rand(4)
    hmg.broadcast_interfaces(st[-1].x, g, levels)
    hmg.apply_constraint(st[-1].x, levels, g)
    bl = hmg.BaseLevel(g)
    ctx.sync()
    allocs = ctx.counter("device_allocs")
    for _ in range(cycles):
        if split:
            hmg.vcycle_down(g, [op] * levels, st, levels, steps)
            hmg.vcycle(g, bl, [op] * levels, st, levels - 1, 2)
            hmg.vcycle_up(g, [op] * levels, st, levels, steps)
        else:
            hmg.vcycle(g, bl, [op] * levels, st, levels, steps)
    ctx.sync()
    during = ctx.counter("device_allocs") - allocs
    out = st[-1].x.to_host(), st[-1].r.to_host(), during
    for s in st:
        s.close()
    return out


@pytest.mark.parametrize("dim,n,levels", [(3, 4, 4), (3, 2, 6), (2, 8, 5)])
def test_vcycle_bits(ctx, dim, n, levels):
    """hmg_vcycle_down + hmg_vcycle(k - 1) + hmg_vcycle_up give the bits of hmg_vcycle; the exact savings that stay on with this
    smoother (folded prolongation, cell order, ...) give the bits of all of them off; a second run on fresh vectors gives the
    same bits; no V-cycle allocates."""
    tag = hmg.Tet64 if dim == 3 else hmg.Tri64
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, n, levels, seed=11, values=(1.0, 100.0))
    try:
        g.set_smoother("jacobi")
        ref = _run_vcycles(ctx, g, op, levels, 2)
        again = _run_vcycles(ctx, g, op, levels, 2)
        split = _run_vcycles(ctx, g, op, levels, 2, split=True)
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 0)
        off = _run_vcycles(ctx, g, op, levels, 2)
    finally:
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 1)
        ctx.set_option("lazy_top", 2)
        g.close()
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0
    for name, other in (("again", again), ("down + vcycle + up", split), ("savings off", off)):
        np.testing.assert_array_equal(ref[0], other[0], err_msg=name)
        np.testing.assert_array_equal(ref[1], other[1], err_msg=name)
        assert other[2] == 0, name                                # setup is over once the level vectors exist: no V-cycle allocates
    assert ref[2] == 0


def test_convergence_at_contrast_100(oracle, ctx):
    """The case of test_jacobi_smoother_contracts_where_cg_stalls_at_contrast_100 (3D, n = 4, four grids, lambda = 0, sigma in
    {1, 100}, local_rhs, 14 V-cycles of three steps) on the statement's mesh and coefficients: the 14 residual norms agree with the
    statement's to 1e-6 relative, the factor of the last six cycles is <= 0.62."""
    O, levels = oracle, 4
    case = convergence_case(O)
    base, cond, x0 = case[0], case[1], case[7]
    want = residual_history(O, case, "jacobi")
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), levels)
    g.set_smoother("jacobi")
    A = hmg.L2PlusDivAGrad(g, 0.0, cond)
    sts = [hmg.LevelState(g, i + 1) for i in range(levels)]
    sts[-1].x.from_host(x0)
    hmg.local_rhs(sts[-1].b, g)
    bl = hmg.BaseLevel(g)
    rs = []
    for _ in range(14):
        hmg.vcycle(g, bl, [A] * levels, sts, levels, 3)
        rs.append(hmg.norm_unique(sts[-1].r))
    rs = np.array(rs)
    for s in sts:
        s.close()
    g.close()
    f = (rs[13] / rs[7]) ** (1.0 / 6.0)
    print(f"device {rs[0]:.6e} ... {rs[13]:.6e}, statement {want[0]:.6e} ... {want[13]:.6e}, factor {f:.3f}, "
          f"largest relative difference {np.abs(rs / want - 1).max():.2e}")
    assert np.abs(rs / want - 1).max() <= 1e-6
    assert f <= 0.62


@pytest.mark.parametrize("dim,n,levels", [(3, 2, 4), (2, 4, 5)])
def test_fcg_around_the_jacobi_vcycle(oracle, ctx, dim, n, levels):
    """hmg_fcg_* on a grid with smoother 1 against fcg_local with the Jacobi statement as its V-cycle; a step after
    hmg_grid_set_smoother without a new start is the stale-state error."""
    O, lam, steps = oracle, 1.0, 3
    p = Problem(O, O.hypercube(dim, n), levels, lam, 40 + dim, values=(1.0, 100.0))
    states = [O.LevelState.create(p.mesh.nelements(), p.impl.nf(i + 1)) for i in range(levels)]
    x0 = p.state(levels).x
    b = np.asfortranarray(p.rng.standard_normal(x0.shape))
    g, A = p.device(ctx)
    sts = [hmg.LevelState(g, i + 1) for i in range(levels)]
    x, bd = hmg.DeviceMatrix(g, levels).from_host(x0), hmg.DeviceMatrix(g, levels).from_host(b)
    f = hmg.FlexibleCG(g, hmg.BaseLevel(g), [A] * levels, sts, levels, steps)
    f.start(x, bd)
    r0 = np.abs(f.vec("R")).max()
    loc = fcg_local(JacobiOracle(O, p.dinvs()), p.impl, O.make_base_level(p.mesh, p.sig, lam), p.ops(), states, levels, steps, x0, b)
    for it in range(3):
        wx, wR, wp, wa, wb = next(loc)
        f.step()
        alpha, beta, pq, pr = f.scalars()
        ex, eR = relerr(x.to_host(), wx), np.abs(f.vec("R") - wR).max() / r0
        print(f"step {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.12g} / {wa:.12g}  beta {beta:.12g} / {wb:.12g}")
        assert ex <= 1e-9 and eR <= 1e-8, (it, ex, eR)
        assert abs(alpha - wa) <= 1e-8 * abs(wa) and abs(beta - wb) <= 1e-8 * abs(wb), (it, alpha, wa, beta, wb)
    ctx.sync()
    allocs = ctx.counter("device_allocs")                         # (downloads above allocate staging memory; steps do not)
    for _ in range(2):
        f.step()
    ctx.sync()
    assert ctx.counter("device_allocs") == allocs
    g.set_smoother("cg")
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        f.step()
    f.start(x, bd)
    f.step()
    g.set_smoother("jacobi")
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        f.step()
    f.close()
    g.close()


def test_lifetimes_and_counters(oracle, ctx):
    """The inverse diagonals are setup memory with a reported size; they are formed once per operator, lambda and domain; after
    a shrink the device matches the statement on the shrunk mesh; kind 0 after kind 1 gives the bits of a grid that never saw
    kind 1."""
    O, levels = oracle, 3
    mesh = _cube(O, 3, 6)
    p = Problem(O, mesh, levels, 0.5, 5)
    bytes0, builds0 = ctx.counter("smoother_diag_bytes"), ctx.counter("smoother_diag_builds")
    g, A = p.device(ctx, kind="cg")
    assert g.smoother() == "cg" and ctx.counter("smoother_diag_bytes") == bytes0
    with pytest.raises(HmgError, match="hmg_grid_set_smoother"):
        hmg.smoother_diag(g, 2)
    never = _run_vcycles(ctx, g, A, levels, 2)
    g.set_smoother("jacobi")
    assert ctx.counter("smoother_diag_bytes") - bytes0 == 8 * sum(g.ld(l) * g.ncells() for l in range(2, levels + 1))
    assert ctx.counter("smoother_diag_builds") == builds0                         # formed at the first call that smooths
    _run_vcycles(ctx, g, A, levels, 1)
    assert ctx.counter("smoother_diag_builds") == builds0 + 1
    jac = _run_vcycles(ctx, g, A, levels, 2)
    assert ctx.counter("smoother_diag_builds") == builds0 + 1 and jac[2] == 0
    assert not np.array_equal(jac[0], never[0])
    A.lam = 0.25                                                                 # hmg_grid_set_lambda
    hmg.smoother_diag(g, 2).close()
    assert ctx.counter("smoother_diag_builds") == builds0 + 2
    g.set_operator(p.sig * 2.0, 0.25)
    _run_vcycles(ctx, g, A, levels, 1)
    assert ctx.counter("smoother_diag_builds") == builds0 + 3
    # shrink: against the statement on the shrunk mesh
    ne, nn = O.find_elements_in_radius(mesh, 2), O.find_nodes_in_radius(mesh, 2)
    sub = Problem(O, O.Mesh(mesh.nodes[:nn], np.ascontiguousarray(mesh.elements[:ne])), levels, 0.25, 6,
                  sig=np.ascontiguousarray(p.sig[:ne] * 2.0))
    dsts = [hmg.LevelState(g, i + 1) for i in range(levels)]
    x_full = np.asfortranarray(p.rng.standard_normal((35, mesh.nelements())))
    b_full = np.asfortranarray(p.rng.standard_normal((35, mesh.nelements())))
    dsts[-1].x.from_host(x_full)
    dsts[-1].b.from_host(b_full)
    g.shrink(ne, nn)
    hmg.broadcast_interfaces(dsts[-1].x, g, levels)
    hmg.apply_constraint(dsts[-1].x, levels, g)
    sts = [O.LevelState.create(ne, sub.impl.nf(i + 1)) for i in range(levels)]
    sts[-1].x[...] = x_full[:, :ne]
    sts[-1].b[...] = b_full[:, :ne]
    O.broadcast_interfaces(sts[-1].x, sub.impl, levels)
    O.apply_constraint(sts[-1].x, levels, sub.cons, sub.impl)
    vcycle_jacobi(O, sub.impl, O.make_base_level(sub.mesh, sub.sig, 0.25), sub.ops(), sts, levels, 3, sub.dinvs())
    hmg.vcycle(g, hmg.BaseLevel(g), [A] * levels, dsts, levels, 3)
    assert ctx.counter("smoother_diag_builds") == builds0 + 4
    assert relerr(dsts[-1].x.to_host(), sts[-1].x) <= 1e-9
    assert relerr(dsts[-1].r.to_host(), sts[-1].r) <= 1e-8
    _check_dinv(sub, g, [2, 3])
    for s in dsts:
        s.close()
    g.set_smoother("cg")
    assert ctx.counter("smoother_diag_bytes") == bytes0 and g.smoother() == "cg"
    g.close()
    # kind 0 after kind 1 on a fresh grid of the first operator: the bits of the grid that never saw kind 1
    g, A = p.device(ctx, kind="jacobi")
    _run_vcycles(ctx, g, A, levels, 1)
    g.set_smoother("cg")
    back = _run_vcycles(ctx, g, A, levels, 2)
    g.close()
    assert ctx.counter("smoother_diag_bytes") == bytes0
    np.testing.assert_array_equal(back[0], never[0])
    np.testing.assert_array_equal(back[1], never[1])


def test_host_only_grid_and_bad_kind_are_refused(ctx):
    base = driver.hypercube(hmg.Tet64, 2)
    host = hmg.ImplicitFineGrid(None, base, 3)
    with pytest.raises(HmgError, match="device context"):
        host.set_smoother("jacobi")
    host.close()
    g = hmg.ImplicitFineGrid(ctx, base, 3)
    with pytest.raises(ValueError):
        g.set_smoother("gauss-seidel")
    with pytest.raises(HmgError, match="kind"):
        hmg._lib.check(g._lib.hmg_grid_set_smoother(g.h, 2))
    g.close()


_NF = {2: [3, 6, 15, 45, 153], 3: [4, 10, 35, 165, 969]}


@pytest.mark.parametrize("dim,refinements", [(2, 3), (3, 1), (3, 2)])
def test_driver_converges_to_the_direct_fem_answer(oracle, ctx, dim, refinements):
    """The cases of test_driver_converges_to_the_direct_fem_answer (n = 0, tolerance 1e-12, field and xi from default_rng(8)) with
    smoother="jacobi": the sparse direct solve's number to 1e-8."""
    from _textbook_fem import converged_first_term
    rng = np.random.default_rng(8)
    sgrid = np.where(rng.random((10,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    xi = rng.standard_normal(dim)
    xi /= np.linalg.norm(xi)
    el = hmg.Tet64 if dim == 3 else hmg.Tri64
    tm = {}
    sigma, hist = driver.checkerboard_homogenization(0, el, refinements=refinements, tolerance=1e-12, xi=xi, sigma_grid=sgrid, ctx=ctx,
                                                     max_cycles=60, smoother="jacobi", timings=tm)
    want = converged_first_term(oracle, dim, sgrid, xi, refinements)
    print(f"{len(hist)} cycles, sigma - want = {sigma - want:.3e}")
    assert tm["smoother"] == "jacobi"
    assert abs(sigma - want) <= 1e-8 * abs(want), (sigma, want, len(hist))


def test_driver_at_contrast_100_takes_fewer_cycles(ctx):
    """The case of test_accelerated_driver_at_contrast_100 (3D, sigma in {1, 100}, n = 1, two refinements, tolerance 1e-5):
    strictly fewer cycles than smoother="cg", the same sigma to 1e-3 (the two stop about a tolerance apart); `accelerate` and
    `smoother` combine."""
    rng = np.random.default_rng(7)
    n, refinements = 1, 2
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sgrid = np.where(rng.random((width,) * 3 + (3,)) < 0.5, 1.0, 100.0)
    x0 = rng.random((_NF[3][refinements], 6 * width ** 3))
    kw = dict(refinements=refinements, tolerance=1e-5, sigma_grid=sgrid, x0=x0, ctx=ctx)
    tm = {}
    plain, hist_p = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="cg", timings=tm, **kw)
    assert tm["smoother"] == "cg"
    sigma, hist = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="jacobi", **kw)
    both, hist_b = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="jacobi", accelerate=True, **kw)
    print(f"jacobi {len(hist)} cycles (sigma {sigma:.8f}), cg {len(hist_p)} cycles (sigma {plain:.8f}), "
          f"jacobi + accelerate {len(hist_b)} (sigma {both:.8f})")
    assert len(hist) < len(hist_p), (len(hist), len(hist_p))
    assert abs(sigma - plain) <= 1e-3 * abs(plain)
    assert abs(both - plain) <= 1e-3 * abs(plain)


def test_tensor_driver_with_the_keyword(ctx):
    """driver.checkerboard_homogenization_tensor(smoother="jacobi") against its "cg" run: every entry to 1e-3 of the largest."""
    kw = dict(refinements=2, tolerance=1e-5, ctx=ctx, seed=3, values=(1.0, 100.0))
    tm = {}
    S_cg, h_cg = driver.checkerboard_homogenization_tensor(0, hmg.Tet64, smoother="cg", **kw)
    S_j, h_j = driver.checkerboard_homogenization_tensor(0, hmg.Tet64, smoother="jacobi", timings=tm, **kw)
    print(f"cg {len(h_cg)} cycles, jacobi {len(h_j)} cycles, largest difference {np.abs(S_j - S_cg).max():.3e}")
    assert tm["smoother"] == "jacobi"
    assert np.abs(S_j - S_cg).max() <= 1e-3 * np.abs(S_cg).max()
