"""
The Chebyshev-Jacobi smoother on the device (include/hmg.h: hmg_grid_set_smoother_chebyshev, hmg_grid_smoother_bounds,
csrc/hmg_cheb.hip, smooth_cheb() in csrc/hmg_smooth.cpp, api.set_smoother / smoother_bounds, the drivers' `smoother="chebyshev"`)
against its two CPU statements (tests/_cheb_smoother_form.py): the bound, the smoother by itself, the V-cycle, the flexible CG
around it, lifetimes, refusals, a partitioned grid with explicit bounds, and the drivers.  Tolerances are those the Jacobi
smoother is held to: the bound 1e-11 (the dinv tolerance), x, r, p of a smoother 1e-10, x 1e-9 and r 1e-8 after V-cycles, alpha and
beta 1e-8.  The helpers and fixtures are those of tests/test_gpu_pcg_smoother.py.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

from _cheb_smoother_form import (CONVERGENCE_PIN, DEFAULT_RATIO, ChebGlobalForm, ChebOracle, bounds_local, inverse_diagonals,
                                 lambda_hi_local, residual_history_cheb, smoothing_steps_cheb, vcycle_cheb)
from _fcg_form import fcg_local, local_problem
from _pcg_smoother_form import convergence_case
from test_gpu_pcg_smoother import EXACT_OPTIONS, Problem, _NF, _cube, _run_vcycles, ctx, level7, level9, relerr  # noqa: F401

pytestmark = pytest.mark.gpu


def _hi(p, lev):
    """the statement's bound of a level of a test_gpu_pcg_smoother.Problem"""
    cache = p.__dict__.setdefault("_cheb_hi", {})
    if lev not in cache:
        cache[lev] = lambda_hi_local(p.O, p.impl, p.op(lev), lev, p.dinv(lev))
    return cache[lev]


def _check_bounds(p, g, ctx, levels_checked, ratio=DEFAULT_RATIO):
    for lev in levels_checked:
        lo, hi = hmg.smoother_bounds(g, lev)
        want = _hi(p, lev)
        print(f"level {lev}: lambda_hi {hi:.12f}, statement {want:.12f}, relative difference {abs(hi - want) / want:.2e}")
        assert abs(hi - want) <= 1e-11 * want, (lev, hi, want)
        assert lo == hi / ratio
        # not a property of the bound: of the default Dirichlet set on the meshes this helper is called with.  With the constraint
        # lifted the 2D case of tests/test_gpu_cheb_smoother_cross.py gives 6.39 > 3.06 (tests/test_cheb_smoother_statement.py)
        assert hi <= 1.02 * (p.mesh.dim + 1) * (1 + 1e-12)
    n0 = ctx.counter("smoother_bound_builds")
    again = [hmg.smoother_bounds(g, lev) for lev in levels_checked]
    assert ctx.counter("smoother_bound_builds") == n0                    # a second query forms nothing
    assert again == [hmg.smoother_bounds(g, lev) for lev in levels_checked]


@pytest.mark.parametrize("name,dim,n,levels,lam,perturb", [("3d-width1", 3, 1, 6, 0.7, 0.0), ("3d-width1-lam0", 3, 1, 6, 0.0, 0.0),
                                                          ("3d-width2", 3, 2, 5, 0.0, 0.2), ("2d", 2, 4, 5, 0.7, 0.2),
                                                          ("3d-1296-distinct-rows", 3, 6, 3, 0.7, 0.2)])
def test_bound_matches_the_statement(oracle, ctx, name, dim, n, levels, lam, perturb):
    """hmg_grid_smoother_bounds on every level >= 2 against the bound formed from the oracle's operator tables, contrast 100; lo =
    hi / ratio; a second query forms nothing; after set_lambda and after a shrink the bound is formed again."""
    p = Problem(oracle, _cube(oracle, dim, n, perturb=perturb, seed=3), levels, lam, 3, values=(1.0, 100.0))
    g, A = p.device(ctx, kind="chebyshev")
    assert g.smoother() == "chebyshev"
    n0 = ctx.counter("smoother_bound_builds")
    _check_bounds(p, g, ctx, range(2, levels + 1))
    assert ctx.counter("smoother_bound_builds") == n0 + levels - 1
    A.lam = lam + 0.25                                                   # hmg_grid_set_lambda
    lo, hi = hmg.smoother_bounds(g, 2)
    assert ctx.counter("smoother_bound_builds") == n0 + levels
    p2 = Problem(oracle, p.mesh, levels, lam + 0.25, 3, sig=p.sig)
    assert abs(hi - _hi(p2, 2)) <= 1e-11 * hi
    g.set_smoother("chebyshev", ratio=16.0)
    lo, hi = hmg.smoother_bounds(g, 2)
    assert lo == hi / 16.0 and abs(hi - _hi(p2, 2)) <= 1e-11 * hi
    g.close()


def test_bound_after_a_shrink(oracle, ctx):
    O, levels = oracle, 3
    mesh = _cube(O, 3, 6)
    p = Problem(O, mesh, levels, 0.5, 5, values=(1.0, 100.0))
    g, A = p.device(ctx, kind="chebyshev")
    before = hmg.smoother_bounds(g, 3)
    n0 = ctx.counter("smoother_bound_builds")
    ne, nn = O.find_elements_in_radius(mesh, 2), O.find_nodes_in_radius(mesh, 2)
    g.shrink(ne, nn)
    sub = Problem(O, O.Mesh(mesh.nodes[:nn], np.ascontiguousarray(mesh.elements[:ne])), levels, 0.5, 6, sig=np.ascontiguousarray(p.sig[:ne]))
    _check_bounds(sub, g, ctx, [2, 3])
    assert ctx.counter("smoother_bound_builds") == n0 + 2
    assert np.isfinite(before).all()
    g.close()


def test_bound_level7(ctx, level7):
    g, A = level7.device(ctx, kind="chebyshev")
    _check_bounds(level7, g, ctx, [7])
    g.close()


def test_bound_2d_level9(ctx, level9):
    g, A = level9.device(ctx, kind="chebyshev")
    _check_bounds(level9, g, ctx, [9])
    g.close()


def _check_smoother(p, ctx, levels_checked, shrink=None, explicit=False):
    """x, r, p of hmg_smooth against the cell-local statement run with the STATEMENT's bound.  explicit: the device is given the
    bound it formed itself: the same bits as without."""
    O = p.O
    g, A = p.device(ctx, kind="chebyshev")
    if shrink:
        g.shrink(*shrink)
    for lev in levels_checked:
        n = g.ld(lev) * g.ncells()
        hi = _hi(p, lev)
        for steps in (1, 2, 3):
            st = p.state(lev)
            dst = hmg.LevelState(g, lev)
            dst.x.from_host(st.x)
            dst.b.from_host(st.b)
            a0, s0 = ctx.counter("cheb_applies"), ctx.counter("cheb_smoothings")
            smoothing_steps_cheb(O, steps, p.impl, p.op(lev), st, lev, p.dinv(lev), hi / DEFAULT_RATIO, hi)
            hmg.smoothing_steps(steps, g, A, dst, lev)
            assert ctx.counter("cheb_applies") == a0 + steps and ctx.counter("cheb_smoothings") == s0 + 1
            got = dst.x.to_host(), dst.r.to_host(), dst.p.to_host()
            ex, er, ep = relerr(got[0], st.x), relerr(got[1], st.r), relerr(got[2], st.p)
            print(f"level {lev} ({n} entries), {steps} steps: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
            assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (lev, steps, ex, er, ep)
            if explicit and steps == 3:
                his = [0.0] * p.levels
                his[lev - 1] = hmg.smoother_bounds(g, lev)[1]
                g.set_smoother("chebyshev", lambda_hi=his)
                n0 = ctx.counter("smoother_bound_builds")
                p_x = np.asfortranarray(got[0])                                  # a consistent start, the same for both runs
                dst.x.from_host(p_x)
                hmg.smoothing_steps(steps, g, A, dst, lev)
                given = dst.x.to_host(), dst.r.to_host(), dst.p.to_host()
                assert ctx.counter("smoother_bound_builds") == n0
                assert hmg.smoother_bounds(g, lev)[1] == his[lev - 1]
                g.set_smoother("chebyshev")
                dst.x.from_host(p_x)
                hmg.smoothing_steps(steps, g, A, dst, lev)
                for a, b in zip(given, (dst.x.to_host(), dst.r.to_host(), dst.p.to_host())):
                    np.testing.assert_array_equal(a, b)
            dst.close()
    g.close()


def test_smoother_3d_levels_2_to_6(oracle, ctx):
    """hmg_smooth with 1, 2 and 3 steps against the cell-local statement on every level of a 2 x 2 x 2 grid of 6 levels: the
    packed, pipelined, one-wave and register-blocked applies; Nf = 35, 165, 969, 6545 are odd, no length is a multiple of 512.  An
    explicit bound equal to the formed one gives the formed one's bits."""
    p = Problem(oracle, _cube(oracle, 3, 2, perturb=0.2, seed=21), 6, 0.7, 21, values=(1.0, 100.0))
    _check_smoother(p, ctx, [2, 3, 4, 5, 6], explicit=True)


def test_smoother_on_a_shrunk_grid_with_an_odd_number_of_entries(oracle, ctx):
    """47 of 48 cells kept: 35 x 47 and 165 x 47 entries are odd, so flat pairs straddle columns and the tail entry runs."""
    O = oracle
    full = _cube(O, 3, 2, seed=22)
    sig = np.random.default_rng(22).choice([1.0, 100.0], size=(48, 3))
    sub = O.Mesh(full.nodes.copy(), np.ascontiguousarray(full.elements[:47]))
    p = Problem(O, sub, 4, 0.7, 22, sig=np.ascontiguousarray(sig[:47]))
    p_full = Problem(O, full, 4, 0.7, 22, sig=sig)
    p.device = p_full.device                                  # the device grid is created on all 48 cells, then shrunk
    assert (35 * 47) % 2 == 1 and (165 * 47) % 2 == 1
    _check_smoother(p, ctx, [3, 4], shrink=(47, full.nnodes()))


def test_smoother_level7(ctx, level7):
    n0 = ctx.counter("slab2_launches")
    _check_smoother(level7, ctx, [7])
    assert ctx.counter("slab2_launches") > n0


def test_smoother_2d_level9(ctx, level9):
    n0 = ctx.counter("rows_launches")
    _check_smoother(level9, ctx, [9])
    assert ctx.counter("rows_launches") > n0


@pytest.mark.parametrize("dim,n,grids,contrast", [(3, 2, 4, 100), (3, 2, 5, 9), (2, 4, 5, 9)])
def test_vcycle_matches_both_statements(oracle, ctx, dim, n, grids, contrast):
    """One to three hmg_vcycle's of three smoothing steps against the global form (assembled matrices) and the cell-local one, both
    with the statement's bounds."""
    O, lam, steps = oracle, 1.0, 3
    rng = np.random.default_rng(23)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, float(contrast))
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    top = states[-1]
    top.x[...] = rng.random(top.x.shape)
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    O.local_rhs(top.b, implicit)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    his = bounds_local(O, implicit, ops, grids, dinvs)
    G = ChebGlobalForm(O, base, sgrid, lam, implicit, grids, dim).set_interval(his)
    gx, gb = G.gather(top.x, grids - 1), G.gather_sum(top.b, grids - 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids)
    g.set_smoother("chebyshev")
    A = hmg.L2PlusDivAGrad(g, lam, cond)
    sts = [hmg.LevelState(g, i + 1) for i in range(grids)]
    sts[-1].x.from_host(top.x)
    sts[-1].b.from_host(top.b)
    bl = hmg.BaseLevel(g)
    base_level = O.make_base_level(base, cond, lam)
    for cycle in range(3):
        hmg.vcycle(g, bl, [A] * grids, sts, grids, steps)
        gx, gr = G.vcycle(grids - 1, gx, gb, steps)
        vcycle_cheb(O, implicit, base_level, ops, states, grids, steps, dinvs, his)
        dx, dr = sts[-1].x.to_host(), sts[-1].r.to_host()
        eg = np.abs(G.gather(dx, grids - 1) - gx).max() / np.abs(gx).max()
        egr = np.abs(G.gather(dr, grids - 1) - gr).max() / np.abs(gr).max()
        el, elr = relerr(dx, top.x), relerr(dr, top.r)
        print(f"cycle {cycle + 1}: global x {eg:.2e} r {egr:.2e}  cell-local x {el:.2e} r {elr:.2e}")
        assert eg <= 1e-9 and egr <= 1e-8 and el <= 1e-9 and elr <= 1e-8, (cycle, eg, egr, el, elr)
    for s in sts:
        s.close()
    g.close()


@pytest.mark.parametrize("dim,n,levels", [(3, 4, 4), (3, 2, 6), (2, 8, 5)])
def test_vcycle_bits_and_applies(ctx, dim, n, levels):
    """hmg_vcycle_down + hmg_vcycle(k - 1) + hmg_vcycle_up give the bits of hmg_vcycle; the exact savings all on against all off
    give the same bits; a second run on fresh vectors gives the same bits; no V-cycle allocates.  A three-step pre-smoother launches
    two smoothing applies, and a V-cycle one apply fewer per smoothing whose x alone is read."""
    tag = hmg.Tet64 if dim == 3 else hmg.Tri64
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, n, levels, seed=11, values=(1.0, 100.0))
    try:
        g.set_smoother("chebyshev")
        ref = _run_vcycles(ctx, g, op, levels, 2)
        a0, s0 = ctx.counter("cheb_applies"), ctx.counter("cheb_smoothings")
        again = _run_vcycles(ctx, g, op, levels, 2)
        a1, s1 = ctx.counter("cheb_applies"), ctx.counter("cheb_smoothings")
        split = _run_vcycles(ctx, g, op, levels, 2, split=True)
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 0)
        off = _run_vcycles(ctx, g, op, levels, 2)
    finally:
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 1)
        ctx.set_option("lazy_top", 2)
    try:
        # per V-cycle: the top level's pre-smoother 3 - 1 applies and its post-smoother (x and r are read) 3; every level between
        # 2 and the top 2 - 1 and 2 - 1
        assert s1 - s0 == 2 * 2 * (levels - 1)
        assert a1 - a0 == 2 * ((3 - 1) + 3 + 2 * (levels - 2))
        st = [hmg.LevelState(g, i + 1) for i in range(levels)]
        st[-1].x.rand(3)
        st[-1].b.rand(4)
        a0 = ctx.counter("cheb_applies")
        hmg.vcycle_down(g, [op] * levels, st, levels, 3)
        assert ctx.counter("cheb_applies") == a0 + 2                      # three steps, two applies: the last step is x += d alone
        for s in st:
            s.close()
    finally:
        g.close()
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0
    for name, other in (("again", again), ("down + vcycle + up", split), ("savings off", off)):
        np.testing.assert_array_equal(ref[0], other[0], err_msg=name)
        np.testing.assert_array_equal(ref[1], other[1], err_msg=name)
        assert other[2] == 0, name                                # setup is over once the level vectors exist: no V-cycle allocates
    assert ref[2] == 0


def test_convergence_at_contrast_100(oracle, ctx):
    """convergence_case (3D, n = 4, four grids, lambda = 0, sigma in {1, 100}, local_rhs, 14 V-cycles of three steps) with the
    default ratio and the library's own bounds: the 14 residual norms agree with the statement's to 1e-6 relative, the factor of
    the last six cycles is within the pin of tests/test_cheb_smoother_statement.py."""
    O, levels = oracle, 4
    case = convergence_case(O)
    base, cond, x0 = case[0], case[1], case[7]
    want = residual_history_cheb(O, case)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), levels)
    g.set_smoother("chebyshev")
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
    print(f"device {rs[0]:.6e} ... {rs[13]:.6e}, statement {want[0]:.6e} ... {want[13]:.6e}, factor {f:.4f}, "
          f"largest relative difference {np.abs(rs / want - 1).max():.2e}")
    assert np.abs(rs / want - 1).max() <= 1e-6
    assert f <= CONVERGENCE_PIN


@pytest.mark.parametrize("dim,n,levels", [(3, 2, 4), (2, 4, 5)])
def test_fcg_around_the_chebyshev_vcycle(oracle, ctx, dim, n, levels):
    """hmg_fcg_* on a grid with smoother 2 against fcg_local with the Chebyshev statement as its V-cycle; a step after
    hmg_grid_set_smoother_chebyshev without a new start is the stale-state error."""
    O, lam, steps = oracle, 1.0, 3
    p = Problem(O, O.hypercube(dim, n), levels, lam, 40 + dim, values=(1.0, 100.0))
    states = [O.LevelState.create(p.mesh.nelements(), p.impl.nf(i + 1)) for i in range(levels)]
    x0 = p.state(levels).x
    b = np.asfortranarray(p.rng.standard_normal(x0.shape))
    g, A = p.device(ctx, kind="chebyshev")
    sts = [hmg.LevelState(g, i + 1) for i in range(levels)]
    x, bd = hmg.DeviceMatrix(g, levels).from_host(x0), hmg.DeviceMatrix(g, levels).from_host(b)
    f = hmg.FlexibleCG(g, hmg.BaseLevel(g), [A] * levels, sts, levels, steps)
    f.start(x, bd)
    r0 = np.abs(f.vec("R")).max()
    his = [None] + [_hi(p, l) for l in range(2, levels + 1)]
    loc = fcg_local(ChebOracle(O, p.dinvs(), his), p.impl, O.make_base_level(p.mesh, p.sig, lam), p.ops(), states, levels, steps, x0, b)
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
    g.set_smoother("chebyshev", ratio=16.0)
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        f.step()
    f.start(x, bd)
    f.step()
    f.close()
    g.close()


def test_lifetimes(oracle, ctx):
    """The inverse diagonals are reserved and released as kind 1 reserves them; kind 0 after kind 2 gives the bits of a grid that
    never saw it, kind 1 after kind 2 the bits of kind 1."""
    O, levels = oracle, 3
    p = Problem(O, _cube(O, 3, 6), levels, 0.5, 5)
    bytes0 = ctx.counter("smoother_diag_bytes")
    g, A = p.device(ctx, kind="cg")
    never = _run_vcycles(ctx, g, A, levels, 2)
    with pytest.raises(HmgError, match="hmg_grid_set_smoother_chebyshev"):
        hmg.smoother_bounds(g, 2)
    g.set_smoother("jacobi")
    jac = _run_vcycles(ctx, g, A, levels, 2)
    g.set_smoother("cg")
    assert ctx.counter("smoother_diag_bytes") == bytes0
    g.set_smoother("chebyshev")
    assert g.smoother() == "chebyshev"
    assert ctx.counter("smoother_diag_bytes") - bytes0 == 8 * sum(g.ld(l) * g.ncells() for l in range(2, levels + 1))
    builds0 = ctx.counter("smoother_bound_builds")
    cheb = _run_vcycles(ctx, g, A, levels, 2)
    assert ctx.counter("smoother_bound_builds") == builds0 + levels - 1 and cheb[2] == 0
    assert not np.array_equal(cheb[0], never[0]) and not np.array_equal(cheb[0], jac[0])
    d2 = hmg.smoother_diag(g, 2).to_host()                                        # hmg_grid_smoother_diag serves kind 2
    np.testing.assert_array_equal(d2 == 0.0, p.dinv(2) == 0.0)
    assert relerr(d2, p.dinv(2)) <= 1e-11
    g.set_smoother("jacobi")
    assert g.smoother() == "jacobi"
    assert ctx.counter("smoother_diag_bytes") - bytes0 == 8 * sum(g.ld(l) * g.ncells() for l in range(2, levels + 1))
    back1 = _run_vcycles(ctx, g, A, levels, 2)
    g.set_smoother("chebyshev")
    g.set_smoother("cg")
    assert ctx.counter("smoother_diag_bytes") == bytes0 and g.smoother() == "cg"
    back0 = _run_vcycles(ctx, g, A, levels, 2)
    g.close()
    for got, want in ((back0, never), (back1, jac)):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_refusals(ctx):
    base = driver.hypercube(hmg.Tet64, 2)
    host = hmg.ImplicitFineGrid(None, base, 3)
    with pytest.raises(HmgError, match="device context"):
        host.set_smoother("chebyshev")
    host.close()
    g = hmg.ImplicitFineGrid(ctx, base, 3)
    for ratio in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(HmgError, match="ratio"):
            g.set_smoother("chebyshev", ratio=ratio)
    with pytest.raises(ValueError):
        g.set_smoother("chebyshev", lambda_hi=[2.0, 2.0])
    with pytest.raises(ValueError):
        g.set_smoother("jacobi", ratio=30.0)
    assert g.smoother() == "cg"
    g.set_smoother("chebyshev", ratio=-1.0)                                      # <= 0: the default
    for level in (0, 1, 4):
        with pytest.raises(HmgError, match="level"):
            hmg.smoother_bounds(g, level)
    g.close()


def test_partitioned_grid_needs_and_takes_explicit_bounds(ctx):
    """The synthetic-cut problem of tests/test_gpu_pcg_smoother_dist.py (w = 4, L = 4, one rank): without bounds the grid is refused
    and nothing changes; with the unpartitioned grid's bounds x after two V-cycles equals the unpartitioned grid's bit for bit --
    no reduction enters, dinv and the interface sums are bit-identical there."""
    from homogenization_jl_amd import dist as hdist
    w, L = 4, 4
    prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, values=(1.0, 100.0), backend="rccl", synthetic_cut=True)
    g, cols = prob.implicit, prob.implicit.local_cells
    bytes0 = ctx.counter("smoother_diag_bytes")
    with pytest.raises(HmgError, match="partitioned"):
        g.set_smoother("chebyshev")
    with pytest.raises(HmgError, match="partitioned"):
        g.set_smoother("chebyshev", lambda_hi=[0.0, 3.0, 3.0, 0.0])
    assert g.smoother() == "cg" and ctx.counter("smoother_diag_bytes") == bytes0
    g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
    g1.set_smoother("chebyshev")
    op1 = hmg.L2PlusDivAGrad(g1, 1.0, prob.cond)
    his = [0.0] + [hmg.smoother_bounds(g1, lev)[1] for lev in range(2, L + 1)]
    n0 = ctx.counter("smoother_bound_builds")
    g.set_smoother("chebyshev", lambda_hi=his)
    assert [hmg.smoother_bounds(g, lev)[1] for lev in range(2, L + 1)] == his[1:]
    assert ctx.counter("smoother_bound_builds") == n0
    rng = np.random.default_rng(5)
    nf, ne = g1.nf(L), g1.ncells()
    x0 = np.asfortranarray(rng.random((nf, ne)))
    b0 = np.asfortranarray(rng.standard_normal((nf, ne)))
    out = []
    for gg, op, bl, cc in ((g, prob.op, prob.base_level(), cols), (g1, op1, hmg.BaseLevel(g1), slice(None))):
        sts = [hmg.LevelState(gg, i + 1) for i in range(L)]
        sts[-1].x.from_host(np.asfortranarray(x0[:, cc]))
        sts[-1].b.from_host(np.asfortranarray(b0[:, cc]))
        hmg.broadcast_interfaces(sts[-1].x, gg, L)
        hmg.apply_constraint(sts[-1].x, L, gg)
        for _ in range(2):
            hmg.vcycle(gg, bl, [op] * L, sts, L, 3)
        out.append(sts[-1].x.to_host())
        for s in sts:
            s.close()
    assert ctx.counter("smoother_bound_builds") == n0
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    np.testing.assert_array_equal(out[0], out[1][:, cols])
    g1.close()


@pytest.mark.parametrize("dim,refinements", [(2, 3), (3, 1), (3, 2)])
def test_driver_converges_to_the_direct_fem_answer(oracle, ctx, dim, refinements):
    """The cases of test_driver_converges_to_the_direct_fem_answer (n = 0, tolerance 1e-12, field and xi from default_rng(8)) with
    smoother="chebyshev": the sparse direct solve's number to 1e-8."""
    from _textbook_fem import converged_first_term
    rng = np.random.default_rng(8)
    sgrid = np.where(rng.random((10,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    xi = rng.standard_normal(dim)
    xi /= np.linalg.norm(xi)
    el = hmg.Tet64 if dim == 3 else hmg.Tri64
    tm = {}
    sigma, hist = driver.checkerboard_homogenization(0, el, refinements=refinements, tolerance=1e-12, xi=xi, sigma_grid=sgrid, ctx=ctx,
                                                     max_cycles=120, smoother="chebyshev", timings=tm)
    want = converged_first_term(oracle, dim, sgrid, xi, refinements)
    print(f"{len(hist)} cycles, sigma - want = {sigma - want:.3e}")
    assert tm["smoother"] == "chebyshev"
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
    plain, hist_p = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="cg", **kw)
    sigma, hist = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="chebyshev", **kw)
    both, hist_b = driver.checkerboard_homogenization(n, hmg.Tet64, smoother="chebyshev", accelerate=True, **kw)
    print(f"chebyshev {len(hist)} cycles (sigma {sigma:.8f}), cg {len(hist_p)} cycles (sigma {plain:.8f}), "
          f"chebyshev + accelerate {len(hist_b)} (sigma {both:.8f})")
    assert len(hist) < len(hist_p), (len(hist), len(hist_p))
    assert abs(sigma - plain) <= 1e-3 * abs(plain)
    assert abs(both - plain) <= 1e-3 * abs(plain)


def test_tensor_driver_with_the_keyword(ctx):
    """driver.checkerboard_homogenization_tensor(smoother="chebyshev") against its "cg" run: every entry to 1e-3 of the largest."""
    kw = dict(refinements=2, tolerance=1e-5, ctx=ctx, seed=3, values=(1.0, 100.0))
    tm = {}
    S_cg, h_cg = driver.checkerboard_homogenization_tensor(0, hmg.Tet64, smoother="cg", **kw)
    S_c, h_c = driver.checkerboard_homogenization_tensor(0, hmg.Tet64, smoother="chebyshev", timings=tm, **kw)
    print(f"cg {len(h_cg)} cycles, chebyshev {len(h_c)} cycles, largest difference {np.abs(S_c - S_cg).max():.3e}")
    assert tm["smoother"] == "chebyshev"
    assert np.abs(S_c - S_cg).max() <= 1e-3 * np.abs(S_cg).max()
