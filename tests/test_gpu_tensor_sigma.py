"""GPU tests of full symmetric conductivity tensors per cell (hmg_grid_set_operator_tensor) through every kernel family, against the
CPU statement of tests/_tensor_sigma_form.py (pinned to the real oracle by tests/test_tensor_sigma_statement.py) and, for a
uniformly rotated tensor, against the real oracle on the rotated mesh.  Smallest shapes that reach each family: 3D 48 cells on
levels 2 (packed), 3-4 (pipelined one-wave), 5 (one wave per cell), 6 (register-blocked) and six cells on level 7 (slab); 2D 32
cells on levels 2-5 and two cells on level 9 (row bands).  Bounds: 1e-11 per primitive (tests/test_gpu_parity.py), 1e-9 / 1e-8
on x / r after V-cycles."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def device(ctx, prob, smoother="cg"):
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(prob.base.nodes, prob.base.elements + 1), prob.grids)
    g.set_smoother(smoother)
    return g, hmg.L2PlusDivAGrad(g, prob.lam, prob.sig)


def check_apply(prob, g, A, level, rng):
    O = prob.O
    x, y = prob.rand(rng, level), prob.rand(rng, level)
    dx = hmg.DeviceMatrix(g, level).from_host(x)
    for alpha in (1.0, -1.0):
        dy = hmg.DeviceMatrix(g, level).from_host(y)
        hmg.mul(alpha, g, A, dx, dy)
        want = y.copy(order="F")
        T.mul(O, alpha, prob.base, prob.ops[level - 1], x, want)
        err = relerr(dy.to_host(), want)
        print(f"level {level} alpha {alpha:+.0f}: apply {err:.2e}")
        assert err <= TOL, (level, alpha, err)
        dy.close()
    st = O.LevelState.create(prob.base.nelements(), prob.implicit.nf(level))
    st.x[...], st.b[...] = x, y
    T.local_residual(O, prob.implicit, prob.ops[level - 1], st, level)
    dst = hmg.LevelState(g, level)
    dst.x.from_host(x)
    dst.b.from_host(y)
    hmg.local_residual(g, A, dst, level)
    got = dst.r.to_host()
    err = relerr(got, st.r)
    print(f"level {level}: residual {err:.2e}")
    assert err <= TOL, (level, err)
    np.testing.assert_array_equal(got == 0.0, st.r == 0.0)
    dst.close()
    dx.close()


@pytest.fixture(scope="module")
def cube(oracle):
    """hypercube(3, 2): 48 cells, one random SPD tensor (eigenvalues 1 .. 100) per cell, six grids"""
    O = oracle
    base = O.hypercube(3, 2)
    return T.Problem(O, base, 6, 0.7, T.random_spd(np.random.default_rng(31), base.nelements(), 3))


@pytest.fixture(scope="module")
def square(oracle):
    O = oracle
    base = O.hypercube(2, 4)
    return T.Problem(O, base, 5, 0.7, T.random_spd(np.random.default_rng(32), base.nelements(), 2))


def test_apply_and_residual_3d_levels_2_to_6(ctx, cube):
    g, A = device(ctx, cube)
    rng = np.random.default_rng(1)
    n_small, n_wave = ctx.counter("small_launches"), ctx.counter("wave_launches")
    for level in range(2, 7):
        check_apply(cube, g, A, level, rng)
    assert ctx.counter("small_launches") - n_small >= 9 and ctx.counter("wave_launches") - n_wave >= 3
    assert ctx.counter("weight_cache_classes") >= 48
    g.close()


def test_apply_and_residual_level_7(oracle, ctx):
    """n = 1: six cells of 47 905 nodes, larger than the LDS (slab kernel)"""
    O = oracle
    base = O.hypercube(3, 1)
    prob = T.Problem(O, base, 7, 0.9, T.random_spd(np.random.default_rng(33), base.nelements(), 3), top_only=True)
    g, A = device(ctx, prob)
    n0 = ctx.counter("slab2_launches")
    check_apply(prob, g, A, 7, np.random.default_rng(2))
    assert ctx.counter("slab2_launches") > n0
    g.close()


def test_apply_and_residual_2d_levels_2_to_5(ctx, square):
    g, A = device(ctx, square)
    rng = np.random.default_rng(3)
    for level in range(2, 6):
        check_apply(square, g, A, level, rng)
    g.close()


def test_apply_and_residual_2d_level_9(oracle, ctx):
    """two triangles of 33 153 nodes: the row-band kernels"""
    O = oracle
    base = O.hypercube(2, 1)
    prob = T.Problem(O, base, 9, 0.7, T.random_spd(np.random.default_rng(34), base.nelements(), 2), top_only=True)
    g, A = device(ctx, prob)
    n0 = ctx.counter("rows_launches")
    check_apply(prob, g, A, 9, np.random.default_rng(4))
    assert ctx.counter("rows_launches") > n0
    g.close()


@pytest.mark.parametrize("which", ["cube", "square"])
def test_right_hand_side_integrals_and_level_1_solve(request, ctx, which):
    prob = request.getfixturevalue(which)
    O, top, dim = prob.O, prob.grids, prob.base.dim
    g, A = device(ctx, prob)
    rng = np.random.default_rng(5)
    dphis = O.partial_derivatives_functionals(prob.implicit.reference.levels[-1])
    xi = np.array([0.3, -1.0, 0.7])[:dim]
    want_b = np.zeros((prob.implicit.nf(top), prob.base.nelements()), order="F")
    T.rhs_axi_grad_v(O, want_b, dphis, prob.implicit, prob.sig, xi)
    db = hmg.DeviceMatrix(g, top)
    hmg.rhs_axi_grad_v(db, g, xi)
    assert relerr(db.to_host(), want_b) <= TOL
    # ... which is not the right-hand side of the diagonal parts
    diag_b = np.zeros_like(want_b)
    O.rhs_axi_grad_v(diag_b, dphis, prob.implicit, np.ascontiguousarray(np.einsum("eaa->ea", prob.sig)), xi)
    assert relerr(diag_b, want_b) > 1e-3

    v, w = prob.rand(rng, top), prob.rand(rng, top)
    dv, dw = hmg.DeviceMatrix(g, top).from_host(v), hmg.DeviceMatrix(g, top).from_host(w)
    nsub = prob.base.nelements() - 3
    _, _, det = O.cell_geometry(prob.base)
    mass = prob.mass[-1]
    want0 = T.integrate_first_term(O, v, dphis, prob.implicit, nsub, mass, prob.sig, xi)
    assert abs(hmg.integrate_first_term(dv, g, nsub, xi, b=db) - want0) <= TOL * abs(want0)              # mode 0
    assert abs(hmg.integrate_first_term(dv, g, nsub, xi) - want0) <= TOL * abs(want0)
    want3 = float(np.sum(np.einsum("ie,ie->e", w[:, :nsub], mass @ v[:, :nsub]) * det[:nsub]))
    scale3 = float(np.sum(np.einsum("ie,ie->e", abs(w[:, :nsub]), abs(mass) @ abs(v[:, :nsub])) * det[:nsub]))
    assert abs(hmg.integrate_pair_mass(dv, dw, g, nsub) - want3) <= TOL * scale3                         # mode 3
    want4 = float(np.sum(np.einsum("ie,ie->e", v[:, :nsub], want_b[:, :nsub]) * det[:nsub]))
    scale4 = float(np.sum(np.einsum("ie,ie->e", abs(v[:, :nsub]), abs(want_b[:, :nsub])) * det[:nsub]))
    assert abs(hmg.integrate_pair_load(dv, db, g, nsub) - want4) <= TOL * scale4                         # mode 4

    # level 1: hmg_coarse_solve against a direct solve of the textbook matrix
    b1 = prob.rand(rng, 1)
    st = [O.LevelState.create(prob.base.nelements(), prob.implicit.nf(1))]
    st[0].b[...] = b1
    O.vcycle(prob.implicit, prob.base_level, prob.ops, st, 1)
    d1 = hmg.LevelState(g, 1)
    d1.b.from_host(b1)
    hmg.BaseLevel(g)
    L = hmg._lib
    L.check(L.load().hmg_coarse_solve(g.h, d1.b.h, d1.x.h))
    err = relerr(d1.x.to_host(), st[0].x)
    print("level-1 solve", err)
    assert err <= 1e-10
    g.close()


@pytest.mark.parametrize("smoother", ["cg", "jacobi", "chebyshev"])
@pytest.mark.parametrize("which", ["cube", "square"])
def test_vcycles(request, ctx, which, smoother):
    """three smoothing steps, two V-cycles: x 1e-9, r 1e-8; "jacobi" and "chebyshev": the inverse diagonal first, 1e-11;
    "chebyshev": the bound of every level 1e-11, the cycles those of tests/_cheb_smoother_form.py over the tensor operator"""
    import _cheb_smoother_form as C
    prob = request.getfixturevalue(which)
    O, top = prob.O, prob.grids
    g, A = device(ctx, prob, smoother)
    dinvs = his = None
    if smoother != "cg":
        dinvs = prob.dinvs()
        for level in range(2, top + 1):
            got = hmg.smoother_diag(g, level).to_host()
            err = relerr(got, dinvs[level - 1])
            print(f"level {level}: inverse diagonal {err:.2e}")
            assert err <= 1e-11, (level, err)
            np.testing.assert_array_equal(got == 0.0, dinvs[level - 1] == 0.0)
    if smoother == "chebyshev":
        his = C.bounds_local(O, prob.implicit, prob.ops, top, dinvs)
        for level in range(2, top + 1):
            hi = hmg.smoother_bounds(g, level)[1]
            print(f"level {level}: bound {hi:.12f}, statement {his[level - 1]:.12f}")
            assert abs(hi - his[level - 1]) <= 1e-11 * his[level - 1], (level, hi, his[level - 1])
    rng = np.random.default_rng(6)
    x0, b0 = prob.rand(rng, top), prob.rand(rng, top)
    prob.start(x0, b0)
    dst = [hmg.LevelState(g, i + 1) for i in range(top)]
    dst[-1].x.from_host(prob.states[-1].x)
    dst[-1].b.from_host(b0)
    bl = hmg.BaseLevel(g)
    for cyc in range(2):
        if smoother == "chebyshev":
            C.vcycle_cheb(O, prob.implicit, prob.base_level, prob.ops, prob.states, top, 3, dinvs, his)
        else:
            prob.cycle(3, dinvs if smoother == "jacobi" else None)
        hmg.vcycle(g, bl, [A] * top, dst, top, 3)
        ex, er = relerr(dst[-1].x.to_host(), prob.states[-1].x), relerr(dst[-1].r.to_host(), prob.states[-1].r)
        print(f"{which} {smoother} cycle {cyc + 1}: x {ex:.2e} r {er:.2e}")
        assert ex <= 1e-9 and er <= 1e-8, (cyc, ex, er)
    a0 = ctx.counter("device_allocs")                            # (the downloads above stage through memory of their own)
    hmg.vcycle(g, bl, [A] * top, dst, top, 3)
    ctx.sync()
    assert ctx.counter("device_allocs") == a0                    # a V-cycle allocates nothing
    g.close()


def test_fcg_takes_the_tensor(ctx, cube):
    """hmg_fcg_*: after six steps the residual the method carries along is the true residual of the tensor operator at its
    iterate (1e-8 of the first residual: six updates of rounding size each)"""
    prob = cube
    O, top = prob.O, prob.grids
    g, A = device(ctx, prob)
    rng = np.random.default_rng(7)
    b0 = prob.rand(rng, top)
    dst = [hmg.LevelState(g, i + 1) for i in range(top)]
    dst[-1].b.from_host(b0)
    xv = hmg.DeviceMatrix(g, top)
    fcg = hmg.FlexibleCG(g, hmg.BaseLevel(g), [A] * top, dst, top, 3)
    fcg.start(xv, dst[-1].b)
    r0 = fcg.residual_norm()
    for _ in range(6):
        fcg.step()
    print("flexible CG, six steps: residual", fcg.residual_norm() / r0, "of the first")
    st = O.LevelState.create(prob.base.nelements(), prob.implicit.nf(top))
    st.x[...], st.b[...] = xv.to_host(), b0
    T.local_residual(O, prob.implicit, prob.ops[-1], st, top)
    O.broadcast_interfaces(st.r, prob.implicit, top)
    O.zero_out_all_but_one(st.r, prob.implicit, top)
    assert abs(np.linalg.norm(st.r) - fcg.residual_norm()) <= 1e-8 * r0
    fcg.close()
    g.close()


def test_real_oracle_on_a_uniformly_rotated_mesh(oracle, ctx):
    """Device: sigma = Q D Q^T in every cell, plain mesh.  Oracle: diag D, the mesh x -> Q^T x.  Three V-cycles, five grids."""
    O = oracle
    grids, lam = 5, 0.5
    rng = np.random.default_rng(8)
    base = O.hypercube(3, 2)
    Q = T.random_rotation(rng, 3)
    D = np.array([1.0, 100.0, 9.0])
    S = (Q * D[None, :]) @ Q.T
    sig = np.ascontiguousarray(np.broadcast_to(0.5 * (S + S.T), (base.nelements(), 3, 3)))
    mr = T.rotated_mesh(O, base, Q)
    cond = np.ascontiguousarray(np.broadcast_to(D, (base.nelements(), 3)))
    impl = O.ImplicitFineGrid.create(mr, grids)
    cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(mr))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, lam, cond) for l in impl.reference.levels]
    sts = [O.LevelState.create(mr.nelements(), impl.nf(i + 1)) for i in range(grids)]
    x0 = np.asfortranarray(rng.random(sts[-1].x.shape))
    b0 = np.asfortranarray(rng.random(sts[-1].x.shape) - 0.5)
    sts[-1].x[...] = x0
    O.broadcast_interfaces(sts[-1].x, impl, grids)
    O.apply_constraint(sts[-1].x, grids, cons, impl)
    sts[-1].b[...] = b0
    obase = O.make_base_level(mr, cond, lam)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids)
    A = hmg.L2PlusDivAGrad(g, lam, sig)
    dst = [hmg.LevelState(g, i + 1) for i in range(grids)]
    dst[-1].x.from_host(sts[-1].x)
    dst[-1].b.from_host(b0)
    bl = hmg.BaseLevel(g)
    for cyc in range(3):
        O.vcycle(impl, obase, ops, sts, grids, 3)
        hmg.vcycle(g, bl, [A] * grids, dst, grids, 3)
        ex, er = relerr(dst[-1].x.to_host(), sts[-1].x), relerr(dst[-1].r.to_host(), sts[-1].r)
        print(f"rotated mesh, cycle {cyc + 1}: x {ex:.2e} r {er:.2e}")
        assert ex <= 1e-9 and er <= 1e-8, (cyc, ex, er)
    g.close()


def test_diagonal_field_as_tensors_through_the_2d_driver(ctx):
    """checkerboard_homogenization(2, Tri64, refinements=2): a diagonal field passed as (dim, dim) tensors returns the diagonal
    run's history exactly"""
    from homogenization_jl_amd import driver
    n = 2
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sg = driver.generate_conductivity(2, width, 3)
    st = np.zeros(sg.shape + (2,))
    st[..., 0, 0], st[..., 1, 1] = sg[..., 0], sg[..., 1]
    want, hist = driver.checkerboard_homogenization(n, hmg.Tri64, refinements=2, ctx=ctx, sigma_grid=sg, seed=4)
    got, hist_t = driver.checkerboard_homogenization(n, hmg.Tri64, refinements=2, ctx=ctx, sigma_grid=st, seed=4)
    assert got == want and hist_t == hist and len(hist) > 3


def test_tensor_driver_on_a_polycrystal_matches_polarised_scalar_runs(ctx):
    """checkerboard_homogenization_tensor on driver.generate_polycrystal(2, ...): all three entries against the polarisation of
    three scalar runs (xi = e_1, e_2, (e_1 + e_2) / sqrt 2).  At k = 0 the pair integrals take the load of sigma e_j; with the
    load of sigma_jj e_j the off-diagonal entry is off by the size of sigma_12."""
    from homogenization_jl_amd import driver
    from _tensor_form import polarised
    n = 1
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    grid = driver.generate_polycrystal(2, width, 11, (1.0, 9.0))
    assert grid.shape == (width, width, 2, 2) and (grid == np.swapaxes(grid, -1, -2)).all()
    ev = np.linalg.eigvalsh(grid.reshape(-1, 2, 2))
    assert np.abs(ev - np.array([1.0, 9.0])).max() <= 1e-13 and np.unique(grid[..., 0, 1]).size == width * width
    kw = dict(refinements=2, tolerance=1e-11, ctx=ctx, sigma_grid=grid, seed=4)
    Sigma, hist = driver.checkerboard_homogenization_tensor(n, hmg.Tri64, **kw)
    want = polarised(lambda xi: driver.checkerboard_homogenization(n, hmg.Tri64, xi=xi, **kw)[0], 2)
    print("polycrystal: tensor driver", Sigma.tolist(), "polarised", want.tolist())
    assert np.abs(Sigma - want).max() <= 1e-8
    assert abs(Sigma[0, 1]) > 1e-3


def test_partitioned_grid_takes_per_cell_tensors_bit_for_bit():
    """the synthetic-cut rehearsal grid of tests/test_gpu_dist.py (4^3 cubes, four grids) with one tensor per cell: the
    partitioned grid's stored global field, its local rows and its replicated level-1 matrix; x and r after two V-cycles equal
    the unpartitioned grid's bit for bit"""
    from homogenization_jl_amd import dist as hdist
    w, L = 4, 4
    ctx = hmg.Context(0)
    try:
        prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
        g = prob.implicit
        ctx.set_option("overlap_min_doubles", 1)
        sig = T.random_spd(np.random.default_rng(9), prob.global_base.elements.shape[0], 3)
        opp = hmg.L2PlusDivAGrad(g, 1.0, sig)
        g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
        op1 = hmg.L2PlusDivAGrad(g1, 1.0, sig)
        np.testing.assert_array_equal(g.table_f64("coef"), g1.table_f64("coef").reshape(-1, 8)[g.local_cells].ravel())
        sts_p = [hmg.LevelState(g, i + 1) for i in range(L)]
        sts_s = [hmg.LevelState(g1, i + 1) for i in range(L)]
        for st, gg in ((sts_p, g), (sts_s, g1)):
            st[-1].x.rand(5); st[-1].b.rand(6)
            hmg.broadcast_interfaces(st[-1].x, gg, L)
            hmg.apply_constraint(st[-1].x, L, gg)
        bl_p, bl_s = prob.base_level(), hmg.BaseLevel(g1)
        for _ in range(2):
            hmg.vcycle(g, bl_p, [opp] * L, sts_p, L, 3)
            hmg.vcycle(g1, bl_s, [op1] * L, sts_s, L, 3)
        np.testing.assert_array_equal(sts_p[-1].x.to_host(), sts_s[-1].x.to_host())
        np.testing.assert_array_equal(sts_p[-1].r.to_host(), sts_s[-1].r.to_host())
        # ... and after a domain shrink (the prefix of the global field is cut again)
        from oracle import oracle as O
        m = O.Mesh(prob.global_base.nodes, prob.global_base.elements - 1)
        ne, nn = O.find_elements_in_radius(m, 1), O.find_nodes_in_radius(m, 1)
        g.shrink(ne, nn)
        g1.shrink(ne, nn)
        np.testing.assert_array_equal(g.table_f64("coef"), g1.table_f64("coef").reshape(-1, 8)[g.local_cells].ravel())
    finally:
        ctx.close()
