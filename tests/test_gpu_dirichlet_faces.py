"""
hmg_grid_set_dirichlet_faces on the device.  The call adds no kernel: the constraint has always been a per-cell entity bitmask
that every apply family fuses into its epilogue.  What no kernel had seen before is a mask on a face BETWEEN two cells, so every
case here constrains one: the kernel families level by level against the oracle under the same constraint
(tests/_dirichlet_faces_form.py builds it from the oracle's own helpers), both smoothers, V-cycles, the flexible CG, the exact
savings one by one, the way back to the default set, what the call does to cached state, and the drivers built on it.
Tolerances are those of tests/test_gpu_parity.py and tests/test_gpu_pcg_smoother.py: primitives 1e-11, smoothers 1e-10, V-cycles
x 1e-9 / r 1e-8, drivers 1e-8.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

from _dirichlet_faces_form import (FaceSetForm, block_boundary_faces, default_faces, interior_faces, mid_plane_and_sides,  # noqa: F401
                                   one_based, oracle_base_level, oracle_constraint, plane_faces, sides)
from _fcg_form import fcg_global

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
    """One mesh with a constrained face set, on the oracle and on the device."""

    def __init__(self, O, ctx, mesh, levels, faces, lam=0.7, seed=0, perturb=0.0, fused=1, smoother="cg", classes=0, values=(1.0, 9.0)):
        self.O, self.mesh, self.levels, self.lam, self.faces = O, mesh, levels, lam, faces
        self.rng = np.random.default_rng(seed)
        if perturb:                                                      # (the faces were chosen on the lattice)
            mesh.nodes = mesh.nodes + perturb * (self.rng.random(mesh.nodes.shape) - 0.5)
        self.sig = self.rng.choice(list(values), size=(mesh.nelements(), mesh.dim))
        self.impl = O.ImplicitFineGrid.create(mesh, levels)
        self.cons = oracle_constraint(O, mesh, faces)
        self._ops = {}
        ctx.set_option("fuse_cg", fused)                                 # (read when a grid is created)
        ctx.set_option("weight_cache_classes", classes)                  # (read where the operator is set)
        try:
            self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(mesh.nodes, mesh.elements + 1), levels)
            self.g.set_smoother(smoother)
            self.A = hmg.L2PlusDivAGrad(self.g, lam, self.sig)
        finally:
            ctx.set_option("fuse_cg", 1)
            ctx.set_option("weight_cache_classes", 0)
        self.g.set_dirichlet_faces(one_based(faces))

    def op(self, lev):
        if lev not in self._ops:
            O, l = self.O, self.impl.reference.levels[lev - 1]
            self._ops[lev] = O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), self.cons, self.lam, self.sig)
        return self._ops[lev]

    def ops(self):
        return [self.op(l) for l in range(1, self.levels + 1)]

    def base_level(self):
        return oracle_base_level(self.O, self.mesh, self.sig, self.lam, self.faces)

    def rand(self, lev):
        return np.asfortranarray(self.rng.standard_normal((self.impl.nf(lev), self.mesh.nelements())))

    def state(self, lev):
        O = self.O
        st = O.LevelState.create(self.mesh.nelements(), self.impl.nf(lev))
        st.x[...] = self.rand(lev)
        O.broadcast_interfaces(st.x, self.impl, lev)
        O.apply_constraint(st.x, lev, self.cons, self.impl)
        st.b[...] = self.rand(lev)
        return st

    def dev(self, lev, a):
        return hmg.DeviceMatrix(self.g, lev).from_host(a)

    def close(self):
        self.g.close()


def check_primitives(c, levels_checked):
    """hmg_constraint (the same zeros), hmg_apply_ex with the constraint and hmg_residual against the oracle"""
    O = c.O
    between = {tuple(f) for f in interior_faces(c.mesh.elements)}
    assert any(tuple(f) in between for f in c.faces), "the case constrains no face between two cells"
    for lev in levels_checked:
        a = c.rand(lev)
        want = a.copy(order="F")
        O.apply_constraint(want, lev, c.cons, c.impl)
        d = c.dev(lev, a)
        hmg.apply_constraint(d, lev, c.g)
        np.testing.assert_array_equal(d.to_host(), want)
        assert (want == 0.0).any() and (want != 0.0).any()
        x, src = c.rand(lev), c.rand(lev)
        want = src.copy(order="F")
        O.mul(-1.3, c.mesh, c.op(lev), x, want)
        O.apply_constraint(want, lev, c.cons, c.impl)
        out = hmg.DeviceMatrix(c.g, lev)
        hmg.apply_ex(-1.3, c.g, c.dev(lev, x), c.dev(lev, src), out, constrain=True)
        got = out.to_host()
        e_apply = relerr(got, want)
        np.testing.assert_array_equal(got == 0.0, want == 0.0)
        st = O.LevelState.create(c.mesh.nelements(), c.impl.nf(lev))
        st.x[...] = x
        st.b[...] = src
        O.local_residual(c.impl, c.op(lev), st, lev)
        dst = hmg.LevelState(c.g, lev)
        dst.x.from_host(x)
        dst.b.from_host(src)
        hmg.local_residual(c.g, c.A, dst, lev)
        got = dst.r.to_host()
        e_res = relerr(got, st.r)
        print(f"level {lev}: apply_ex {e_apply:.2e}  residual {e_res:.2e}")
        assert e_apply <= TOL and e_res <= TOL, (lev, e_apply, e_res)
        np.testing.assert_array_equal(got == 0.0, st.r == 0.0)
        for v in (d, out):
            v.close()
        dst.close()


@pytest.fixture(scope="module")
def cubes(oracle, ctx):
    """2 x 2 x 2 cubes, six levels, the cells perturbed"""
    m = oracle.hypercube(3, 2)
    c = Case(oracle, ctx, m, 6, mid_plane_and_sides(m), seed=1, perturb=0.2)
    yield c
    c.close()


def test_3d_levels_2_to_6(ctx, cubes):
    """k_apply_small / _pack (levels 2 to 4), k_apply_wave (5), k_apply with the class-weight cache (6)"""
    n0 = {n: ctx.counter(n) for n in ("small_launches", "wave_launches", "weight_cache_launches")}
    check_primitives(cubes, [2, 3, 4, 5, 6])
    assert all(ctx.counter(n) > v for n, v in n0.items()), n0


def test_3d_level_6_without_the_weight_cache(oracle, ctx):
    """option "weight_cache_classes" = 1: more coefficient rows than the cache may hold, the instantiations that form their
    weights per cell"""
    m = oracle.hypercube(3, 2)
    c = Case(oracle, ctx, m, 6, mid_plane_and_sides(m), seed=2, perturb=0.2, classes=1)
    assert c.g.table_i32("cell_class").size == 0
    n0 = ctx.counter("weight_cache_launches")
    check_primitives(c, [5, 6])
    assert ctx.counter("weight_cache_launches") == n0
    c.close()


def test_3d_level_7_faces_between_the_tetrahedra_of_one_cube(oracle, ctx):
    """k_apply_slab2: six cells larger than the LDS, constrained on the six faces they share -- and on none of the outer ones"""
    m = oracle.hypercube(3, 1)
    c = Case(oracle, ctx, m, 7, interior_faces(m.elements), lam=0.9, seed=13, perturb=0.1)
    n0 = ctx.counter("slab2_launches")
    check_primitives(c, [7])
    assert ctx.counter("slab2_launches") > n0
    c.close()


@pytest.mark.parametrize("levels,counter", [(5, None), (9, "rows_launches")])
def test_2d_levels_5_and_9(oracle, ctx, levels, counter):
    """2 x 2 squares: the lattice image (level 5) and k_apply_rows (level 9, cells larger than the LDS)"""
    m = oracle.hypercube(2, 2)
    c = Case(oracle, ctx, m, levels, mid_plane_and_sides(m), seed=9, perturb=0.2)
    n0 = ctx.counter(counter) if counter else 0
    check_primitives(c, [levels])
    assert counter is None or ctx.counter(counter) > n0
    c.close()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("smoother", ["cg", "jacobi", "chebyshev"])
@pytest.mark.parametrize("dim", [3, 2])
def test_smoothing_steps(oracle, ctx, dim, smoother, fused):
    """hmg_smooth, three steps on every level of a small grid, the three smoothers, with and without the fused CG pass: x, r, p to
    1e-10.  The Jacobi smoother's inverse diagonal is 0 on the constrained nodes, the internal plane's among them; the Chebyshev
    smoother's bound (1e-11) and steps are the statement's under the case's constraint."""
    from _cheb_smoother_form import DEFAULT_RATIO, lambda_hi_local, smoothing_steps_cheb
    from _pcg_smoother_form import inverse_diagonal, smoothing_steps_jacobi
    O = oracle
    m = O.hypercube(dim, 2)
    levels = 5 if dim == 3 else 6
    c = Case(O, ctx, m, levels, mid_plane_and_sides(m), seed=17 + dim, perturb=0.2, fused=fused, smoother=smoother)
    for lev in range(2, levels + 1):
        st = c.state(lev)
        dst = hmg.LevelState(c.g, lev)
        dst.x.from_host(st.x)
        dst.b.from_host(st.b)
        if smoother != "cg":
            dinv = inverse_diagonal(O, c.impl, c.op(lev), lev)
            got = hmg.smoother_diag(c.g, lev).to_host()
            assert relerr(got, dinv) <= TOL
            np.testing.assert_array_equal(got == 0.0, dinv == 0.0)
        if smoother == "jacobi":
            smoothing_steps_jacobi(O, 3, c.impl, c.op(lev), st, lev, dinv)
        elif smoother == "chebyshev":
            hi = lambda_hi_local(O, c.impl, c.op(lev), lev, dinv)
            got = hmg.smoother_bounds(c.g, lev)[1]
            assert abs(got - hi) <= TOL * hi, (lev, got, hi)
            smoothing_steps_cheb(O, 3, c.impl, c.op(lev), st, lev, dinv, hi / DEFAULT_RATIO, hi)
        else:
            O.smoothing_steps(3, c.impl, c.op(lev), st, lev)
        hmg.smoothing_steps(3, c.g, c.A, dst, lev)
        ex, er, ep = relerr(dst.x.to_host(), st.x), relerr(dst.r.to_host(), st.r), relerr(dst.p.to_host(), st.p)
        print(f"level {lev}, {smoother}, fuse_cg {fused}: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
        assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (lev, ex, er, ep)
        dst.close()
    c.close()


@pytest.mark.parametrize("dim,n,levels,which", [(3, 2, 4, "mid"), (3, 2, 6, "mid"), (2, 4, 5, "blocks")])
def test_vcycle_matches_oracle(oracle, ctx, dim, n, levels, which):
    """Three hmg_vcycle's, the level-1 system on the set's free nodes: x 1e-9, r and its first-copy norm 1e-8 against the oracle's
    vcycle! under the same constraint."""
    O = oracle
    m = O.hypercube(dim, n)
    faces = mid_plane_and_sides(m) if which == "mid" else block_boundary_faces(m.nodes, m.elements, 2)
    c = Case(O, ctx, m, levels, faces, lam=1.0, seed=11)
    sts = [O.LevelState.create(m.nelements(), c.impl.nf(i + 1)) for i in range(levels)]
    sts[-1] = c.state(levels)
    dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
    dsts[-1].x.from_host(sts[-1].x)
    dsts[-1].b.from_host(sts[-1].b)
    base, dbase = c.base_level(), hmg.BaseLevel(c.g)
    np.testing.assert_array_equal(c.g.interior_nodes(), base.interior_nodes)
    norms = []
    for cyc in range(3):
        O.vcycle(c.impl, base, c.ops(), sts, levels, 3)
        hmg.vcycle(c.g, dbase, [c.A] * levels, dsts, levels, 3)
        ex, er = relerr(dsts[-1].x.to_host(), sts[-1].x), relerr(dsts[-1].r.to_host(), sts[-1].r)
        print(f"cycle {cyc + 1}: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-9 and er <= 1e-8, (cyc, ex, er)
        r = sts[-1].r.copy(order="F")
        O.zero_out_all_but_one(r, c.impl, levels)
        norms.append((np.linalg.norm(r), hmg.norm_unique(dsts[-1].r)))
    for a, b in norms:
        assert abs(a - b) <= 1e-8 * a
    assert norms[-1][0] < norms[0][0]                                    # (the oracle's cycles reduce the residual: a live case)
    for s in dsts:
        s.close()
    c.close()


def test_fcg_matches_the_global_form(oracle, ctx):
    """hmg_fcg_* under a constraint on an internal plane against tests/_fcg_form.py's fcg_global on the global form whose constrained
    nodes come from the set by geometry: x 1e-9, R 1e-8, alpha and beta 1e-8.  The call between two steps asks for a new start."""
    O, dim, n, grids, lam, steps = oracle, 3, 2, 4, 1.0, 3
    rng = np.random.default_rng(23)
    base = O.hypercube(dim, n)
    faces = mid_plane_and_sides(base)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    cond = O.conductivity_per_element(base, sgrid, (0.0,) * dim)
    implicit = O.ImplicitFineGrid.create(base, grids)
    G = FaceSetForm(O, base, sgrid, lam, implicit, grids, dim, faces)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids)
    A = hmg.L2PlusDivAGrad(g, lam, cond)
    g.set_dirichlet_faces(one_based(faces))
    sts = [hmg.LevelState(g, i + 1) for i in range(grids)]
    x = hmg.DeviceMatrix(g, grids).rand(5)
    hmg.broadcast_interfaces(x, g, grids)
    hmg.apply_constraint(x, grids, g)
    b = hmg.DeviceMatrix(g, grids)
    hmg.local_rhs(b, g)
    gx, gb = G.gather(x.to_host(), grids - 1), G.gather_sum(b.to_host(), grids - 1)
    r0 = np.abs(np.where(G.inner[-1], gb - G.A[-1] @ gx, 0.0)).max()
    f = hmg.FlexibleCG(g, hmg.BaseLevel(g), [A] * grids, sts, grids, steps)
    f.start(x, b)
    want = fcg_global(G, grids - 1, gx, gb, steps)
    for it in range(3):
        wx, wR, wp, wa, wb = next(want)
        f.step()
        alpha, beta, pq, pr = f.scalars()
        ex = np.abs(G.gather(x.to_host(), grids - 1) - wx).max() / np.abs(wx).max()
        eR = np.abs(G.gather_sum(f.vec("R"), grids - 1) - wR).max() / r0
        print(f"step {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.12g} / {wa:.12g}  beta {beta:.12g} / {wb:.12g}")
        assert ex <= 1e-9 and eR <= 1e-8, (it, ex, eR)
        assert abs(alpha - wa) <= 1e-8 * abs(wa) and abs(beta - wb) <= 1e-8 * abs(wb), (it, alpha, wa, beta, wb)
    g.set_dirichlet_faces(one_based(faces))                              # (even the same set: a new operator epoch)
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        f.step()
    f.start(x, b)
    f.step()
    f.close()
    g.close()


def _vcycles(ctx, g, op, levels, cycles=3):
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(3)
    st[-1].b.rand(4)
    hmg.broadcast_interfaces(st[-1].x, g, levels)
    hmg.apply_constraint(st[-1].x, levels, g)
    bl = hmg.BaseLevel(g)
    allocs = ctx.counter("device_allocs")
    for _ in range(cycles):
        hmg.vcycle(g, bl, [op] * levels, st, levels, 3)
    assert ctx.counter("device_allocs") == allocs
    out = st[-1].x.to_host(), st[-1].r.to_host()
    for s in st:
        s.close()
    return out


def _mid_plane(base):
    x = base.nodes[:, 0]
    return driver.faces_on_plane(base, 0, 0.5 * (x.min() + x.max()))


@pytest.mark.parametrize("dim,n,levels", [(3, 2, 6), (2, 4, 5)])
def test_exact_savings_are_exact_one_by_one(ctx, dim, n, levels):
    """The pattern of test_gpu_parity.py::test_exact_savings_are_exact on a grid whose set is an internal plane: every exact saving
    of hmg_vcycle switched off by itself, then all of them, then lazy_top = 1 -- x and r after three V-cycles are the bits of the
    run with everything on."""
    tag = hmg.Tet64 if dim == 3 else hmg.Tri64
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, n, levels, seed=11)
    faces = _mid_plane(base)
    assert faces.shape[0] > 0
    g.set_dirichlet_faces(faces)
    try:
        ref = _vcycles(ctx, g, op, levels)
        assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0
        for off in [(o,) for o in EXACT_OPTIONS] + [EXACT_OPTIONS, ("lazy_top=1",)]:
            for o in off:
                ctx.set_option("lazy_top", 1) if o == "lazy_top=1" else ctx.set_option(o, 0)
            try:
                other = _vcycles(ctx, g, op, levels)
            finally:
                for o in EXACT_OPTIONS:
                    ctx.set_option(o, 1)
                ctx.set_option("lazy_top", 2)
            np.testing.assert_array_equal(ref[0], other[0], err_msg=str(off))
            np.testing.assert_array_equal(ref[1], other[1], err_msg=str(off))
    finally:
        g.close()


@pytest.mark.parametrize("smoother", ["cg", "jacobi", "chebyshev"])
def test_back_to_the_default_set_gives_the_bits_of_a_grid_that_never_left_it(ctx, smoother):
    """set(custom), a V-cycle, set(-1), coarse_setup, V-cycles: x and r of a grid that never saw the call, bit for bit; the device
    masks live where they lived ("device_allocs" constant across the setter) and the tables are the default ones again."""
    levels = 5
    res = []
    for visit in (False, True):
        base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, levels, seed=12)
        g.set_smoother(smoother)
        if visit:
            before = g.table_i32("dmask").copy()
            warm = [hmg.LevelState(g, i + 1) for i in range(levels)]
            allocs = ctx.counter("device_allocs")
            g.set_dirichlet_faces(_mid_plane(base))
            assert ctx.counter("device_allocs") == allocs
            assert not np.array_equal(g.table_i32("dmask"), before)
            warm[-1].b.rand(9)
            hmg.vcycle(g, hmg.BaseLevel(g), [op] * levels, warm, levels, 3)
            allocs = ctx.counter("device_allocs")
            g.set_dirichlet_faces(None)
            assert ctx.counter("device_allocs") == allocs
            np.testing.assert_array_equal(g.table_i32("dmask"), before)
            np.testing.assert_array_equal(g.dirichlet_faces(), hmg.api.boundary_faces(base))
            for s in warm:
                s.close()
        res.append(_vcycles(ctx, g, op, levels))                         # (BaseLevel inside: hmg_coarse_setup)
        g.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_setter_under_a_pending_r_leaves_the_eager_r(ctx):
    """hmg_vcycle leaves its last r-update pending (option lazy_r); the call forms it first, with the masks it was recorded under:
    "r_materialized" + 1, not counted as a read, and r is the eager tail's bit for bit."""
    levels = 5
    out = []
    try:
        for lazy in (0, 1):
            ctx.set_option("lazy_r", lazy)
            base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, levels, seed=17, lam=0.8)
            st = [hmg.LevelState(g, i + 1) for i in range(levels)]
            st[-1].x.rand(3)
            st[-1].b.rand(4)
            hmg.broadcast_interfaces(st[-1].x, g, levels)
            hmg.apply_constraint(st[-1].x, levels, g)
            bl = hmg.BaseLevel(g)
            for _ in range(2):
                hmg.vcycle(g, bl, [op] * levels, st, levels, 3, 2)
            assert ctx.counter("lazy_r_form") == lazy
            formed, by_read = ctx.counter("r_materialized"), ctx.counter("r_materialized_by_read")
            g.set_dirichlet_faces(_mid_plane(base))
            assert ctx.counter("r_materialized") - formed == lazy and ctx.counter("r_materialized_by_read") == by_read
            formed = ctx.counter("r_materialized")
            out.append((st[-1].r.to_host(), st[-1].x.to_host()))
            assert ctx.counter("r_materialized") == formed               # (nothing was left to form)
            for s in st:
                s.close()
            g.close()
    finally:
        ctx.set_option("lazy_r", 1)
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def _laminate(dim, n):
    layers = np.array([1.0, 9.0, 3.0, 0.5][:n])[:, None] * np.array([1.0, 2.0, 0.25][:dim])[None, :]     # sigma_kk per layer
    return layers, np.broadcast_to(layers.reshape((n,) + (1,) * (dim - 1) + (dim,)), (n,) * dim + (dim,)).copy()


@pytest.mark.parametrize("dim,smoother,accelerate", [(2, "cg", False), (3, "jacobi", True), (2, "chebyshev", False),
                                                     (3, "chebyshev", True)])
def test_uniaxial_driver_is_exact_for_a_laminate(ctx, dim, smoother, accelerate):
    """Layers normal to e_1: "tensor" is diag(harmonic mean of sigma_11, arithmetic means of the others), in the energy and in the
    flux form.  Solver-limited: 1e-8, the bound tests/test_gpu_pcg_smoother.py holds its driver to against the direct solve, with
    tolerance 1e-12."""
    n = 4 if dim == 2 else 3
    layers, sgrid = _laminate(dim, n)
    want = np.diag([n / (1.0 / layers[:, 0]).sum()] + [layers[:, k].mean() for k in range(1, dim)])
    out = driver.uniaxial_homogenization_tensor(n, hmg.Tet64 if dim == 3 else hmg.Tri64, 2, ctx=ctx, sigma_grid=sgrid, tolerance=1e-12,
                                                smoother=smoother, accelerate=accelerate)
    print(f"cycles {out['cycles']}, tensor error {np.abs(out['tensor'] - want).max():.3e}, flux error {np.abs(out['tensor_flux'] - want).max():.3e}")
    assert np.abs(out["tensor"] - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(out["tensor_flux"] - want).max() <= 1e-8 * np.abs(want).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_uniaxial_diagonal_is_at_most_the_dirichlet_diagonal(ctx, dim):
    """Fewer constrained faces, a larger space, a lower energy minimum -- on a checkerboard strictly (beyond the 1e-8 of the solves)."""
    tag, n = (hmg.Tet64, 2) if dim == 3 else (hmg.Tri64, 4)
    kw = dict(ctx=ctx, seed=5, tolerance=1e-12)
    uni = driver.uniaxial_homogenization_tensor(n, tag, 2, **kw)
    full = driver.dirichlet_homogenization_tensor(n, tag, 2, **kw)
    du, df = np.diag(uni["tensor"]), np.diag(full["tensor"])
    print(f"uniaxial {du}, all faces {df}")
    assert (du <= df * (1.0 + 1e-8)).all() and (du < df).all()
    assert np.abs(uni["tensor"] - uni["tensor"].T).max() == 0.0


@pytest.mark.parametrize("dim", [2, 3])
def test_block_tensors_equal_the_blocks_run_alone(ctx, dim):
    """block_homogenization_tensor(n = 4, block = 2), one refinement: every block's tensor against dirichlet_homogenization_tensor on
    that block's cubes as a mesh of their own (n = 2, the block's part of sigma_grid).  Both solver-limited: 1e-8 of the largest entry.
    The result is a sigma_grid for the next scale."""
    tag, n, block = (hmg.Tet64 if dim == 3 else hmg.Tri64), 4, 2
    sgrid = driver.generate_conductivity(dim, n, 21)
    out = driver.block_homogenization_tensor(n, block, tag, 1, ctx=ctx, sigma_grid=sgrid, tolerance=1e-12)
    T = out["tensor"]
    assert T.shape == (n // block,) * dim + (dim, dim) and out["tensor_flux"].shape == T.shape
    worst = 0.0
    for idx in np.ndindex(*(n // block,) * dim):
        sub = sgrid[tuple(slice(block * i, block * (i + 1)) for i in idx)]
        alone = driver.dirichlet_homogenization_tensor(block, tag, 1, ctx=ctx, sigma_grid=np.ascontiguousarray(sub), tolerance=1e-12)
        worst = max(worst, np.abs(T[idx] - alone["tensor"]).max() / np.abs(alone["tensor"]).max(),
                    np.abs(out["tensor_flux"][idx] - alone["tensor_flux"]).max() / np.abs(alone["tensor_flux"]).max())
    print(f"{dim}D: largest relative difference over the blocks {worst:.3e}")
    assert worst <= 1e-8
    assert np.array_equal(T, np.swapaxes(T, -1, -2))
    nxt = driver.dirichlet_homogenization_tensor(n // block, tag, 1, ctx=ctx, sigma_grid=T, tolerance=1e-8)   # the next scale takes it
    assert np.isfinite(nxt["tensor"]).all() and (np.linalg.eigvalsh(nxt["tensor"]) > 0).all()
    with pytest.raises(ValueError, match="block must divide"):
        driver.block_homogenization_tensor(n, 3, tag, 1, ctx=ctx)


def test_the_empty_set_without_a_mass_term_is_refused(ctx):
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tri64, 2, 3, seed=1, lam=0.0)
    g.set_dirichlet_faces(np.zeros((0, 2), dtype=np.int64))
    with pytest.raises(HmgError, match="no node is constrained.*lambda = 0"):
        hmg.BaseLevel(g)
    op.lam = 0.5
    hmg.BaseLevel(g)                                                     # (with a mass term the level-1 matrix is regular)
    op.lam = 0.0
    st = [hmg.LevelState(g, i + 1) for i in range(3)]
    st[-1].b.rand(4)
    g.set_dirichlet_faces(None)
    hmg.vcycle(g, hmg.BaseLevel(g), [op] * 3, st, 3, 3)
    assert np.isfinite(hmg.norm_unique(st[-1].r))
    for s in st:
        s.close()
    g.close()
