"""
Grids on a torus on the device (hmg_grid_create_periodic, hmg_grid_set_mean_free, driver.periodic_homogenization_tensor).  No
apply, smoother or interface kernel knows about the torus: the tests hold every apply family, the interface sum, the level-1
solve on the complement of the constants, converged correctors, the exact savings of hmg_vcycle and the driver to statements
that never see the torus connectivity (tests/_periodic_form.py): the cell-local part from the oracle on the cells as disjoint
simplices, the sum over copies from a grouping of the fine nodes by position modulo the period, converged answers from a sparse
direct solve of the textbook system on the explicitly refined disjoint simplices.  The grid, its oracle twin and the check of
the primitives are tests/_periodic_device.py's, shared with tests/test_gpu_periodic_general.py (general tori, full tensors).  Tolerances are the project's: primitives 1e-11,
level-1 solve 1e-10 (tests/test_gpu_coarse_solve.py), converged answers and drivers 1e-8 at tolerance 1e-12.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

import _coarse_form as CF
import _tensor_sigma_form as TS
from _periodic_device import Torus, check_primitives, per_cube, relerr
from _periodic_form import DEN, TorusSystem, fine_ids, general_torus

pytestmark = pytest.mark.gpu

EXACT_OPTIONS = ("lean_post", "lazy_post", "lazy_top", "lazy_dead", "lazy_pre", "fold_x", "swap_rp", "fold_prolong", "prolong_in_image",
                 "fold_faces", "fold_restrict", "fold_coarse_x", "zero_entry", "cell_order", "lazy_r", "lazy_ap", "lazy_x")


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torus3(oracle, ctx):
    c = Torus(oracle, ctx, 3, 6, seed=1)
    yield c
    c.close()


def test_3d_levels_2_to_6(ctx, torus3):
    """k_apply_small / _pack (levels 2 to 4), k_apply_wave (5), k_apply with the class-weight cache (6)"""
    n0 = {n: ctx.counter(n) for n in ("small_launches", "wave_launches", "weight_cache_launches")}
    check_primitives(torus3, [2, 3, 4, 5, 6])
    assert all(ctx.counter(n) > v for n, v in n0.items()), n0


def test_3d_level_6_without_the_weight_cache(oracle, ctx):
    c = Torus(oracle, ctx, 3, 6, seed=2, classes=1)
    assert c.g.table_i32("cell_class").size == 0
    n0 = ctx.counter("weight_cache_launches")
    check_primitives(c, [6])
    assert ctx.counter("weight_cache_launches") == n0
    c.close()


def test_3d_level_7_once(oracle, ctx):
    """k_apply_slab2: 162 cells larger than the LDS, 7.8 M entries"""
    c = Torus(oracle, ctx, 3, 7, seed=3)
    n0 = ctx.counter("slab2_launches")
    check_primitives(c, [7], lams=(0.7,))
    assert ctx.counter("slab2_launches") > n0
    c.close()


@pytest.mark.parametrize("levels,counter", [(5, None), (9, "rows_launches")])
def test_2d_levels_5_and_9(oracle, ctx, levels, counter):
    c = Torus(oracle, ctx, 2, levels, seed=4)
    n0 = ctx.counter(counter) if counter else 0
    check_primitives(c, [levels])
    assert counter is None or ctx.counter(counter) > n0
    c.close()


def test_sampling_refuses_a_torus(ctx):
    """hmg_sample and hmg_sample_raster (and their host twin) refuse a periodic grid before the locator reads a coordinate"""
    from homogenization_jl_amd._lib import HmgError
    for dim in (2, 3):
        g = hmg.ImplicitFineGrid(ctx, driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, 3), 3)
        v = hmg.DeviceMatrix(g, 3).rand(1)
        with pytest.raises(HmgError, match="hmg_sample: periodic"):
            hmg.sample(v, g, np.full((2, dim), 1.25))
        du, dv = np.eye(dim)[0] * 0.5, np.eye(dim)[1] * 0.5
        with pytest.raises(HmgError, match="hmg_sample_raster: periodic"):
            hmg.sample_raster(v, g, np.full(dim, 0.25), du, dv, 4, 4)
        with pytest.raises(HmgError, match="hmg_grid_locate: periodic"):
            hmg.locate(g, 3, np.full((2, dim), 1.25))
        v.close()
        g.close()


# ---- the level-1 solve on the complement of the constants ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 5), (4, 3)], ids=["3x4x5", "4x3"])
@pytest.mark.parametrize("contrast", [9.0, 1e4])
def test_level_1_solve_against_the_pseudo_inverse(ctx, shape, contrast):
    dim = len(shape)
    mesh = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, shape)
    rng = np.random.default_rng(7)
    g = hmg.ImplicitFineGrid(ctx, mesh, 2)
    assert g.mean_free()
    g.set_operator(per_cube(mesh, rng.choice([1.0, contrast], size=tuple(shape) + (dim,))), 0.0)
    g.coarse_setup()
    A, interior = CF.matrix(g)
    nn = mesh.nodes.shape[0]
    w, V = np.linalg.eigh(A.toarray())
    assert abs(w[0]) <= 1e-12 * w[-1] and w[1] > 1e-6 * w[-1] / contrast   # one zero eigenvalue: the constants
    cells = mesh.elements - 1
    lib = hmg._lib
    db, dx = hmg.DeviceMatrix(g, 1), hmg.DeviceMatrix(g, 1)
    for constant in (0.0, 3.0, 0.0, -250.0):
        b1 = np.asfortranarray(rng.standard_normal((dim + 1, cells.shape[0])) + constant)
        u = CF.node_sum(cells, nn, b1)
        want = V[:, 1:] @ ((V[:, 1:].T @ u) / w[1:])
        db.from_host(b1)
        dx.fill(7.0)                                                     # (every entry has to be written)
        allocs = ctx.counter("device_allocs")                            # (around the solve alone: up- and downloads stage)
        lib.check(lib.load().hmg_coarse_solve(g.h, db.h, dx.h))
        ctx.sync()
        assert ctx.counter("device_allocs") == allocs                    # (no solve allocates)
        x1 = dx.to_host()
        xg = CF.gather(cells, nn, x1)
        np.testing.assert_array_equal(CF.distribute(cells, xg), x1)
        err = relerr(xg - xg.mean(), want - want.mean())
        print(f"contrast {contrast:g}, constant {constant:g}: x {err:.2e}  mean {abs(xg.mean()):.2e}  max {np.abs(xg).max():.2e}")
        assert err <= 1e-10, err
        assert abs(xg.mean()) <= 1e-13 * np.abs(xg).max()
    for v in (db, dx):
        v.close()
    g.close()


# ---- converged correctors ------------------------------------------------------------------------------------------------------
def _full_per_cube(dim, mesh):
    """one full SPD tensor per cube: 3D the grains of driver.generate_polycrystal(3, 3, 8), 2D nine of random_spd"""
    sg = driver.generate_polycrystal(3, 3, 8) if dim == 3 else TS.random_spd(np.random.default_rng(8), 9, 2).reshape(3, 3, 2, 2)
    return per_cube(mesh, sg)


def _converged_case(oracle, dim, refinements, general, full):
    """the torus, its medium, and the direct solution of the corrector of e_1"""
    if general:
        mesh, den = general_torus((3,) * dim, 19 + dim), DEN
    else:
        mesh, den = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, 3), 1
    if full:
        cond = _full_per_cube(dim, mesh)
    else:
        cond = per_cube(mesh, np.random.default_rng(21 + dim).choice([1.0, 9.0], size=(3,) * dim + (dim,)))
    sys = TorusSystem(oracle, mesh, cond, refinements, den=den)
    xi = np.eye(dim)[0]
    v = sys.corrector(xi)
    return dim, refinements, mesh, cond, sys, xi, v, sys.energy(v, xi)


@pytest.fixture(scope="module", params=[(2, 2), (3, 1)], ids=["2d", "3d"])
def converged(request, oracle):
    """the unit-cube torus, a random two-valued sigma per cube and direction, and the direct solution of the corrector of e_1"""
    return _converged_case(oracle, *request.param, general=False, full=False)


MEDIA = {"full": (False, True), "general-diagonal": (True, False), "general-full": (True, True)}


@pytest.fixture(scope="module", params=[(d, r, m) for d, r in ((2, 2), (3, 1)) for m in MEDIA],
                ids=lambda p: f"{p[0]}d-{p[2]}")
def converged_media(request, oracle):
    """the other three media of a dimension: a full SPD tensor per cube, and both on a moved and stretched torus"""
    dim, refinements, medium = request.param
    return _converged_case(oracle, dim, refinements, *MEDIA[medium])


def _check_converged(ctx, case, how):
    dim, refinements, mesh, cond, sys, xi, v, sigma11 = case
    levels = refinements + 1
    g = hmg.ImplicitFineGrid(ctx, mesh, levels)
    g.set_smoother("cg" if how == "fcg" else how)
    op = hmg.L2PlusDivAGrad(g, 0.0, cond)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(levels)]
    accelerate = how == "fcg"
    xv = hmg.DeviceMatrix(g, levels) if accelerate else states[-1].x
    fcg = hmg.FlexibleCG(g, bl, [op] * levels, states, levels, 3) if accelerate else None
    cycles, rnorm, r0 = driver._dirichlet_solve(g, op, bl, states, xv, fcg, xi, 3, 1e-12, 200, "test")
    assert rnorm <= 1e-12 * r0, (cycles, rnorm / r0)
    x = xv.to_host()
    ids, n = fine_ids(g, levels, sys.den)
    u = np.zeros(n)
    u[ids.ravel()] = x.ravel()
    np.testing.assert_array_equal(u[ids], x)                             # a consistent level vector
    got = sys.gather(g, levels, x)
    err = np.linalg.norm((got - got.mean()) - v) / np.linalg.norm(v)
    mean, gram = hmg.cell_moments(xv, g, xi)
    entry = float(hmg.fields.energy(cond, gram).sum() / hmg.fields.cell_volumes(mesh).sum())
    print(f"{dim}D, {how}, sigma {cond.shape[1:]}: {cycles} cycles, corrector {err:.2e}, Sigma_11 {entry:.12g} / {sigma11:.12g}")
    assert err <= 1e-8, err
    assert abs(entry - sigma11) <= 1e-8 * abs(sigma11)
    if accelerate:
        fcg.close()
        xv.close()
    for s in states:
        s.close()
    g.close()


@pytest.mark.parametrize("how", ["cg", "jacobi", "chebyshev", "fcg"])
def test_converged_corrector(ctx, converged, how):
    _check_converged(ctx, converged, how)


def test_converged_corrector_on_the_other_media(ctx, converged_media):
    """the CG smoother on full tensors per cube, and on a general torus with either medium"""
    _check_converged(ctx, converged_media, "cg")


# ---- exact savings ---------------------------------------------------------------------------------------------------------------
def _vcycles(ctx, g, op, levels, cycles=3):
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(3)
    st[-1].b.rand(4)
    hmg.broadcast_interfaces(st[-1].x, g, levels)
    bl = hmg.BaseLevel(g)                                                # (hmg_coarse_setup: the level-1 system's memory)
    allocs = ctx.counter("device_allocs")
    for _ in range(cycles):
        hmg.vcycle(g, bl, [op] * levels, st, levels, 3)
    assert ctx.counter("device_allocs") == allocs
    form = ctx.counter("lazy_x_form")
    out = st[-1].x.to_host(), st[-1].r.to_host(), form
    for s in st:
        s.close()
    return out


def test_exact_savings_are_exact_on_a_torus(ctx):
    """3 x 3 x 3 torus, level 6, lambda = 0 (the level-1 solve projects): three V-cycles with every exact saving on give the bits of
    the plain sequence, x and r; and the last one leaves the x-updates pending in the form it does on an ordinary grid"""
    levels = 6
    mesh = driver.periodic_mesh(hmg.Tet64, 3)
    cond = per_cube(mesh, np.random.default_rng(11).choice([1.0, 9.0], size=(3, 3, 3, 3)))
    g = hmg.ImplicitFineGrid(ctx, mesh, levels)
    op = hmg.L2PlusDivAGrad(g, 0.0, cond)
    try:
        ref = _vcycles(ctx, g, op, levels)
        assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0
        for o in EXACT_OPTIONS:
            ctx.set_option(o, 0)
        try:
            plain = _vcycles(ctx, g, op, levels)
        finally:
            for o in EXACT_OPTIONS:
                ctx.set_option(o, 1)
            ctx.set_option("lazy_top", 2)
        np.testing.assert_array_equal(ref[0], plain[0])
        np.testing.assert_array_equal(ref[1], plain[1])
        assert plain[2] == 0
    finally:
        g.close()
    base, bcond, bg, bop = driver.checkerboard_problem(ctx, hmg.Tet64, 2, levels, seed=11)
    try:
        assert _vcycles(ctx, bg, bop, levels)[2] == ref[2] > 0
    finally:
        bg.close()


# ---- driver -----------------------------------------------------------------------------------------------------------------------
def _laminate(dim, n):
    layers = np.array([1.0, 9.0, 3.0, 0.5][:n])[:, None] * np.array([1.0, 2.0, 0.25][:dim])[None, :]     # sigma_kk per layer
    return layers, np.broadcast_to(layers.reshape((n,) + (1,) * (dim - 1) + (dim,)), (n,) * dim + (dim,)).copy()


@pytest.mark.parametrize("dim,smoother,accelerate", [(2, "cg", False), (3, "jacobi", True), (2, "chebyshev", False),
                                                     (3, "chebyshev", True)])
def test_periodic_driver_is_exact_for_a_laminate(ctx, dim, smoother, accelerate):
    """Layers normal to e_1: diag(harmonic mean of sigma_11, arithmetic means of the others), in the energy and the flux form"""
    n = 4 if dim == 2 else 3
    layers, sgrid = _laminate(dim, n)
    want = np.diag([n / (1.0 / layers[:, 0]).sum()] + [layers[:, k].mean() for k in range(1, dim)])
    out = driver.periodic_homogenization_tensor(n, hmg.Tet64 if dim == 3 else hmg.Tri64, 2, ctx=ctx, sigma_grid=sgrid, tolerance=1e-12,
                                                smoother=smoother, accelerate=accelerate)
    print(f"cycles {out['cycles']}, tensor error {np.abs(out['tensor'] - want).max():.3e}, flux error {np.abs(out['tensor_flux'] - want).max():.3e}")
    assert np.abs(out["tensor"] - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(out["tensor_flux"] - want).max() <= 1e-8 * np.abs(want).max()
    assert out["volume"] == float(n ** dim)


def test_2d_tensor_does_not_depend_on_where_the_period_starts(ctx):
    """the refinement of a triangle does not depend on the order of its vertices: the 2D fine mesh is translation invariant"""
    n = 4
    sgrid = driver.generate_conductivity(2, n, 3)
    kw = dict(ctx=ctx, tolerance=1e-12)
    ref = driver.periodic_homogenization_tensor(n, hmg.Tri64, 2, sigma_grid=sgrid, **kw)["tensor"]
    for axis in (0, 1):
        got = driver.periodic_homogenization_tensor(n, hmg.Tri64, 2, sigma_grid=np.roll(sgrid, 1, axis=axis), **kw)["tensor"]
        print(f"shift along axis {axis}: {np.abs(got - ref).max():.3e}")
        assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_periodic_tensor_bounds_and_the_dirichlet_diagonal(ctx, dim):
    """symmetric exactly; between the harmonic and the arithmetic mean (as tensors: Voigt and Reuss); its diagonal at most the
    Dirichlet problem's on the same field -- whose space is a subspace of the periodic one --, on a checkerboard strictly"""
    tag, n = (hmg.Tet64, 3) if dim == 3 else (hmg.Tri64, 4)
    sgrid = driver.generate_conductivity(dim, n, 5)
    kw = dict(ctx=ctx, sigma_grid=sgrid, tolerance=1e-12)
    per = driver.periodic_homogenization_tensor(n, tag, 2, **kw)
    full = driver.dirichlet_homogenization_tensor(n, tag, 2, **kw)
    S = per["tensor"]
    assert np.abs(S - S.T).max() == 0.0
    flat = sgrid.reshape(-1, dim)
    harmonic, arithmetic = np.diag(1.0 / (1.0 / flat).mean(axis=0)), np.diag(flat.mean(axis=0))
    ev = np.linalg.eigvalsh(S)
    assert ev[0] >= harmonic.diagonal().min() * (1 - 1e-8) and ev[-1] <= arithmetic.diagonal().max() * (1 + 1e-8)
    assert np.linalg.eigvalsh(S - harmonic)[0] >= -1e-8 and np.linalg.eigvalsh(arithmetic - S)[0] >= -1e-8
    dp, df = np.diag(S), np.diag(full["tensor"])
    print(f"periodic {dp}, dirichlet {df}")
    assert (dp <= df * (1.0 + 1e-8)).all() and (dp < df).all()


def test_polycrystal_runs_and_gives_an_spd_tensor(ctx):
    n = 3
    sgrid = driver.generate_polycrystal(3, n, 8)
    assert sgrid.shape == (n, n, n, 3, 3)
    out = driver.periodic_homogenization_tensor(n, hmg.Tet64, 1, ctx=ctx, sigma_grid=sgrid, tolerance=1e-10, smoother="jacobi")
    S = out["tensor"]
    assert np.abs(S - S.T).max() == 0.0 and np.linalg.eigvalsh(S)[0] > 0.0
    assert np.abs(out["tensor_flux"] - S).max() <= 1e-6 * np.abs(S).max()
    assert max(out["residual"]) <= 1e-10


@pytest.mark.parametrize("medium", ["diagonal", "full"])
@pytest.mark.parametrize("dim,refinements", [(2, 2), (3, 1)], ids=["2d", "3d"])
def test_periodic_driver_against_the_direct_solve(oracle, ctx, dim, refinements, medium):
    """every entry of both forms of the tensor against the energies of the d direct correctors on the explicitly refined torus;
    the mean gradient over the torus is e_k (the corrector's gradient is mean-free: every wrapped cell's geometry enters)"""
    n = 3
    mesh = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, n)
    if medium == "full":
        sgrid = driver.generate_polycrystal(3, 3, 8) if dim == 3 else TS.random_spd(np.random.default_rng(8), 9, 2).reshape(3, 3, 2, 2)
    else:
        sgrid = driver.generate_conductivity(dim, n, 5)                  # (seed 5: off-diagonal entries in 2D and in 3D)
    sys = TorusSystem(oracle, mesh, per_cube(mesh, sgrid), refinements)
    eye = np.eye(dim)
    V = [sys.corrector(eye[k]) for k in range(dim)]
    want = np.array([[sys.energy(V[k], eye[k], eye[l], V[l]) for l in range(dim)] for k in range(dim)])
    off = np.abs(want[np.triu_indices(dim, 1)])
    assert off.min() > 1e-3 * np.abs(want).max(), want                   # (on the reference: the off-diagonal entries are there)
    out = driver.periodic_homogenization_tensor(n, hmg.Tet64 if dim == 3 else hmg.Tri64, refinements, ctx=ctx, sigma_grid=sgrid,
                                                tolerance=1e-12, fields=True)
    scale = np.abs(want).max()
    e_t, e_f = np.abs(out["tensor"] - want).max() / scale, np.abs(out["tensor_flux"] - want).max() / scale
    vol = out["volumes"]
    grad = np.einsum("c,kcd->kd", vol, out["means"]) / vol.sum()
    e_g = np.abs(grad - eye).max()
    print(f"{dim}D, {medium}: cycles {out['cycles']}, tensor {e_t:.2e}, flux form {e_f:.2e}, mean gradient {e_g:.2e}, "
          f"off-diagonal {off.min() / scale:.2e} of the largest entry")
    assert e_t <= 1e-8 and e_f <= 1e-8
    assert e_g <= 1e-11
    for k in range(dim):
        for l in range(dim):
            assert np.array_equal(out["pairs"][k, l], out["pairs"][l, k])


def test_periodic_driver_on_large_cells(ctx):
    """the laminate of test_periodic_driver_is_exact_for_a_laminate on 3 x 3 cubes at level 9 (18 cells larger than the LDS): exact
    through the window kernels of the moments, refused -- after the solve, by hmg_fields.cpp -- without `large_cells`"""
    from homogenization_jl_amd._lib import HmgError
    n = 3
    layers, sgrid = _laminate(2, n)
    want = np.diag([n / (1.0 / layers[:, 0]).sum(), layers[:, 1].mean()])
    kw = dict(ctx=ctx, sigma_grid=sgrid, tolerance=1e-12)
    n0 = ctx.counter("cell_moments_window_launches")
    out = driver.periodic_homogenization_tensor(n, hmg.Tri64, 8, large_cells=True, **kw)
    launches = ctx.counter("cell_moments_window_launches") - n0
    print(f"cycles {out['cycles']}, tensor error {np.abs(out['tensor'] - want).max():.3e}, flux error "
          f"{np.abs(out['tensor_flux'] - want).max():.3e}, {launches} window launches")
    assert np.abs(out["tensor"] - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(out["tensor_flux"] - want).max() <= 1e-8 * np.abs(want).max()
    assert launches >= 3                                                 # (two correctors and their pair)
    assert ctx.counter("cell_moments_windows") == 0                      # (the option is back where it was)
    with pytest.raises(HmgError, match=r"level 9 .*does not fit the LDS.*cell_moments_windows"):
        driver.periodic_homogenization_tensor(n, hmg.Tri64, 8, **kw)
