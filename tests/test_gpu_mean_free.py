"""
The level-1 solve on the complement of the constants (hmg_grid_set_mean_free, k_coarse_remove_mean) where its one workgroup of
1024 threads strides -- n = 1024, 1025 and 2197 unknowns --, the natural-boundary problem on an ordinary grid, and the regular
systems a grid with `mean_free` on must NOT project: a torus with a plane of fixed potential, a torus with lambda > 0.

References: level 1, a sparse direct solve of the exported matrix (tests/_coarse_form.py; tests/test_periodic_host.py holds the
matrix to the textbook assembly) with one node pinned and the mean removed behind; converged answers, a sparse direct solve of
the textbook system on the explicitly refined mesh (tests/_periodic_form.py: TorusSystem; an ordinary box: TextbookP1).
Bounds are the project's: level-1 solve 1e-10 (tests/test_gpu_coarse_solve.py), converged answers 1e-8 at tolerance 1e-12.  The
first is not vacuous: a PCG stopped at coarse_rtol = 1e-13 is within kappa 1e-13 of the answer, kappa the condition on the
complement of the constants, and the tests assert kappa 1e-13 <= 1e-10 on the reference before they look at the device.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

import _cell_extrema_form as X
import _coarse_form as CF
from _periodic_device import per_cube, relerr
from _periodic_form import TorusSystem, fine_ids, stiffness
from _textbook_fem import TextbookP1

pytestmark = pytest.mark.gpu

COARSE_RTOL = 1e-13


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def solve_level_1(ctx, g, db, dx, b1):
    """hmg_coarse_solve of b1 (the solve leaves the interface sum in its right-hand side, so it is uploaded anew); no allocation"""
    lib = hmg._lib
    db.from_host(b1)
    dx.fill(7.0)                                                         # (every entry has to be written)
    allocs = ctx.counter("device_allocs")
    lib.check(lib.load().hmg_coarse_solve(g.h, db.h, dx.h))
    ctx.sync()
    assert ctx.counter("device_allocs") == allocs
    return dx.to_host()


def on_the_complement(A, u):
    """the mean-free x with A x = u - mean(u), A symmetric with exactly the constants in its kernel: node 0 pinned, sparse LU"""
    A = A.tocsr()
    x = np.zeros(A.shape[0])
    x[1:] = spla.spsolve(A[1:][:, 1:].tocsc(), (u - u.mean())[1:])
    return x - x.mean()


def kappa_on_the_complement(A):
    """lambda_max / lambda_2 of a matrix with one zero eigenvalue (dense: the callers' matrices have at most 1024 rows)"""
    w = np.linalg.eigvalsh(A.toarray())
    assert abs(w[0]) <= 1e-12 * w[-1] and w[1] > 1e-9 * w[-1]
    return w[-1] / w[1]


def check_singular_solves(ctx, g, cells, nn, rng, kappa):
    """constants 0, 3, 0, -250 on the right-hand side, as tests/test_gpu_periodic.py::test_level_1_solve_against_the_pseudo_inverse"""
    assert kappa * COARSE_RTOL <= 1e-10, kappa                          # (the bound below says something)
    A, interior = CF.matrix(g)
    np.testing.assert_array_equal(interior, np.arange(nn))
    dim = cells.shape[1] - 1
    db, dx = hmg.DeviceMatrix(g, 1), hmg.DeviceMatrix(g, 1)
    worst = 0.0
    for constant in (0.0, 3.0, 0.0, -250.0):
        b1 = np.asfortranarray(rng.standard_normal((dim + 1, cells.shape[0])) + constant)
        want = on_the_complement(A, CF.node_sum(cells, nn, b1))
        x1 = solve_level_1(ctx, g, db, dx, b1)
        xg = CF.gather(cells, nn, x1)
        np.testing.assert_array_equal(CF.distribute(cells, xg), x1)
        err = relerr(xg, want)
        worst = max(worst, err)
        print(f"n {nn}, constant {constant:g}: x {err:.2e}  mean {abs(xg.mean()):.2e}  max {np.abs(xg).max():.2e}  kappa {kappa:.4g}")
        assert err <= 1e-10, err
        assert abs(xg.mean()) <= 1e-13 * np.abs(xg).max()
        again = solve_level_1(ctx, g, db, dx, b1)
        assert np.array_equal(again.view(np.int64), x1.view(np.int64))
    for v in (db, dx):
        v.close()
    return worst


# ---- a. the torus at sizes that stride ------------------------------------------------------------------------------------------
KAPPA = {(25, 41): 734.0, (13, 13, 13): 71.5}      # on the complement, from a CPU run of this recipe (dense eigenvalues)


@pytest.mark.parametrize("shape", [(32, 32), (25, 41), (13, 13, 13)], ids=["32x32", "25x41", "13x13x13"])
def test_level_1_solve_where_the_mean_kernel_strides(ctx, shape):
    """n = 1024: one entry per thread exactly; 1025: one thread has two; 2197: three strides with a ragged tail"""
    dim = len(shape)
    mesh = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, shape)
    nn = mesh.nodes.shape[0]
    assert nn == int(np.prod(shape))
    rng = np.random.default_rng(7)
    g = hmg.ImplicitFineGrid(ctx, mesh, 2)
    assert g.mean_free()
    g.set_operator(per_cube(mesh, rng.choice([1.0, 9.0], size=tuple(shape) + (dim,))), 0.0)
    g.coarse_setup()
    kappa = KAPPA[shape] if shape in KAPPA else kappa_on_the_complement(CF.matrix(g)[0])
    check_singular_solves(ctx, g, mesh.elements - 1, nn, rng, kappa)
    g.close()


# ---- b. the natural-boundary problem on a box -------------------------------------------------------------------------------------
def node_of_entry(points, fine_nodes):
    """the node of the explicitly refined mesh behind every entry of a level vector (cell-major, as vtk.construct_full_grid
    numbers them), found by position"""
    from scipy.spatial import cKDTree
    dist, at = cKDTree(fine_nodes).query(points)
    assert dist.max() <= 1e-12 * np.abs(fine_nodes).max() and np.unique(at).size == fine_nodes.shape[0]
    return at


def nodal(at, n, x):
    """the level vector x (Nf, Ne) as a nodal vector; the copies must agree bitwise"""
    flat = np.asarray(x).T.ravel()
    u = np.zeros(n)
    u[at] = flat
    np.testing.assert_array_equal(u[at], flat)                           # a consistent level vector
    return u


class Box:
    """the perturbed cube, sigma in {1, 9} per cell and direction, and the textbook system of the explicitly refined mesh with no
    constrained node: solved with node 0 pinned, then mean-free"""

    def __init__(self, O, dim, n, levels):
        self.dim, self.levels = dim, levels
        self.base = X.perturbed_cube(O, dim, n)
        self.cond = CF.two_valued(self.base, 31 + dim)
        self.fine = O.refine_uniformly(self.base, times=levels - 1)
        self.T = TextbookP1(self.fine.nodes, self.fine.elements)
        self.a = np.repeat(self.cond, self.fine.elements.shape[0] // self.base.nelements(), axis=0)
        self.n = self.fine.nodes.shape[0]
        self.K = stiffness(self.T, self.a, np.arange(self.n), self.n)
        self.lu = spla.splu(self.K[1:][:, 1:].tocsc())

    def solve(self, F):
        assert abs(F.sum()) <= 1e-12 * np.abs(F).sum()                   # (in the range: the constants see nothing)
        v = np.zeros(self.n)
        v[1:] = self.lu.solve(F[1:])
        return v - v.mean()

    def grid(self, ctx, smoother):
        """the device grid with no constrained node and the level-1 solve on the complement of the constants"""
        g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.base.nodes, self.base.elements + 1), self.levels)
        assert g.mean_free() is False
        g.set_smoother(smoother)
        op = hmg.L2PlusDivAGrad(g, 0.0, self.cond)
        g.set_dirichlet_faces(np.zeros((0, self.dim), dtype=np.int64))
        g.set_mean_free(True)
        return g, op


@pytest.fixture(scope="module", params=[(3, 2, 3), (2, 4, 4)], ids=["3d", "2d"])
def box(request, oracle):
    return Box(oracle, *request.param)


def test_natural_boundary_level_1_solve(ctx, box):
    dim, base = box.dim, box.base
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), box.levels)
    assert g.mean_free() is False
    g.set_operator(box.cond, 0.0)
    g.set_dirichlet_faces(np.zeros((0, dim), dtype=np.int64))
    with pytest.raises(HmgError, match="no node is constrained"):        # the flag is off: refused on the device grid too
        g.coarse_setup()
    g.set_mean_free(True)
    g.coarse_setup()
    assert g.interior_nodes().size == base.nnodes() and not g.table_i32("dmask").any()
    check_singular_solves(ctx, g, base.elements, base.nnodes(), np.random.default_rng(7), kappa_on_the_complement(CF.matrix(g)[0]))
    g.set_mean_free(False)
    with pytest.raises(HmgError, match="no node is constrained"):
        g.coarse_setup()
    g.close()


@pytest.mark.parametrize("smoother", ["cg", "chebyshev"])
def test_natural_boundary_converged_corrector(ctx, box, smoother):
    """The corrector of e_1 through driver._dirichlet_solve.  With no constrained node the affine function -x_1 is in the space,
    so the corrector IS -x_1 up to a constant, whatever sigma, and the energy of u = x_1 + v is zero: the reference's comes out as
    1e-26, rounding of rounding.  The corrector is held at 1e-8 as it stands; the energy -- a difference of terms of the size of
    int sigma_11 -- at 1e-8 of that size, the only scale a zero has.  (test_natural_boundary_random_load holds an energy that is
    not zero at 1e-8 of itself.)"""
    dim, levels, xi = box.dim, box.levels, np.eye(box.dim)[0]
    v = box.solve(box.T.load(box.a, xi))
    gu = np.einsum("kid,ki->kd", box.T.grad, v[box.T.elements]) + xi[None, :]
    energy = float(np.sum(box.T.vol[:, None] * box.a * gu * gu))
    scale = float(np.sum(box.T.vol * box.a[:, 0]))                       # int sigma e_1 . e_1
    line = -box.fine.nodes[:, 0]
    assert np.abs(v - (line - line.mean())).max() <= 1e-10 * np.abs(v).max() and abs(energy) <= 1e-20 * scale
    g, op = box.grid(ctx, smoother)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(levels)]
    xv = states[-1].x
    cycles, rnorm, r0 = driver._dirichlet_solve(g, op, bl, states, xv, None, xi, 3, 1e-12, 200, "test")
    assert rnorm <= 1e-12 * r0, (cycles, rnorm / r0)
    at = node_of_entry(hmg.vtk.construct_full_grid(g, levels)[0], box.fine.nodes)
    got = nodal(at, box.n, xv.to_host())
    err = np.linalg.norm((got - got.mean()) - v) / np.linalg.norm(v)
    _, gram = hmg.cell_moments(xv, g, xi)
    e_dev = float(hmg.fields.energy(box.cond, gram).sum())
    print(f"{dim}D natural boundary, {smoother}: {cycles} cycles, corrector {err:.2e}, energy {e_dev:.3e} / {energy:.3e} of {scale:.6g}")
    assert err <= 1e-8, err
    assert abs(e_dev - energy) <= 1e-8 * scale
    for s in states:
        s.close()
    g.close()


@pytest.mark.parametrize("smoother", ["cg", "chebyshev"])
def test_natural_boundary_random_load(ctx, box, smoother):
    """A load that no affine function answers: random cell-local contributions with zero total (so their nodal sums are in the
    range), V-cycles until the residual has fallen by 1e-12; the mean-free solution and its energy int sigma |grad v|^2 against the
    direct solve, both at 1e-8"""
    dim, levels = box.dim, box.levels
    g, op = box.grid(ctx, smoother)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(levels)]
    top = states[-1]
    at = node_of_entry(hmg.vtk.construct_full_grid(g, levels)[0], box.fine.nodes)
    b = np.random.default_rng(51 + dim).standard_normal((g.nf(levels), g.ncells()))
    b = np.asfortranarray(b - b.mean())
    F = np.bincount(at, weights=b.T.ravel(), minlength=box.n)
    v = box.solve(F)
    energy = float(v @ (box.K @ v))
    top.b.from_host(b)
    top.x.fill(0.0)

    def residual_norm():
        hmg.local_residual(g, op, top, levels)
        hmg.broadcast_interfaces(top.r, g, levels)
        return hmg.norm_unique(top.r)

    r0 = rnorm = residual_norm()
    cycles = 0
    while rnorm > 1e-12 * r0 and cycles < 200:
        hmg.vcycle(g, bl, [op] * levels, states, levels, 3)
        cycles += 1
        rnorm = residual_norm()
    assert rnorm <= 1e-12 * r0, (cycles, rnorm / r0)
    got = nodal(at, box.n, top.x.to_host())
    err = np.linalg.norm((got - got.mean()) - v) / np.linalg.norm(v)
    _, gram = hmg.cell_moments(top.x, g)
    e_dev = float(hmg.fields.energy(box.cond, gram).sum())
    print(f"{dim}D natural boundary, random load, {smoother}: {cycles} cycles, solution {err:.2e}, energy {e_dev:.12g} / {energy:.12g}")
    assert err <= 1e-8, err
    assert abs(e_dev - energy) <= 1e-8 * abs(energy)
    for s in states:
        s.close()
    g.close()


# ---- c. regular matrices with mean_free on are not projected ------------------------------------------------------------------------
REGULAR = [((3, 3, 3), 2), ((4, 3), 3)]


def regular_case(shape):
    dim = len(shape)
    mesh = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, shape)
    cond = per_cube(mesh, np.random.default_rng(41 + dim).choice([1.0, 9.0], size=tuple(shape) + (dim,)))
    return dim, mesh, cond


def check_regular_level_1(ctx, g, mesh, rng):
    """right-hand sides with a large mean against the direct solve of the exported matrix: the mean survives"""
    cells, nn = mesh.elements - 1, mesh.nodes.shape[0]
    A, interior = CF.matrix(g)
    direct = CF.Direct(A, interior, cells, nn)
    fixed = np.setdiff1d(np.arange(nn), interior)
    db, dx = hmg.DeviceMatrix(g, 1), hmg.DeviceMatrix(g, 1)
    for constant in (250.0, 0.0):
        b1 = np.asfortranarray(rng.standard_normal((mesh.dim + 1, cells.shape[0])) + constant)
        want = direct.nodal(direct.solve_interior(b1))
        x1 = solve_level_1(ctx, g, db, dx, b1)
        xg = CF.gather(cells, nn, x1)
        np.testing.assert_array_equal(CF.distribute(cells, xg), x1)
        err = relerr(xg, want)
        print(f"n {interior.size}, constant {constant:g}: x {err:.2e}  mean {xg[interior].mean():.3e} / {want[interior].mean():.3e}")
        assert err <= 1e-10, err
        assert np.all(xg[fixed] == 0.0)
        if constant:
            assert abs(want[interior].mean()) > 0.1 * np.abs(want).max()    # (on the reference: a projection would be seen)
            assert abs(xg[interior].mean() - want[interior].mean()) <= 1e-10 * np.abs(want).max()
    for v in (db, dx):
        v.close()


def converge(ctx, g, op, levels, xi):
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(levels)]
    cycles, rnorm, r0 = driver._dirichlet_solve(g, op, bl, states, states[-1].x, None, xi, 3, 1e-12, 200, "test")
    assert rnorm <= 1e-12 * r0, (cycles, rnorm / r0)
    x = states[-1].x.to_host()
    for s in states:
        s.close()
    ids, n = fine_ids(g, levels)
    u = np.zeros(n)
    u[ids.ravel()] = x.ravel()
    np.testing.assert_array_equal(u[ids], x)
    return cycles, x


@pytest.mark.parametrize("shape,levels", REGULAR, ids=["3x3x3", "4x3"])
def test_a_plane_of_fixed_potential_is_not_projected(oracle, ctx, shape, levels):
    dim, mesh, cond = regular_case(shape)
    g = hmg.ImplicitFineGrid(ctx, mesh, levels)
    assert g.mean_free()
    op = hmg.L2PlusDivAGrad(g, 0.0, cond)
    g.set_dirichlet_faces(driver.faces_on_plane(mesh, 0, 1.0))
    g.coarse_setup()
    check_regular_level_1(ctx, g, mesh, np.random.default_rng(7))
    xi = np.eye(dim)[0]
    sys = TorusSystem(oracle, mesh, cond, levels - 1, pinned=lambda pos: pos[:, 0] == 1.0)
    assert sys.pinned.sum() == int(np.prod(shape[1:])) * sys.m ** (dim - 1) and not sys.singular
    v = sys.corrector(xi)
    cycles, x = converge(ctx, g, op, levels, xi)
    got = sys.gather(g, levels, x)
    err = np.linalg.norm(got - v) / np.linalg.norm(v)
    print(f"{dim}D, plane x_1 = 1 fixed: {cycles} cycles, corrector {err:.2e}, mean {got.mean():.3e} / {v.mean():.3e}")
    assert err <= 1e-8, err
    assert np.all(got[sys.pinned] == 0.0)
    g.close()


@pytest.mark.parametrize("shape,levels", REGULAR, ids=["3x3x3", "4x3"])
def test_lambda_above_zero_is_not_projected(oracle, ctx, shape, levels):
    dim, mesh, cond = regular_case(shape)
    g = hmg.ImplicitFineGrid(ctx, mesh, levels)
    assert g.mean_free()
    op = hmg.L2PlusDivAGrad(g, 0.7, cond)
    g.coarse_setup()
    check_regular_level_1(ctx, g, mesh, np.random.default_rng(7))
    xi = np.eye(dim)[0]
    sys = TorusSystem(oracle, mesh, cond, levels - 1, lam=0.7)
    v = sys.corrector(xi)
    cycles, x = converge(ctx, g, op, levels, xi)
    got = sys.gather(g, levels, x)
    err = np.linalg.norm(got - v) / np.linalg.norm(v)
    print(f"{dim}D, lambda 0.7: {cycles} cycles, corrector {err:.2e}")
    assert err <= 1e-8, err
    g.close()
