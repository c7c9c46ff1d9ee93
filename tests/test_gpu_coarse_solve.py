"""hmg_coarse_solve (the level-1 solve of the V-cycle, src/multigrid.jl:74-93: a device PCG with a Chebyshev preconditioner where
the reference factorises) against direct solves of its own exported matrix: tests/_coarse_form.py, splu in float64.  The shapes
are the ones at which the kernels of csrc/hmg_kernels.hip take another path; tests/test_coarse_solve_host.py proves on the CPU
that each mesh reaches the path its case is named for.  Tolerance of the call: 1e-10 (tests/test_gpu_tensor_sigma.py).

Case 4, the stopping rule at contrast 1e6 without a mass term: the library promises a recurrence residual of 1e-13; the true
residual rho and the forward error e are held to ten times what a float64 Jacobi-preconditioned scipy CG reaches on the same
matrix to the same rtol (computed again in every run).  Measured:

    mesh   n     scipy CG: it   rho_cg     e_cg       device: it   rho_dev    e_dev
    cu6    125             38   7.13e-14   7.34e-14           17   4.50e-14   3.38e-14
    sq16   225            146   3.71e-12   5.82e-12           33   1.85e-12   1.08e-11

(splu itself leaves a residual of 2.7e-16 and 9.5e-13 there.)  Case 3, 263 169 rows, lambda = 1e4: scipy CG 28 iterations,
rho_cg 4.4e-14; device 17 iterations, rho_dev 5.0e-14, x to 5.6e-14 of the direct solve.

Right-hand sides scaled by 1e-150 (case 6): 1e-26 b.b is below the smallest double and the dot products of the iteration
underflow on the way there; the solve runs to coarse_maxit and says so -- an error, as the case allows, not a silent zero.
Scaled by 1e+150 the solve is within tolerance.
"""
import time

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError
import _coarse_form as C

pytestmark = pytest.mark.gpu
TOL = 1e-10
LAM = 0.7


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class System:
    """a two-level grid on the device, its operator, and the direct solver of the matrix it exports"""

    def __init__(self, ctx, O, name, lam=LAM, values=(1.0, 9.0), seed=1, mesh=None):
        self.m = mesh if mesh is not None else C.mesh(O, name)
        self.name = name
        self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.m.nodes, self.m.elements + 1), 2)
        self.sig = C.two_valued(self.m, seed, values)
        self.op = hmg.L2PlusDivAGrad(self.g, lam, self.sig)
        self.bl = hmg.BaseLevel(self.g)
        self.cells, self.nnodes = self.m.elements, self.m.nnodes()
        self.refresh()

    def refresh(self):
        """the direct solver of the level-1 matrix the grid holds now"""
        A, interior = C.matrix(self.g)
        self.D = C.Direct(A, interior, self.cells, self.nnodes)
        return self.D

    def rand(self, seed):
        return np.asfortranarray(np.random.default_rng(seed).random((self.m.dim + 1, self.cells.shape[0])) - 0.5)

    def at_nodes(self, nodes, seed):
        """a right-hand side that is non-zero only at the copies of `nodes`"""
        return np.asfortranarray(self.rand(seed) * np.isin(self.cells.T, nodes))

    def solve(self, b1):
        """hmg_coarse_solve: (x1, b1 as the call leaves it)"""
        db = hmg.DeviceMatrix(self.g, 1).from_host(b1)
        dx = hmg.DeviceMatrix(self.g, 1).fill(7.0)                       # (every entry has to be written)
        L = hmg._lib
        try:
            L.check(L.load().hmg_coarse_solve(self.g.h, db.h, dx.h))
            return dx.to_host(), db.to_host()
        finally:
            db.close()
            dx.close()

    def broadcast_on_device(self, b1):
        db = hmg.DeviceMatrix(self.g, 1).from_host(b1)
        hmg.broadcast_interfaces(db, self.g, 1)
        out = db.to_host()
        db.close()
        return out

    def check(self, b1, tag="", want=None):
        x1, b_after = self.solve(b1)
        D = self.D
        want = D.solve(b1) if want is None else want
        err = C.relerr(x1, want)
        print(f"{self.name} {tag}: n {D.n} iterations {self.bl.last_iterations()} relerr {err:.2e}")
        assert np.isfinite(x1).all()
        assert err <= TOL, (self.name, tag, err)
        constrained = ~np.isin(self.cells.T, D.interior)
        assert (x1[constrained] == 0.0).all()
        # every copy of a node carries the same bits
        np.testing.assert_array_equal(C.distribute(self.cells, C.gather(self.cells, self.nnodes, x1)), x1)
        # the call sums b1 in place, as the reference does
        np.testing.assert_array_equal(b_after, self.broadcast_on_device(b1))
        np.testing.assert_allclose(b_after, C.broadcast(self.cells, self.nnodes, b1), rtol=1e-13, atol=1e-15 * np.abs(b1).max())
        return x1

    def close(self):
        self.g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. shapes of the row groups (four rows per group of 16 lanes: the clamp of the row pointers, `mine`)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sq1", "sq2", "sq3", "sq4", "cu2", "cu3", "cu4", "del2_18", "del2_19", "del2_20", "del2_21"])
def test_row_group_shapes(oracle, ctx, name):
    """n = 0, 1, 4, 9, 1, 8, 27 and 11 .. 14 unknowns"""
    s = System(ctx, oracle, name)
    try:
        assert s.D.n == C.UNKNOWNS[name]
        b1 = s.rand(3)
        first = s.check(b1, "counted")
        np.testing.assert_array_equal(s.check(b1, "budgeted"), first)
        if s.D.n == 0:
            assert (first == 0.0).all() and s.bl.last_iterations() == 0
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rows of more than 16 and of more than 32 entries (the extra trips of coarse_rows_product)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["del3_120", "fan2", "fan3"])
def test_long_rows(oracle, ctx, name):
    s = System(ctx, oracle, name)
    try:
        rows = C.row_lengths(s.D.A)
        i = int(np.argmax(rows))
        assert rows[i] > (32 if name.startswith("fan") else 16)
        centre = s.D.interior[i]
        shell = np.setdiff1d(s.D.interior[s.D.A[i].indices], [centre])
        for b1, tag in ((s.rand(5), "random"), (s.at_nodes([centre], 6), "the long row's node alone"),
                        (s.at_nodes(shell, 7), "its neighbours alone")):     # (the long row is then the one that matters)
            s.g.coarse_setup()                                           # (each right-hand side: counted, then under its own budget)
            first = s.check(b1, tag)
            np.testing.assert_array_equal(s.check(b1, tag + ", budgeted"), first)
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the second trip of the grid-stride loops: 263 169 rows, above 4 * 16 * 1024 (products) and 256 * 1024 (init, update)
# ---------------------------------------------------------------------------------------------------------------------------
def test_second_loop_trips(oracle, ctx):
    """lambda = 1e4: the mass term dominates, the iteration is short and the test is about the loops"""
    t0 = time.time()
    s = System(ctx, oracle, "sq514", lam=1.0e4)
    t1 = time.time()
    try:
        assert s.D.n == 263169 > 256 * 1024 > 4 * 16 * 1024
        b1 = s.rand(8)
        x1 = s.check(b1, "lambda 1e4")
        t2 = time.time()
        u = s.D.rhs(b1)
        x_cg, it_cg = C.jacobi_cg(s.D.A, u)
        rho_cg = C.true_residual(s.D.A, u, x_cg)
        rho_dev = s.D.residual(b1, s.D.interior_of(x1))
        print(f"sq514: grid, matrix and splu {t1 - t0:.1f} s, solve and checks {t2 - t1:.1f} s; scipy CG {it_cg} iterations "
              f"rho_cg {rho_cg:.2e}; device {s.bl.last_iterations()} iterations rho_dev {rho_dev:.2e}")
        assert rho_dev <= 10.0 * max(1e-13, rho_cg)
        np.testing.assert_array_equal(s.check(b1, "budgeted"), x1)
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the stopping rule under bad conditioning
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cu6", "sq16"])
def test_stopping_rule_at_contrast_1e6_without_a_mass_term(oracle, ctx, name):
    s = System(ctx, oracle, name, lam=0.0, values=(1.0, 1.0e6))
    try:
        D = s.D
        b1 = s.rand(9)
        u = D.rhs(b1)
        x_lu = D.solve_interior(b1)
        x_cg, it_cg = C.jacobi_cg(D.A, u, rtol=1e-13)
        rho_cg = C.true_residual(D.A, u, x_cg)
        e_cg = np.abs(x_cg - x_lu).max() / np.abs(x_lu).max()
        x1, _ = s.solve(b1)
        it_dev = s.bl.last_iterations()
        x_dev = D.interior_of(x1)
        rho_dev = D.residual(b1, x_dev)
        e_dev = np.abs(x_dev - x_lu).max() / np.abs(x_lu).max()
        print(f"{name}: n {D.n} scipy CG: it {it_cg} rho_cg {rho_cg:.2e} e_cg {e_cg:.2e}   device: it {it_dev} rho_dev {rho_dev:.2e} "
              f"e_dev {e_dev:.2e}   (splu: rho {D.residual(b1, x_lu):.2e})")
        assert rho_dev <= 10.0 * max(1e-13, rho_cg), (rho_dev, rho_cg)
        assert e_dev <= 10.0 * max(1e-10, e_cg), (e_dev, e_cg)
        assert 0 < it_dev < 5000                                         # coarse_maxit
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. counted against budgeted solves
# ---------------------------------------------------------------------------------------------------------------------------
def test_counted_and_budgeted_solves_give_the_same_bits(oracle, ctx):
    """Every kernel returns at once when S_DONE is set, partial sums are folded in a fixed order and the bookkeeping launch
    publishes the same r.z again: how often the host looks does not show in x."""
    s = System(ctx, oracle, "sq16", values=(1.0, 100.0))
    try:
        b1 = s.rand(10)
        xa = s.check(b1, "counted")
        it = s.bl.last_iterations()
        assert it > 5
        xb = s.check(b1, "budgeted")
        ctx.sync()
        xc = s.check(b1, "budgeted, after a sync")
        assert s.bl.last_iterations() == it and s.bl.misses() == 0
        np.testing.assert_array_equal(xb, xa)
        np.testing.assert_array_equal(xc, xa)
        # a harder right-hand side under the budget counted for b1: within tolerance, or reported as a miss -- never silently wrong
        hard = s.at_nodes(s.D.interior[:1], 11)
        x1, _ = s.solve(hard)
        try:
            ctx.sync()
            missed = False
        except HmgError as e:
            assert "did not reach coarse_rtol" in str(e)
            missed = True
        print(f"harder right-hand side, budgeted: {'a miss, reported' if missed else 'converged'}")
        assert s.bl.misses() == (1 if missed else 0)
        if not missed:
            assert C.relerr(x1, s.D.solve(hard)) <= TOL
        s.check(hard, "after it")                                        # (after a miss: counted again)
        # how often the counted solve looks: coarse_check = 1 and 25
        try:
            for every in (1, 25):
                ctx.set_option("coarse_check", every)
                s.g.coarse_setup()                                       # (the next solve counts)
                xe = s.check(b1, f"counted, coarse_check {every}")
                assert s.bl.last_iterations() == it
                np.testing.assert_array_equal(xe, xa)
        finally:
            ctx.set_option("coarse_check", 25)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. degenerate right-hand sides
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_right_hand_sides(oracle, ctx):
    s = System(ctx, oracle, "cu4")
    try:
        for turn in ("counted", "budgeted"):
            x1 = s.check(np.zeros_like(s.rand(0)), f"b1 = 0, {turn}")
            assert (x1 == 0.0).all()
            outside = np.setdiff1d(np.arange(s.nnodes), s.D.interior)
            b1 = s.at_nodes(outside, 12)
            assert np.abs(b1).max() > 0
            x1 = s.check(b1, f"b1 on constrained nodes only, {turn}")
            assert (x1 == 0.0).all()
            s.check(s.rand(13), f"random b1 after them, {turn}")
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


@pytest.mark.parametrize("scale", [1e-150, 1e150])
def test_right_hand_sides_whose_squares_leave_the_range(oracle, ctx, scale):
    """b.b under- or overflows: the solve is within tolerance or the call reports an error -- no silent zero, no NaN"""
    s = System(ctx, oracle, "cu4")
    try:
        for turn in ("counted", "budgeted"):
            b1 = s.rand(14) * scale
            want = s.D.solve(s.rand(14)) * scale
            try:
                x1, _ = s.solve(b1)
                ctx.sync()
            except HmgError as e:
                print(f"scale {scale:g}, {turn}: reported: {e}")
                continue
            err = C.relerr(x1, want)
            print(f"scale {scale:g}, {turn}: relerr {err:.2e}")
            assert np.isfinite(x1).all() and err <= TOL, (scale, turn, err)
        s.g.coarse_setup()
        s.check(s.rand(15), "an ordinary right-hand side after them")
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. a new matrix
# ---------------------------------------------------------------------------------------------------------------------------
def test_new_lambda_and_new_sigma(oracle, ctx):
    s = System(ctx, oracle, "cu6")
    try:
        b1 = s.rand(16)
        x_old = s.check(b1, "first matrix")
        s.check(b1, "budgeted")
        a_old = s.D.A.copy()
        s.op.lam = 2.5                                                   # hmg_grid_set_lambda; the solve forms the system itself
        x1, _ = s.solve(b1)
        assert abs(s.refresh().A - a_old).max() > 1e-3
        assert C.relerr(x1, s.D.solve(b1)) <= TOL and C.relerr(x1, x_old) > 1e-3
        s.check(b1, "lambda 2.5")
        # a new sigma while the probe of a budgeted solve is pending
        s.solve(b1)
        op2 = hmg.L2PlusDivAGrad(s.g, 2.5, C.two_valued(s.m, 17, (1.0, 1.0e3)))
        hmg.BaseLevel(s.g)
        a_old = s.D.A.copy()
        assert abs(s.refresh().A - a_old).max() > 1.0
        s.check(b1, "sigma in {1, 1e3}")
        s.check(b1, "budgeted")
        ctx.sync()
        assert s.bl.misses() == 0 and op2.lam == 2.5
    finally:
        s.close()


def test_shrunk_grid(oracle, ctx):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 6, origin=(-3.0, -3.0, -3.0)))
    s = System(ctx, O, "cu6 by magnitude", mesh=m)
    try:
        b_full = s.rand(18)
        s.check(b_full, "whole")
        s.check(b_full, "budgeted")
        ne, nn = O.find_elements_in_radius(m, 2), O.find_nodes_in_radius(m, 2)
        s.g.shrink(ne, nn)
        hmg.BaseLevel(s.g)
        s.cells, s.nnodes = np.ascontiguousarray(m.elements[:ne]), nn
        D = s.refresh()
        sub = O.Mesh(m.nodes[:nn], s.cells)
        np.testing.assert_array_equal(D.interior, O.list_interior_nodes(sub))
        assert 0 < D.n < 125
        b1 = np.asfortranarray(b_full[:, :ne])
        s.check(b1, "shrunk")
        s.check(b1, "budgeted")
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()


def test_dirichlet_faces_of_the_caller(oracle, ctx):
    O = oracle
    s = System(ctx, O, "cu4")
    try:
        b1 = s.rand(19)
        s.check(b1, "default faces")
        s.check(b1, "budgeted")
        base = hmg.Mesh(s.m.nodes, s.m.elements + 1)
        x = s.m.nodes[:, 0]
        mid = 0.5 * (x.min() + x.max())
        faces = driver.faces_on_plane(base, 0, mid)
        assert faces.shape[0] > 0
        s.g.set_dirichlet_faces(faces)
        hmg.BaseLevel(s.g)
        D = s.refresh()
        on_plane = np.flatnonzero(np.abs(x - mid) <= 1e-9)
        np.testing.assert_array_equal(D.interior, np.setdiff1d(np.arange(s.nnodes), on_plane))    # the table follows the set
        s.check(b1, "a plane inside")
        s.check(b1, "budgeted")
        # no constraint at all: every node is an unknown (lambda > 0)
        s.g.set_dirichlet_faces(np.zeros((0, 3), dtype=np.int64))
        hmg.BaseLevel(s.g)
        D = s.refresh()
        assert D.n == s.nnodes == 125
        s.check(b1, "no constrained node")
        s.check(b1, "budgeted")
        ctx.sync()
        s.op.lam = 0.0                                                   # ... which without a mass term is singular
        with pytest.raises(HmgError, match="no node is constrained.*lambda = 0"):
            hmg.BaseLevel(s.g)
        with pytest.raises(HmgError, match="no node is constrained.*lambda = 0"):
            s.solve(b1)
        s.op.lam = LAM
        s.g.set_dirichlet_faces(None)
        hmg.BaseLevel(s.g)
        assert s.refresh().n == 27
        s.check(b1, "default faces again")
        assert s.bl.misses() == 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. options of the preconditioner
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cu6", "fan3"])
def test_preconditioner_options(oracle, ctx, name):
    s = System(ctx, oracle, name)
    try:
        b1 = s.rand(20)
        got = {}
        try:
            for poly in (1, 2, 4, 16):
                for ratio in (2.0, 20.0, 1000.0):
                    ctx.set_option("coarse_poly", poly)
                    ctx.set_option("coarse_poly_ratio", ratio)
                    s.g.coarse_setup()                                   # (the next solve counts its iterations)
                    got[poly, ratio] = s.check(b1, f"coarse_poly {poly} ratio {ratio:g}")
                    s.check(b1, "budgeted", want=got[poly, ratio])
        finally:
            ctx.set_option("coarse_poly", 4)
            ctx.set_option("coarse_poly_ratio", 20.0)
        assert C.relerr(got[1, 20.0], got[4, 20.0]) <= TOL
        ctx.sync()
        assert s.bl.misses() == 0
    finally:
        s.close()
