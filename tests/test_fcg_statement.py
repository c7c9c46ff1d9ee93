"""The CPU statements of the V-cycle-preconditioned flexible CG (tests/_fcg_form.py) that the device is held against
(tests/test_gpu_fcg.py): they agree with each other, and the iteration is worth having.  No GPU; these pass with or without
the device feature -- they pin the yardstick."""
import numpy as np
import pytest

from _fcg_form import fcg_global, fcg_local, local_problem, residual_norm_global
from _global_form import GlobalForm


@pytest.mark.parametrize("dim,n,grids,steps", [(2, 4, 3, 3), (2, 3, 4, 1), (3, 2, 3, 3), (3, 2, 4, 3)])
def test_cell_local_statement_equals_the_global_form(oracle, dim, n, grids, steps):
    """Loads and consistent vectors on Nf x Ne arrays with plain dots over the storage against global vectors with assembled
    matrices, contrast 100, after each of 4 iterations: x to 1e-11 max|x|, R (summed over the copies) to 1e-11 max|R_0| -- the
    tolerance of test_vcycle_equals_its_global_matrix_form, whose set-up this is (measured: 1.2e-13 and 2.7e-14)."""
    O, lam = oracle, 1.0
    rng = np.random.default_rng(11)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 100.0)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    base_level = O.make_base_level(base, cond, lam)
    x0 = np.asfortranarray(rng.random(states[-1].x.shape))
    O.broadcast_interfaces(x0, implicit, grids)
    O.apply_constraint(x0, grids, constraint, implicit)
    b = np.zeros_like(x0, order="F")
    O.local_rhs(b, implicit)
    G = GlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    l = grids - 1
    gx, gb = G.gather(x0, l), G.gather_sum(b, l)
    r0 = np.abs(np.where(G.inner[l], gb - G.A[l] @ gx, 0.0)).max()
    glob = fcg_global(G, l, gx, gb, steps)
    loc = fcg_local(O, implicit, base_level, ops, states, grids, steps, x0, b)
    for it in range(4):
        wx, wR, wp, wa, wb = next(glob)
        x, R, p, alpha, beta = next(loc)
        ex = np.abs(G.gather(x, l) - wx).max() / np.abs(wx).max()
        eR = np.abs(G.gather_sum(R, l) - wR).max() / r0
        print(f"iteration {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.6f} / {wa:.6f}  beta {beta:.3e} / {wb:.3e}")
        assert ex <= 1e-11 and eR <= 1e-11, (it, ex, eR)
        assert abs(alpha - wa) <= 1e-9 * abs(wa) and abs(beta - wb) <= 1e-9 * max(abs(wb), 1e-300)


def test_fcg_needs_fewer_iterations_than_the_stationary_vcycle(oracle):
    """3D, n = 4, 4 grids, sigma in {1, 9}, 3 smoothing steps: the true residual falls below 1e-6 of its start within 10 FCG
    iterations; repeating the V-cycle needs more than 14 (measured: 10 and 16)."""
    O, dim, n, grids, steps, lam = oracle, 3, 4, 4, 3, 1.0
    rng = np.random.default_rng(11)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    base = O.hypercube(dim, n)
    implicit = O.ImplicitFineGrid.create(base, grids)
    G = GlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    l = grids - 1
    b = np.where(G.inner[l], rng.standard_normal(G.meshes[l].nnodes()), 0.0)
    x0 = np.where(G.inner[l], rng.random(G.meshes[l].nnodes()), 0.0)
    r0 = residual_norm_global(G, l, x0, b)
    it_fcg = None
    for it, (x, R, p, alpha, beta) in enumerate(fcg_global(G, l, x0, b, steps), 1):
        assert abs(np.linalg.norm(R) - residual_norm_global(G, l, x, b)) <= 1e-9 * r0     # the recurred residual is the true one
        if np.linalg.norm(R) < 1e-6 * r0:
            it_fcg = it
            break
        assert it < 40
    x, it_v = x0, None
    for it in range(1, 41):
        x, _ = G.vcycle(l, x, b, steps)
        if residual_norm_global(G, l, x, b) < 1e-6 * r0:
            it_v = it
            break
    print(f"to 1e-6: FCG {it_fcg} iterations, stationary V-cycle {it_v}")
    assert it_fcg is not None and it_fcg <= 10
    assert it_v is None or it_v > 14
