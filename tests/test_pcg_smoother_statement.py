"""The CPU statements of the Jacobi-preconditioned CG smoother (tests/_pcg_smoother_form.py) that the device is held against
(tests/test_gpu_pcg_smoother.py): the cell-local one and the global one agree, the diagonal built from the oracle's operator
tables is the diagonal of the oracle's operator, and the smoother is worth having at high contrast.  No GPU; these pass with or
without the device feature -- they pin the yardstick."""
import numpy as np
import pytest

from _fcg_form import local_problem
from _pcg_smoother_form import (JacobiGlobalForm, cell_local_diagonal, convergence_case, inverse_diagonals, residual_history,
                                vcycle_jacobi)


def _field(rng, n, dim, contrast):
    return np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, float(contrast))


@pytest.mark.parametrize("dim,n,grids,lam", [(3, 2, 3, 0.7), (2, 4, 4, 0.7)])
def test_cell_local_diagonal_is_the_diagonal_of_the_oracles_operator(oracle, dim, n, grids, lam):
    """Unit-vector probes of O.mul on every level >= 2: column s of a probe holds e_s in every cell, the result's entry s is the
    cell's diagonal entry.  1e-13 relative (sums of at most 24 products each side)."""
    O = oracle
    rng = np.random.default_rng(5)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, _field(rng, n, dim, 100))
    for k in range(2, grids + 1):
        A = ops[k - 1]
        d = cell_local_diagonal(O, implicit, A)
        nf, ne = d.shape
        probe = np.zeros_like(d, order="F")
        for s in range(nf):
            e = np.zeros((nf, ne), order="F")
            e[s, :] = 1.0
            out = np.zeros((nf, ne), order="F")
            O.mul(1.0, base, A, e, out)
            probe[s, :] = out[s, :]
        assert np.abs(d - probe).max() <= 1e-13 * np.abs(probe).max(), (k, np.abs(d - probe).max())
        assert d.min() > 0.0


@pytest.mark.parametrize("dim,n,grids,lam,contrast", [(3, 2, 3, 0.7, 100), (2, 4, 4, 1.0, 100), (3, 2, 4, 1.0, 9)])
def test_cell_local_statement_equals_the_global_form(oracle, dim, n, grids, lam, contrast):
    """dinv on every level, x and r after one, two and three V-cycles of three smoothing steps: 1e-11 relative, the bound the CG
    statements are held to (measured: dinv <= 6e-16, x <= 7e-14, r <= 1.3e-14)."""
    O, steps = oracle, 3
    rng = np.random.default_rng(11)
    sgrid = _field(rng, n, dim, contrast)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    base_level = O.make_base_level(base, cond, lam)
    top = states[-1]
    top.x[...] = rng.random(top.x.shape)
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    O.local_rhs(top.b, implicit)
    G = JacobiGlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    for k in range(2, grids + 1):
        want = G.dinv(k - 1)
        got = G.gather(dinvs[k - 1], k - 1)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"level {k}: dinv {err:.2e}")
        assert err <= 1e-11, (k, err)
        assert np.array_equal(got == 0.0, ~G.inner[k - 1])
    gx, gb = G.gather(top.x, grids - 1), G.gather_sum(top.b, grids - 1)
    for cycle in range(3):
        vcycle_jacobi(O, implicit, base_level, ops, states, grids, steps, dinvs)
        gx, gr = G.vcycle(grids - 1, gx, gb, steps)
        ex = np.abs(G.gather(top.x, grids - 1) - gx).max() / np.abs(gx).max()
        er = np.abs(G.gather(top.r, grids - 1) - gr).max() / max(np.abs(gr).max(), 1e-300)
        print(f"cycle {cycle + 1}: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-11 and er <= 1e-11, (cycle, ex, er)


def test_jacobi_smoother_contracts_where_cg_stalls_at_contrast_100(oracle):
    """Why the smoother exists: residual factor per V-cycle, mean of cycles 9-14 -- the reference's CG smoother 0.811, the
    Jacobi-preconditioned one 0.554 (measured)."""
    O = oracle
    case = convergence_case(O)
    f = {}
    for smoother in ("cg", "jacobi"):
        rs = residual_history(O, case, smoother)
        f[smoother] = (rs[13] / rs[7]) ** (1.0 / 6.0)
        print(f"{smoother}: factor {f[smoother]:.3f}  residuals {rs[0]:.3e} ... {rs[13]:.3e}")
    assert f["cg"] >= 0.75, f
    assert f["jacobi"] <= 0.62, f
