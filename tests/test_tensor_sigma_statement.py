"""Pins the yardstick of the tensor-operator tests: tests/_tensor_sigma_form.py with sigma = Q D Q^T in every cell is the real
oracle's diagonal operator on the mesh x -> Q^T x -- operator, residual, right-hand side, V-cycle.  No library code runs here."""
import numpy as np
import pytest

import _tensor_sigma_form as T

CASES = [(3, 2, 3), (2, 4, 4)]          # dim, n, grids


def rotated_pair(O, dim, n, grids, lam=0.5, seed=11):
    rng = np.random.default_rng(seed)
    base = O.hypercube(dim, n)
    Q = T.random_rotation(rng, dim)
    D = np.array([1.0, 100.0, 9.0])[:dim]                # contrast 100
    S = (Q * D[None, :]) @ Q.T
    sig = np.ascontiguousarray(np.broadcast_to(0.5 * (S + S.T), (base.nelements(), dim, dim)))
    prob = T.Problem(O, base, grids, lam, sig)
    # the real oracle: diagonal field, rotated mesh
    mr = T.rotated_mesh(O, base, Q)
    cond = np.ascontiguousarray(np.broadcast_to(D, (base.nelements(), dim)))
    implicit = O.ImplicitFineGrid.create(mr, grids)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(mr))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), constraint, lam, cond)
           for l in implicit.reference.levels]
    states = [O.LevelState.create(mr.nelements(), implicit.nf(i + 1)) for i in range(grids)]
    shape = states[-1].x.shape
    x0 = np.asfortranarray(rng.random(shape))
    b0 = np.asfortranarray(rng.random(shape) - 0.5)
    return prob, (mr, cond, implicit, constraint, ops, states, O.make_base_level(mr, cond, lam)), Q, D, x0, b0


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_operator_and_residual(oracle, dim, n, grids):
    O = oracle
    prob, (mr, cond, implicit, constraint, ops, states, _), Q, D, x0, b0 = rotated_pair(O, dim, n, grids)
    for alpha in (1.0, -1.0, 0.375):
        y = b0.copy(order="F")
        T.mul(O, alpha, prob.base, prob.ops[-1], x0, y)
        want = b0.copy(order="F")
        O.mul(alpha, mr, ops[-1], x0, want)
        print("mul", alpha, rel(y, want))
        assert rel(y, want) <= 1e-13                      # (measured 9e-16)
    top, otop = prob.states[-1], states[-1]
    top.x[...] = otop.x[...] = x0
    top.b[...] = otop.b[...] = b0
    T.local_residual(O, prob.implicit, prob.ops[-1], top, grids)
    O.local_residual(implicit, ops[-1], otop, grids)
    assert rel(top.r, otop.r) <= 1e-13
    # the diagonals of the Jacobi smoother
    d = T.cell_local_diagonal(O, prob.implicit, prob.ops[-1])
    from _pcg_smoother_form import cell_local_diagonal
    assert rel(d, cell_local_diagonal(O, implicit, ops[-1])) <= 1e-13


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_right_hand_side_and_first_term(oracle, dim, n, grids):
    """xi on the plain mesh is Q^T xi on the rotated one"""
    O = oracle
    prob, (mr, cond, implicit, constraint, ops, states, _), Q, D, x0, b0 = rotated_pair(O, dim, n, grids)
    xi = np.array([0.3, -1.0, 0.7])[:dim]
    b, want = np.zeros_like(b0), np.zeros_like(b0)
    T.rhs_axi_grad_v(O, b, O.partial_derivatives_functionals(prob.implicit.reference.levels[-1]), prob.implicit, prob.sig, xi)
    dphis = O.partial_derivatives_functionals(implicit.reference.levels[-1])
    O.rhs_axi_grad_v(want, dphis, implicit, cond, Q.T @ xi)
    assert rel(b, want) <= 1e-13
    nsub = prob.base.nelements() - 2
    got = T.integrate_first_term(O, x0, dphis, prob.implicit, nsub, prob.mass[-1], prob.sig, xi)
    ref = O.integrate_first_term(x0, dphis, implicit, nsub, O.mass_matrix(implicit.reference.levels[-1]), cond, Q.T @ xi)
    assert abs(got - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_vcycles(oracle, dim, n, grids):
    """x and r after one, two and three V-cycles (three smoothing steps): 1e-11"""
    O = oracle
    prob, (mr, cond, implicit, constraint, ops, states, base_level), Q, D, x0, b0 = rotated_pair(O, dim, n, grids)
    prob.start(x0, b0)
    top = states[-1]
    top.x[...] = x0
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    top.b[...] = b0
    for cycle in range(3):
        prob.cycle(3)
        O.vcycle(implicit, base_level, ops, states, grids, 3)
        ex, er = rel(prob.states[-1].x, top.x), rel(prob.states[-1].r, top.r)
        print("cycle", cycle + 1, ex, er)
        assert ex <= 1e-11 and er <= 1e-11


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_jacobi_vcycles(oracle, dim, n, grids):
    """... and with the Jacobi-preconditioned smoother, against tests/_pcg_smoother_form.py on the rotated mesh"""
    import _pcg_smoother_form as J
    O = oracle
    prob, (mr, cond, implicit, constraint, ops, states, base_level), Q, D, x0, b0 = rotated_pair(O, dim, n, grids)
    prob.start(x0, b0)
    top = states[-1]
    top.x[...] = x0
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    top.b[...] = b0
    dinvs, odinvs = prob.dinvs(), J.inverse_diagonals(O, implicit, ops, grids)
    for cycle in range(2):
        prob.cycle(3, dinvs)
        J.vcycle_jacobi(O, implicit, base_level, ops, states, grids, 3, odinvs)
        ex, er = rel(prob.states[-1].x, top.x), rel(prob.states[-1].r, top.r)
        print("jacobi cycle", cycle + 1, ex, er)
        assert ex <= 1e-11 and er <= 1e-11
