"""The V-cycle-preconditioned flexible CG iteration with one retained direction (Notay's FCG(1)), stated twice on the CPU:
`fcg_global` on global vectors with tests/_global_form.py's GlobalForm (its V-cycle as the preconditioner, assembled matrices,
ordinary dot products) and `fcg_local` with the oracle's cell-local operations on Nf x Ne arrays, where x, z, p are consistent
vectors, b, R, q are loads, and the plain dot product over the storage of one of each is the global inner product.  The device
(include/hmg.h, hmg_fcg_*) is held against both; tests/test_fcg_statement.py holds them against each other.

    R = b - A x on the interior, 0 on the boundary
    z = V(0, R);  first: p = z, later: beta = -(z.q) / (p.q)_prev, p = z + beta p
    q = A p on the interior;  alpha = (p.R) / (p.q);  x += alpha p;  R -= alpha q
"""
import numpy as np


def fcg_global(G, l, x, b, steps):
    """Generator: (x, R, p, alpha, beta) after every iteration on level index l (0-based) of GlobalForm G."""
    A, inner = G.A[l], G.inner[l]
    x = x.copy()
    R = np.where(inner, b - A @ x, 0.0)
    p = q = pq = None
    while True:
        z, _ = G.vcycle(l, np.zeros_like(x), R, steps)
        beta = 0.0 if p is None else -float(z @ q) / pq
        p = z.copy() if p is None else z + beta * p
        q = np.where(inner, A @ p, 0.0)
        pq = float(p @ q)
        alpha = float(p @ R) / pq
        x = x + alpha * p
        R = R - alpha * q
        yield x, R, p, alpha, beta


def residual_norm_global(G, l, x, b):
    return float(np.linalg.norm(np.where(G.inner[l], b - G.A[l] @ x, 0.0)))


def fcg_local(O, implicit, base_level, ops, states, k, steps, x, b):
    """The same with the oracle's cell-local operations; k is the 1-based top level, `states` its LevelStates (the top
    level's x, b, r, p, Ap are the V-cycle's work space), x consistent and constrained, b a load.  Yields copies."""
    A, top = ops[k - 1], states[k - 1]
    dot = lambda u, v: float(np.dot(u.reshape(-1, order="F"), v.reshape(-1, order="F")))

    def a_loc(alpha, v, out):
        O.mul(alpha, implicit.base, A, v, out)
        O.apply_constraint(out, k, A.constraint, implicit)
        return out

    x = np.asfortranarray(x.copy())
    R = a_loc(-1.0, x, np.asfortranarray(b.copy()))
    p = q = pq = None
    while True:
        top.b[...] = R
        top.x.fill(0.0)
        O.vcycle(implicit, base_level, ops, states, k, steps)
        z = top.x
        beta = 0.0 if p is None else -dot(z, q) / pq
        p = np.asfortranarray(z.copy() if p is None else z + beta * p)
        q = a_loc(1.0, p, np.zeros_like(p, order="F"))
        pq = dot(p, q)
        alpha = dot(p, R) / pq
        x = np.asfortranarray(x + alpha * p)
        R = np.asfortranarray(R - alpha * q)
        yield x.copy(order="F"), R.copy(order="F"), p.copy(order="F"), alpha, beta


def local_problem(O, dim, n, grids, lam, sgrid):
    """Oracle-side objects of a hypercube(dim, n) problem with `grids` levels (as test_vcycle_equals_its_global_matrix_form)."""
    base = O.hypercube(dim, n)
    cond = O.conductivity_per_element(base, sgrid, (0.0,) * dim)
    implicit = O.ImplicitFineGrid.create(base, grids)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(m), O.mass_matrix(m), constraint, lam, cond)
           for m in implicit.reference.levels]
    states = [O.LevelState.create(base.nelements(), implicit.nf(i + 1)) for i in range(grids)]
    return base, cond, implicit, constraint, ops, states
