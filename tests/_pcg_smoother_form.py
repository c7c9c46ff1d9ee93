"""The Jacobi-preconditioned CG smoother (include/hmg.h: hmg_grid_set_smoother, kind 1) and the V-cycle around it, stated twice
on the CPU.  The two statements share no code:

`inverse_diagonal` / `smoothing_steps_jacobi` / `vcycle_jacobi` use the oracle's cell-local operations on Nf x Ne arrays.  The
diagonal comes from the oracle's operator tables (the reference-element matrices of L2PlusDivAGrad and the cell geometry), not
from any stencil table:

    dinv = 0 on constrained nodes, else 1 / (interface sum of the cell-local diagonal of lambda M + K_sigma)
    r = b - A x, constraint, interface sum;  z = dinv o r;  p = z;  rz = dot(r, z)       (dot over the storage, copies counted)
    steps x { Ap = A p, constraint, interface sum;  alpha = rz / dot(p, Ap);  x += alpha p;  r -= alpha Ap;
              rz' = dot(r, dinv o r);  p = dinv o r + (rz'/rz) p;  rz = rz' }

`JacobiGlobalForm` is tests/_global_form.py's GlobalForm (global vectors, assembled matrices) with 1 / A.diagonal() on the
interior nodes and the multiplicity-weighted dot product.  In both, the V-cycle is the reference's (src/multigrid.jl:73-119):
`steps` is not forwarded, level 1 is solved directly."""
import numpy as np

from _global_form import GlobalForm


def cell_local_diagonal(O, implicit, A):
    """Nf x Ne: the diagonal of every cell's own lambda M + K_sigma (before the interface sum)."""
    base = implicit.base
    _, Jinv, det = O.cell_geometry(base)
    P = np.einsum("eki,ek,ekj->eij", Jinv, A.sigmas, Jinv)
    d = np.outer(A.mass.diagonal(), A.lam * det)
    for a in range(base.dim):
        for b in range(base.dim):
            d += np.outer(A.diffusion_terms[a][b].diagonal(), det * P[:, a, b])
    return np.asfortranarray(d)


def free_nodes(O, implicit, A, k):
    """Nf x Ne booleans: the entries the constraint leaves alone."""
    ones = np.ones((A.mass.shape[0], implicit.base.nelements()), order="F")
    O.apply_constraint(ones, k, A.constraint, implicit)
    return ones == 1.0


def inverse_diagonal(O, implicit, A, k):
    d = cell_local_diagonal(O, implicit, A)
    O.broadcast_interfaces(d, implicit, k)
    free = free_nodes(O, implicit, A, k)
    return np.asfortranarray(np.where(free, 1.0 / np.where(free, d, 1.0), 0.0))


def _dot(u, v):
    return float(np.dot(u.reshape(-1, order="F"), v.reshape(-1, order="F")))


def smoothing_steps_jacobi(O, steps, implicit, A, curr, k, dinv):
    O.local_residual(implicit, A, curr, k)
    O.broadcast_interfaces(curr.r, implicit, k)
    curr.p[...] = dinv * curr.r
    rz = _dot(curr.r, curr.p)
    for _ in range(steps):
        curr.Ap.fill(0.0)
        O.mul(1.0, implicit.base, A, curr.p, curr.Ap)
        O.apply_constraint(curr.Ap, k, A.constraint, implicit)
        O.broadcast_interfaces(curr.Ap, implicit, k)
        alpha = rz / _dot(curr.p, curr.Ap)
        curr.x += alpha * curr.p
        curr.r -= alpha * curr.Ap
        z = dinv * curr.r
        rz_new = _dot(curr.r, z)
        curr.p[...] = z + (rz_new / rz) * curr.p
        rz = rz_new


def vcycle_jacobi(O, implicit, base_level, ops, levels, k, steps, dinvs):
    """dinvs[l] = inverse_diagonal of level l + 1 (entry 0 is not used: level 1 is solved)."""
    if k == 1:
        O.vcycle(implicit, base_level, ops, levels, 1)
        return
    curr, nxt = levels[k - 1], levels[k - 2]
    P = implicit.reference.interops[k - 2]
    smoothing_steps_jacobi(O, steps, implicit, ops[k - 1], curr, k, dinvs[k - 1])
    O.local_residual(implicit, ops[k - 1], curr, k)
    O.restrict_to(nxt.b, P, curr.r)
    nxt.x.fill(0.0)
    vcycle_jacobi(O, implicit, base_level, ops, levels, k - 1, 2, dinvs)       # `steps` is not forwarded (src/multigrid.jl:109)
    O.interpolate_and_sum_to(curr.x, P, nxt.x)
    smoothing_steps_jacobi(O, steps, implicit, ops[k - 1], curr, k, dinvs[k - 1])


def inverse_diagonals(O, implicit, ops, grids):
    return [None] + [inverse_diagonal(O, implicit, ops[k - 1], k) for k in range(2, grids + 1)]


def first_copy_residual_norm(O, implicit, A, curr, k):
    """norm of b - A x, constrained, summed over the interfaces, every node counted once (curr.r is overwritten)"""
    O.local_residual(implicit, A, curr, k)
    O.broadcast_interfaces(curr.r, implicit, k)
    O.zero_out_all_but_one(curr.r, implicit, k)
    return float(np.linalg.norm(curr.r))


def convergence_case(O):
    """3D, n = 4, four grids, lambda = 0, sigma in {1, 100} per direction, right-hand side local_rhs, random x0."""
    dim, n, grids, lam = 3, 4, 4, 0.0
    rng = np.random.default_rng(3)
    sgrid = np.where(rng.random((4, 4, 4, 3)) < 0.5, 1.0, 100.0)
    x0 = np.asfortranarray(rng.random((165, 384)))
    from _fcg_form import local_problem
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    O.broadcast_interfaces(x0, implicit, grids)
    O.apply_constraint(x0, grids, constraint, implicit)
    return base, cond, implicit, constraint, ops, states, O.make_base_level(base, cond, lam), x0, sgrid


def residual_history(O, case, smoother, cycles=14, steps=3):
    base, cond, implicit, constraint, ops, states, base_level, x0, _ = case
    grids = len(states)
    top = states[-1]
    top.x[...] = x0
    top.b.fill(0.0)
    O.local_rhs(top.b, implicit)
    dinvs = inverse_diagonals(O, implicit, ops, grids) if smoother == "jacobi" else None
    rs = []
    for _ in range(cycles):
        if smoother == "jacobi":
            vcycle_jacobi(O, implicit, base_level, ops, states, grids, steps, dinvs)
        else:
            O.vcycle(implicit, base_level, ops, states, grids, steps)
        rs.append(first_copy_residual_norm(O, implicit, ops[-1], top, grids))
    return np.array(rs)


class JacobiOracle:
    """The oracle with vcycle_jacobi in the place of its V-cycle: what tests/_fcg_form.py's fcg_local takes as `O` to state the
    flexible CG around the Jacobi-smoothed V-cycle."""

    def __init__(self, O, dinvs):
        self._O, self._dinvs = O, dinvs

    def __getattr__(self, name):
        return getattr(self._O, name)

    def vcycle(self, implicit, base_level, ops, levels, k, steps=2):
        vcycle_jacobi(self._O, implicit, base_level, ops, levels, k, steps, self._dinvs)


class JacobiGlobalForm(GlobalForm):
    def dinv(self, l):
        return np.where(self.inner[l], 1.0 / self.A[l].diagonal(), 0.0)

    def smooth(self, l, x, b, nsteps):
        A, inner, mult, dinv = self.A[l], self.inner[l], self.mult[l], self.dinv(l)
        mdot = lambda u, v: float(np.dot(mult * u, v))
        r = np.where(inner, b - A @ x, 0.0)
        p = dinv * r
        rz = mdot(r, p)
        for _ in range(nsteps):
            Ap = np.where(inner, A @ p, 0.0)
            alpha = rz / mdot(p, Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            z = dinv * r
            rz_new = mdot(r, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
        return x, r
