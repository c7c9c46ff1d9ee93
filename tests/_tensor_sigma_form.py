"""lambda u - div(sigma grad u) with a FULL symmetric tensor sigma per base cell (include/hmg.h: hmg_grid_set_operator_tensor),
stated on the CPU.  The oracle knows diagonal tensors only, so the statement is made from its parts that do not depend on sigma:

  operator     y += alpha (sum_ab |J| P_ab K_ab x + lambda |J| M x), K_ab / M the oracle's reference-element matrices
               (build_local_diffusion_operators, mass_matrix) and P = J^-1 sigma J^-T from oracle.cell_geometry
  smoothers    the reference's CG (src/multigrid.jl:46-71) and tests/_pcg_smoother_form.py's Jacobi-preconditioned CG, restated
               over that operator; constraint, interface sums, restriction and prolongation are the oracle's
  V-cycle      src/multigrid.jl:73-119 (`steps` is not forwarded); level 1 is solved directly on a textbook P1 matrix with
               full tensors (assemble_p1)
  load         b = dphi . (-|J| J^-1 (sigma xi)), from the oracle's d phi functional tables

What ties it to the real oracle: for sigma = Q D Q^T in every cell it is the oracle's own diagonal operator on the mesh
x -> Q^T x (tests/test_tensor_sigma_statement.py)."""
import numpy as np
import scipy.sparse as sp

from _pcg_smoother_form import free_nodes


def rotated_mesh(O, mesh, Q):
    """the mesh x -> Q^T x"""
    return O.Mesh(np.ascontiguousarray(mesh.nodes @ Q), mesh.elements.copy())


def random_rotation(rng, dim):
    Q, R = np.linalg.qr(rng.standard_normal((dim, dim)))
    Q = Q * np.sign(np.diag(R))[None, :]
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def random_spd(rng, n, dim, lo=1.0, hi=100.0):
    """n tensors Q diag(d) Q^T, d log-uniform in [lo, hi], Q a random rotation: exactly symmetric"""
    out = np.empty((n, dim, dim))
    for c in range(n):
        Q = random_rotation(rng, dim)
        d = np.exp(rng.uniform(np.log(lo), np.log(hi), dim))
        S = (Q * d[None, :]) @ Q.T
        out[c] = 0.5 * (S + S.T)
    return out


def pack(sig):
    """(n, dim, dim) -> (n, ncomp): 3D 11, 12, 13, 22, 23, 33; 2D 11, 12, 22"""
    iu = np.triu_indices(sig.shape[1])
    return np.ascontiguousarray(sig[:, iu[0], iu[1]])


def coefficient_rows(O, base, sig):
    """(Ne, 8): |J| P in the order of pack(), then |J|, zero padded -- what table_f64("coef") holds"""
    _, Jinv, det = O.cell_geometry(base)
    P = np.einsum("eki,ekl,elj->eij", Jinv, sig, Jinv)
    rows = np.zeros((base.nelements(), 8))
    pk = pack(P) * det[:, None]
    rows[:, :pk.shape[1]] = pk
    rows[:, pk.shape[1]] = det
    return rows


class TensorOp:
    """what oracle.L2PlusDivAGrad is for diagonal tensors; sig: (Ne, dim, dim)"""

    def __init__(self, diffusion_terms, mass, constraint, lam, sig):
        self.diffusion_terms, self.mass, self.constraint, self.lam = diffusion_terms, mass, constraint, lam
        self.sig = np.ascontiguousarray(sig, dtype=np.float64)


def mul(O, alpha, base, A, x, y):
    """y <- alpha A x + y, cell-local"""
    _, Jinv, det = O.cell_geometry(base)
    P = np.einsum("eki,ekl,elj->eij", Jinv, A.sig, Jinv)
    acc = (A.mass @ x) * (A.lam * det)[None, :]
    for a in range(base.dim):
        for b in range(base.dim):
            acc += (A.diffusion_terms[a][b] @ x) * (det * P[:, a, b])[None, :]
    y += alpha * acc
    return y


def local_residual(O, implicit, A, curr, k):
    curr.r[...] = curr.b
    mul(O, -1.0, implicit.base, A, curr.x, curr.r)
    O.apply_constraint(curr.r, k, A.constraint, implicit)


def _dot(u, v):
    return float(np.dot(u.reshape(-1, order="F"), v.reshape(-1, order="F")))


def cell_local_diagonal(O, implicit, A):
    base = implicit.base
    _, Jinv, det = O.cell_geometry(base)
    P = np.einsum("eki,ekl,elj->eij", Jinv, A.sig, Jinv)
    d = np.outer(A.mass.diagonal(), A.lam * det)
    for a in range(base.dim):
        for b in range(base.dim):
            d += np.outer(A.diffusion_terms[a][b].diagonal(), det * P[:, a, b])
    return np.asfortranarray(d)


def inverse_diagonal(O, implicit, A, k):
    d = cell_local_diagonal(O, implicit, A)
    O.broadcast_interfaces(d, implicit, k)
    free = free_nodes(O, implicit, A, k)
    return np.asfortranarray(np.where(free, 1.0 / np.where(free, d, 1.0), 0.0))


def smoothing_steps(O, steps, implicit, A, curr, k, dinv=None):
    """dinv None: the reference's CG; else CG preconditioned by dinv (tests/_pcg_smoother_form.py)"""
    local_residual(O, implicit, A, curr, k)
    O.broadcast_interfaces(curr.r, implicit, k)
    curr.p[...] = curr.r if dinv is None else dinv * curr.r
    rz = _dot(curr.r, curr.p)
    for _ in range(steps):
        curr.Ap.fill(0.0)
        mul(O, 1.0, implicit.base, A, curr.p, curr.Ap)
        O.apply_constraint(curr.Ap, k, A.constraint, implicit)
        O.broadcast_interfaces(curr.Ap, implicit, k)
        alpha = rz / _dot(curr.p, curr.Ap)
        curr.x += alpha * curr.p
        curr.r -= alpha * curr.Ap
        z = curr.r if dinv is None else dinv * curr.r
        rz_new = _dot(curr.r, z)
        curr.p[...] = z + (rz_new / rz) * curr.p
        rz = rz_new


def assemble_p1(O, mesh, sig, lam):
    """textbook P1 matrix of int lam u v + grad u . sigma grad v, all nodes (CSR)"""
    dim, N = mesh.dim, mesh.dim + 1
    _, Jinv, det = O.cell_geometry(mesh)
    grads = np.einsum("eab,bn->ean", Jinv, O._REF_GRADS[dim])            # (Ne, dim, N)
    vol = det / (6.0 if dim == 3 else 2.0)
    gsg = np.einsum("eki,ekl,elj->eij", grads, sig, grads)
    massloc = (np.ones((N, N)) + np.eye(N)) / ((dim + 1) * (dim + 2))    # int phi_i phi_j / volume
    V = (vol[:, None, None] * (gsg + lam * massloc[None])).reshape(-1)
    els = mesh.elements
    I = np.repeat(els[:, :, None], N, axis=2).reshape(-1)
    J = np.repeat(els[:, None, :], N, axis=1).reshape(-1)
    A = sp.coo_matrix((V, (I, J)), shape=(mesh.nnodes(),) * 2).tocsr()
    A.sum_duplicates()
    return A


def make_base_level(O, base, sig, lam):
    interior = O.list_interior_nodes(base)
    A = assemble_p1(O, base, sig, lam)[interior][:, interior]
    return O.BaseLevel.create(O._SpluSolver(A), base.nnodes(), interior)


def vcycle(O, implicit, base_level, ops, levels, k, steps=2, dinvs=None):
    """dinvs: None (CG smoother) or the list of inverse_diagonal per level (entry 0 unused)"""
    if k == 1:
        O.vcycle(implicit, base_level, ops, levels, 1)          # (level 1 does not look at the operator: the direct solve)
        return
    curr, nxt = levels[k - 1], levels[k - 2]
    P = implicit.reference.interops[k - 2]
    dinv = None if dinvs is None else dinvs[k - 1]
    smoothing_steps(O, steps, implicit, ops[k - 1], curr, k, dinv)
    local_residual(O, implicit, ops[k - 1], curr, k)
    O.restrict_to(nxt.b, P, curr.r)
    nxt.x.fill(0.0)
    vcycle(O, implicit, base_level, ops, levels, k - 1, 2, dinvs)
    O.interpolate_and_sum_to(curr.x, P, nxt.x)
    smoothing_steps(O, steps, implicit, ops[k - 1], curr, k, dinv)


def rhs_axi_grad_v(O, b, dphis, implicit, sig, xi):
    _, Jinv, det = O.cell_geometry(implicit.base)
    P = -det[:, None] * np.einsum("eki,ek->ei", Jinv, sig @ np.asarray(xi, dtype=np.float64))
    b[...] = dphis @ P.T


def integrate_first_term(O, v0, dphis, implicit, nsubset, mass, sig, xi):
    _, Jinv, det = O.cell_geometry(implicit.base)
    P = -det[:, None] * np.einsum("eki,ek->ei", Jinv, sig @ np.asarray(xi, dtype=np.float64))
    V = v0[:, :nsubset]
    run = np.einsum("ie,ie->e", V, dphis @ P[:nsubset].T + mass @ V)
    return float(np.sum(run * det[:nsubset]))


class Problem:
    """base mesh, `grids` levels, one TensorOp per level, level states and the level-1 solve; top_only: the operator of the
    finest level alone (large cells: no V-cycle is stated)"""

    def __init__(self, O, base, grids, lam, sig, top_only=False):
        self.O, self.base, self.grids, self.lam, self.sig = O, base, grids, lam, sig
        self.implicit = O.ImplicitFineGrid.create(base, grids)
        self.constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
        refs = self.implicit.reference.levels
        made = [not top_only or i == grids - 1 for i in range(grids)]
        self.mass = [O.mass_matrix(m) if mk else None for m, mk in zip(refs, made)]
        self.ops = [TensorOp(O.build_local_diffusion_operators(m), M, self.constraint, lam, sig) if mk else None
                    for m, M, mk in zip(refs, self.mass, made)]
        if top_only:
            return
        self.states = [O.LevelState.create(base.nelements(), self.implicit.nf(i + 1)) for i in range(grids)]
        self.base_level = make_base_level(O, base, sig, lam)

    def rand(self, rng, level):
        return np.asfortranarray(rng.standard_normal((self.implicit.nf(level), self.base.nelements())))

    def dinvs(self):
        return [None] + [inverse_diagonal(self.O, self.implicit, self.ops[k - 1], k) for k in range(2, self.grids + 1)]

    def start(self, x0, b0):
        O, top = self.O, self.states[-1]
        top.x[...] = x0
        O.broadcast_interfaces(top.x, self.implicit, self.grids)
        O.apply_constraint(top.x, self.grids, self.constraint, self.implicit)
        top.b[...] = b0

    def cycle(self, steps, dinvs=None):
        vcycle(self.O, self.implicit, self.base_level, self.ops, self.states, self.grids, steps, dinvs)
