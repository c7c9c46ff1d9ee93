"""The Chebyshev-Jacobi smoother (include/hmg.h: hmg_grid_set_smoother_chebyshev, kind 2) and the V-cycle around it, stated twice
on the CPU.  The two statements share no code:

`lambda_hi_local` / `smoothing_steps_cheb` / `vcycle_cheb` use the oracle's cell-local operations on Nf x Ne arrays, with dinv from
tests/_pcg_smoother_form.py (the oracle's operator tables).  The bound comes from the same tables, as sparse matrices:

    s[i, c]   = sum_j | (lambda |J_c| M + sum_ab |J_c| P_ab(c) D_ab)[i, j] |        (the cell's own absolute row sum)
    lambda_hi = 1.02 * max over the storage of dinv o (interface sum of s)
    lambda_lo = lambda_hi / ratio
    theta = (hi + lo) / 2;  delta = (hi - lo) / 2;  sigma1 = theta / delta;  rho_0 = 1 / sigma1
    r = b - A x, constraint, interface sum;  d = (1 / theta) dinv o r
    steps x { x += d;  Ad = A d, constraint, interface sum;  r -= Ad;
              rho_{k+1} = 1 / (2 sigma1 - rho_k);  d = (rho_{k+1} rho_k) d + (2 rho_{k+1} / delta) dinv o r }

Tails (the names of smooth_form() in csrc/hmg_smooth.cpp): "full" as above (p holds the next d), "scratch_p" ends with x += d, r -= Ad,
"dead_xp" ends with x += d alone -- no apply for the last step.

Both operator objects are served: the oracle's L2PlusDivAGrad (diagonal sigma) and tests/_tensor_sigma_form.py's TensorOp (a full
symmetric tensor per cell, P = J^-1 sigma J^-T from its coefficient_rows, its mul and local_residual) -- with a TensorOp the
inverse diagonals are _tensor_sigma_form.inverse_diagonal's and the level-1 solve _tensor_sigma_form.make_base_level's.  The
constraint is the operator's own, whichever face set it was built from (tests/_dirichlet_faces_form.py: oracle_constraint).  A
level without a free entry (dinv = 0 everywhere) has the bound 0 and no interval: the smoother is not stated there.

`ChebGlobalForm` is tests/_global_form.py's GlobalForm (global vectors, assembled matrices) with 1 / A.diagonal() on the interior
nodes; it takes the interval as numbers.  In both, the V-cycle is the reference's (src/multigrid.jl:73-119): `steps` is not
forwarded, level 1 is solved directly."""
import numpy as np

import _tensor_sigma_form as T
from _dirichlet_faces_form import FaceSetForm, all_faces, default_faces, oracle_constraint
from _global_form import GlobalForm
from _pcg_smoother_form import first_copy_residual_norm, inverse_diagonal

SAFETY = 1.02
DEFAULT_RATIO = 30.0     # the ratio with the fewest V-cycles over the cases of its table
# convergence_case (tests/_pcg_smoother_form.py) with the default ratio, 14 V-cycles of three steps: the residual factor per cycle, mean
# of the last six, as this statement measures it (0.7651; the CG smoother 0.811, the Jacobi-preconditioned one 0.554), and the pin
# both tests/test_cheb_smoother_statement.py and the device test hold: the margin of 0.03 kind 1 has over its own number
CONVERGENCE_FACTOR = 0.765
CONVERGENCE_PIN = CONVERGENCE_FACTOR + 0.03


def _is_tensor(A):
    return isinstance(A, T.TensorOp)


def _scaled_P(O, base, A):
    """(|J|, |J| P) per cell, P = J^-1 sigma J^-T: (Ne,), (Ne, dim, dim)"""
    dim = base.dim
    if _is_tensor(A):
        rows = T.coefficient_rows(O, base, A.sig)                # |J| P, upper triangle by rows, then |J|
        iu = np.triu_indices(dim)
        dP = np.empty((base.nelements(), dim, dim))
        dP[:, iu[0], iu[1]] = rows[:, :iu[0].size]
        dP[:, iu[1], iu[0]] = rows[:, :iu[0].size]
        return rows[:, iu[0].size], dP
    _, Jinv, det = O.cell_geometry(base)
    return det, det[:, None, None] * np.einsum("eki,ek,ekj->eij", Jinv, A.sigmas, Jinv)


def _mul(O, alpha, base, A, x, y):
    return T.mul(O, alpha, base, A, x, y) if _is_tensor(A) else O.mul(alpha, base, A, x, y)


def _local_residual(O, implicit, A, curr, k):
    return T.local_residual(O, implicit, A, curr, k) if _is_tensor(A) else O.local_residual(implicit, A, curr, k)


def cell_local_rowabs(O, implicit, A, chunk=64):
    """Nf x Ne: the absolute row sums of every cell's own lambda M + K_sigma.  One sparse matrix per distinct coefficient row:
    the terms share one sparsity pattern (the union), a coefficient row weighs their values, the row sums are one sparse product."""
    import scipy.sparse as sp
    base = implicit.base
    dim = base.dim
    det, dP = _scaled_P(O, base, A)
    terms = [A.mass.tocoo()] + [A.diffusion_terms[a][b].tocoo() for a in range(dim) for b in range(dim)]
    coef = np.column_stack([A.lam * det] + [dP[:, a, b] for a in range(dim) for b in range(dim)])            # Ne x (1 + dim^2)
    nf = A.mass.shape[0]
    keys = [t.row.astype(np.int64) * nf + t.col for t in terms]
    pattern = np.unique(np.concatenate(keys))
    vals = np.zeros((len(terms), pattern.size))
    for q, (t, k) in enumerate(zip(terms, keys)):
        np.add.at(vals[q], np.searchsorted(pattern, k), t.data)
    to_row = sp.csr_matrix((np.ones(pattern.size), (np.arange(pattern.size), pattern // nf)), shape=(pattern.size, nf))
    rows, inverse = np.unique(coef, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    s = np.empty((rows.shape[0], nf))
    for i in range(0, rows.shape[0], chunk):
        s[i:i + chunk] = (to_row.T @ np.abs(rows[i:i + chunk] @ vals).T).T
    return np.asfortranarray(s[inverse].T)


def lambda_hi_local(O, implicit, A, k, dinv):
    s = cell_local_rowabs(O, implicit, A)
    O.broadcast_interfaces(s, implicit, k)
    return SAFETY * float((dinv * s).max())


def bounds_local(O, implicit, ops, grids, dinvs):
    """[None, hi of level 2, ...]"""
    return [None] + [lambda_hi_local(O, implicit, ops[k - 1], k, dinvs[k - 1]) for k in range(2, grids + 1)]


def inverse_diagonals(O, implicit, ops, grids):
    return [None] + [(T.inverse_diagonal if _is_tensor(ops[k - 1]) else inverse_diagonal)(O, implicit, ops[k - 1], k)
                     for k in range(2, grids + 1)]


def coefficients(lo, hi, steps):
    """c0 and [(c1, c2)] of `steps` steps, in the order the recurrences of the statement form them."""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    out = []
    for _ in range(steps):
        rho1 = 1.0 / (2.0 * sigma1 - rho)
        out.append((rho1 * rho, 2.0 * rho1 / delta))
        rho = rho1
    return 1.0 / theta, out


def smoothing_steps_cheb(O, steps, implicit, A, curr, k, dinv, lo, hi, tail="full"):
    c0, cs = coefficients(lo, hi, steps)
    _local_residual(O, implicit, A, curr, k)
    O.broadcast_interfaces(curr.r, implicit, k)
    curr.p[...] = c0 * (dinv * curr.r)
    for i in range(steps):
        last = i == steps - 1
        curr.x += curr.p
        if last and tail == "dead_xp":
            return
        curr.Ap.fill(0.0)
        _mul(O, 1.0, implicit.base, A, curr.p, curr.Ap)
        O.apply_constraint(curr.Ap, k, A.constraint, implicit)
        O.broadcast_interfaces(curr.Ap, implicit, k)
        curr.r -= curr.Ap
        if last and tail == "scratch_p":
            return
        c1, c2 = cs[i]
        curr.p[...] = c1 * curr.p + c2 * (dinv * curr.r)


def vcycle_cheb(O, implicit, base_level, ops, levels, k, steps, dinvs, his, ratio=DEFAULT_RATIO):
    """dinvs[l], his[l]: inverse diagonal and lambda_hi of level l + 1 (entry 0 is not used: level 1 is solved)."""
    if k == 1:
        O.vcycle(implicit, base_level, ops, levels, 1)
        return
    curr, nxt = levels[k - 1], levels[k - 2]
    P = implicit.reference.interops[k - 2]
    hi = his[k - 1]
    smoothing_steps_cheb(O, steps, implicit, ops[k - 1], curr, k, dinvs[k - 1], hi / ratio, hi)
    _local_residual(O, implicit, ops[k - 1], curr, k)
    O.restrict_to(nxt.b, P, curr.r)
    nxt.x.fill(0.0)
    vcycle_cheb(O, implicit, base_level, ops, levels, k - 1, 2, dinvs, his, ratio)       # `steps` is not forwarded (src/multigrid.jl:109)
    O.interpolate_and_sum_to(curr.x, P, nxt.x)
    smoothing_steps_cheb(O, steps, implicit, ops[k - 1], curr, k, dinvs[k - 1], hi / ratio, hi)


def residual_history_cheb(O, case, ratio=DEFAULT_RATIO, cycles=14, steps=3, his=None):
    """The residual norms of tests/_pcg_smoother_form.py's residual_history with the Chebyshev smoother."""
    base, cond, implicit, constraint, ops, states, base_level, x0, _ = case
    grids = len(states)
    top = states[-1]
    top.x[...] = x0
    top.b.fill(0.0)
    O.local_rhs(top.b, implicit)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    his = bounds_local(O, implicit, ops, grids, dinvs) if his is None else his
    rs = []
    for _ in range(cycles):
        vcycle_cheb(O, implicit, base_level, ops, states, grids, steps, dinvs, his, ratio)
        rs.append(first_copy_residual_norm(O, implicit, ops[-1], top, grids))
    return np.array(rs)


class ChebOracle:
    """The oracle with vcycle_cheb in the place of its V-cycle: what tests/_fcg_form.py's fcg_local takes as `O` to state the
    flexible CG around the Chebyshev-smoothed V-cycle."""

    def __init__(self, O, dinvs, his, ratio=DEFAULT_RATIO):
        self._O, self._dinvs, self._his, self._ratio = O, dinvs, his, ratio

    def __getattr__(self, name):
        return getattr(self._O, name)

    def vcycle(self, implicit, base_level, ops, levels, k, steps=2):
        vcycle_cheb(self._O, implicit, base_level, ops, levels, k, steps, self._dinvs, self._his, self._ratio)


class ChebGlobalForm(GlobalForm):
    """his[l]: lambda_hi of level index l (0-based; entry 0 is not used)."""

    def set_interval(self, his, ratio=DEFAULT_RATIO):
        self.his, self.ratio = his, ratio
        return self

    def dinv(self, l):
        return np.where(self.inner[l], 1.0 / self.A[l].diagonal(), 0.0)

    def gershgorin(self, l):
        """max over the interior rows of sum_j |a_ij| / a_ii: the assembled matrix's own bound of lambda_max(D^-1 A)"""
        rows = np.asarray(abs(self.A[l]).sum(axis=1)).reshape(-1)
        return float((self.dinv(l) * rows).max())

    def lambda_max(self, l):
        """the largest eigenvalue of D^-1 A on the free nodes (Lanczos on the symmetric D^-1/2 A D^-1/2)"""
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        idx = np.flatnonzero(self.inner[l])
        A = self.A[l][idx][:, idx]
        s = sp.diags(1.0 / np.sqrt(A.diagonal()))
        return float(spla.eigsh((s @ A @ s).tocsc(), k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])

    def smooth(self, l, x, b, nsteps):
        A, inner, dinv = self.A[l], self.inner[l], self.dinv(l)
        hi = self.his[l]
        lo = hi / self.ratio
        theta, delta = (hi + lo) / 2, (hi - lo) / 2
        sigma1 = theta / delta
        rho = 1 / sigma1
        r = np.where(inner, b - A @ x, 0.0)
        d = dinv * r / theta
        for _ in range(nsteps):
            x = x + d
            r = r - np.where(inner, A @ d, 0.0)
            rho_next = 1 / (2 * sigma1 - rho)
            d = rho_next * rho * d + (2 * rho_next / delta) * (dinv * r)
            rho = rho_next
        return x, r


class ChebFaceSetForm(FaceSetForm, ChebGlobalForm):
    """ChebGlobalForm whose constrained nodes are those lying on a chosen face of the base mesh (FaceSetForm: geometry only),
    with one conductivity row per base cell."""


FACE_SET_CASES = {3: (20, 4), 2: (19, 5)}        # dim: (seed, levels) on hypercube(dim, 2), sigma in {1, 100}, lambda 0.7, perturbed by 0.2


def face_sets(mesh):
    """The constrained sets the bound is followed through, chosen on the lattice (before the nodes move): the default one (the
    outer boundary), none at all, every face of every cell."""
    return {"default": default_faces(mesh.elements), "empty": np.zeros((0, mesh.dim), dtype=np.int64),
            "every": all_faces(mesh.elements)[0]}


class FaceSetCase:
    """The oracle's side of one of FACE_SET_CASES, as tests/test_gpu_dirichlet_faces.py's Case draws it (nodes moved first, then
    sigma, from one generator); under(faces): operators, inverse diagonals and bounds with that set's constraint."""

    def __init__(self, O, dim, lam=0.7, perturb=0.2):
        self.O, self.dim, self.lam = O, dim, lam
        seed, self.levels = FACE_SET_CASES[dim]
        self.mesh = O.hypercube(dim, 2)
        self.sets = face_sets(self.mesh)
        rng = np.random.default_rng(seed)
        self.mesh.nodes = self.mesh.nodes + perturb * (rng.random(self.mesh.nodes.shape) - 0.5)
        self.sig = rng.choice([1.0, 100.0], size=(self.mesh.nelements(), dim))
        self.impl = O.ImplicitFineGrid.create(self.mesh, self.levels)
        self.tables = [(O.build_local_diffusion_operators(l), O.mass_matrix(l)) for l in self.impl.reference.levels]

    def under(self, faces):
        O = self.O
        cons = oracle_constraint(O, self.mesh, faces)
        ops = [O.L2PlusDivAGrad(d, m, cons, self.lam, self.sig) for d, m in self.tables]
        dinvs = inverse_diagonals(O, self.impl, ops, self.levels)
        return cons, ops, dinvs, bounds_local(O, self.impl, ops, self.levels, dinvs)
