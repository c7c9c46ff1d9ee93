"""The statements behind the periodic-grid tests, in numpy / scipy.  None of the C++ under test takes part (the table builder,
cell_edge_vectors, the level-1 projection); what they do rest on is the Python twin of the unwrap rule, `api.Mesh.cell_corners`,
and `vtk.construct_full_grid`, which places the fine nodes on those corners.  tests/test_periodic_host.py holds `cell_corners` to
the cells of the checkerboard box of the same shape (test_the_synthesiser).

A mesh on a torus is restated as DISJOINT SIMPLICES: every cell gets d + 1 nodes of its own, placed at its unwrapped corners
(`api.Mesh.cell_corners`: the cell's first corner plus the minimal images of the others) and numbered ascending in the cell's
own order.  That is an ordinary mesh without a single shared entity, so the oracle's cell-local operators and the textbook
elements of tests/_textbook_fem.py apply to it as they stand.  What makes it a torus again is said by POSITION: two nodes --
coarse or fine -- are the same node iff their positions agree modulo the period.  On the unit-cube tori of the tests every
position is a multiple of 1 / m, m = 2^(level - 1), so position * m modulo period * m is an exact integer key.  `general_torus`
moves, stretches and re-represents the nodes of such a torus by dyadic amounts: its positions are multiples of 1 / (16 m)
(`den` = 16), and the key stays exact.
"""
import numpy as np
import scipy.sparse as sp

from homogenization_jl_amd import vtk

from _textbook_fem import TextbookP1


def disjoint(mesh):
    """(nodes (Ne (d + 1), d), elements (Ne, d + 1) 0-based) of the disjoint simplices of an api.Mesh"""
    X = np.asarray(mesh.cell_corners(), dtype=np.float64)
    ne, nv, d = X.shape
    return X.reshape(-1, d), np.arange(ne * nv, dtype=np.int64).reshape(ne, nv)


def keys(pos, period, m, den=1):
    """one integer per position: (position * m * den) modulo (period * m * den), axis by axis; asserts that the positions are
    multiples of 1 / (m * den).  den = 1: the unit-cube tori; general_torus needs den = 16"""
    s = m * den
    q = np.asarray(pos, dtype=np.float64) * s
    k = np.rint(q).astype(np.int64)
    assert np.array_equal(k.astype(np.float64), q), "positions are no multiples of 1 / (m den)"
    Pq = np.asarray(period, dtype=np.float64) * s
    P = np.rint(Pq).astype(np.int64)
    assert np.array_equal(P.astype(np.float64), Pq), "the period is no multiple of 1 / (m den)"
    k %= P
    out = k[:, 0].copy()
    for a in range(1, k.shape[1]):
        out = out * P[a] + k[:, a]
    return out


DEN = 16        # general_torus: coarse positions are multiples of 1 / 16


def general_torus(shape, seed, *, jitter=True, scale=(2.0, 0.5, 1.0), shift=False):
    """driver.periodic_mesh(shape) with every node moved by a random vector of {-1/8, 0, 1/8}^d (`jitter`), positions and period
    multiplied by scale[:d], and (`shift`) a random whole number of periods in [-2, 2] per node and axis added to the stored
    representative.  Every number is a dyadic rational, so jitter, stretch and shift are exact; the shifted mesh is the same torus."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import driver
    d = len(shape)
    base = driver.periodic_mesh(hmg.Tet64 if d == 3 else hmg.Tri64, shape)
    rng = np.random.default_rng(seed)
    nodes = base.nodes.copy()
    move = rng.integers(-1, 2, size=nodes.shape) / 8.0                   # (drawn always: `jitter` does not move the stream)
    if jitter:
        nodes += move
    sc = np.asarray(scale, dtype=np.float64)[:d]
    nodes *= sc
    period = np.asarray(base.period, dtype=np.float64) * sc
    whole = rng.integers(-2, 3, size=nodes.shape).astype(np.float64)
    if shift:
        nodes += whole * period
    return hmg.Mesh(np.ascontiguousarray(nodes), base.elements.copy(), period)


def coarse_ids(mesh, den=1):
    """torus node id (0-based row of mesh.nodes) of every node of the disjoint simplices, found by position"""
    nodes, _ = disjoint(mesh)
    tk = keys(mesh.nodes, mesh.period, 1, den)
    order = np.argsort(tk)
    assert np.unique(tk).size == tk.size, "two torus nodes at one position"
    pos = np.searchsorted(tk[order], keys(nodes, mesh.period, 1, den))
    assert np.array_equal(tk[order][pos], keys(nodes, mesh.period, 1, den))
    return order[pos]


def fine_ids(g, level, den=1):
    """(ids (Nf, Ne), n): the torus fine node behind entry (hierarchical node, cell) of a level vector, and their number.  The
    positions are vtk.construct_full_grid's: slot_ijk / hier2slot on the unwrapped corners.  n = (coarse nodes) m^d, which holds
    on the Kuhn tori of driver.periodic_mesh however their nodes are moved."""
    nodes, _ = vtk.construct_full_grid(g, level)
    uniq, inv = np.unique(keys(nodes, g.base.period, 2 ** (level - 1), den), return_inverse=True)
    n = int(g.base.nodes.shape[0]) * (2 ** (level - 1)) ** g.base.dim
    assert uniq.size == n, (uniq.size, n)
    return inv.reshape(g.ncells(), g.nf(level)).T, n


def node_sum(a, ids, n):
    """u[node] = sum of all copies"""
    return np.bincount(ids.ravel(), weights=a.ravel(), minlength=n)


def broadcast(a, ids, n):
    """a with every copy of a torus node replaced by the sum of its copies"""
    return np.asfortranarray(node_sum(a, ids, n)[ids])


def stiffness(T, a_cell, ids, n, lam=0.0):
    """(lam M + K_a) of TextbookP1 T with the conductivity a_cell per cell -- (Ne, d) diagonal or (Ne, d, d) full --, its nodes
    identified by ids: n x n CSR"""
    nv = T.elements.shape[1]
    a_cell = np.asarray(a_cell, dtype=np.float64)
    if a_cell.ndim == 2:
        ag = T.grad * a_cell[:, None, :]
    else:
        ag = np.einsum("kid,kde->kie", T.grad, a_cell)
    loc = np.einsum("kid,kjd->kij", ag, T.grad) * T.vol[:, None, None]
    loc = loc + lam * (np.ones((nv, nv)) + np.eye(nv))[None, :, :] * (T.vol / (nv * (nv + 1)))[:, None, None]
    el = ids[T.elements]
    rows = np.repeat(el, nv, axis=1).ravel()
    cols = np.tile(el, (1, nv)).ravel()
    return sp.csr_matrix((loc.ravel(), (rows, cols)), shape=(n, n))


class TorusSystem:
    """The torus problem on the explicitly refined disjoint simplices: (lam M + K) u = F_xi.  cond: (Ne, d) or (Ne, d, d) per
    coarse cell.  pinned: a boolean mask over the torus fine nodes (this system's numbering), or a function of their positions
    (`self.pos`, modulo the period) that gives one; those nodes are fixed to zero.  With lam = 0 and nothing pinned the constants
    are in K's kernel."""

    def __init__(self, O, mesh, cond, refinements, lam=0.0, pinned=None, den=1):
        nodes, elements = disjoint(mesh)
        fine = O.refine_uniformly(O.Mesh(nodes, elements), times=refinements)
        self.m, self.den, self.lam = 2 ** refinements, den, float(lam)
        self.T = TextbookP1(fine.nodes, fine.elements)
        per_cell = fine.elements.shape[0] // elements.shape[0]              # (children of a cell are consecutive)
        self.a = np.repeat(np.asarray(cond, dtype=np.float64), per_cell, axis=0)
        uniq, first, self.ids = np.unique(keys(fine.nodes, mesh.period, self.m, den), return_index=True, return_inverse=True)
        self.n = uniq.size
        self.uniq = uniq
        self.period = np.asarray(mesh.period, dtype=np.float64)
        self.pos = np.mod(fine.nodes[first], self.period)
        self.K = stiffness(self.T, self.a, self.ids, self.n, self.lam)
        self.volume = float(self.T.vol.sum())
        if callable(pinned):
            pinned = pinned(self.pos)
        self.pinned = np.zeros(self.n, dtype=bool) if pinned is None else np.asarray(pinned, dtype=bool)
        assert self.pinned.shape == (self.n,)
        self.singular = self.lam == 0.0 and not self.pinned.any()

    def sigma_xi(self, xi):
        xi = np.asarray(xi, dtype=np.float64)
        return self.a * xi[None, :] if self.a.ndim == 2 else self.a @ xi

    def load(self, xi):
        """F_i = -int (sigma xi) . grad phi_i, summed over the copies of torus node i"""
        contrib = -self.T.vol[:, None] * np.einsum("kid,kd->ki", self.T.grad, self.sigma_xi(xi))
        return np.bincount(self.ids[self.T.elements].ravel(), weights=contrib.ravel(), minlength=self.n)

    def solve(self, F):
        """u with (lam M + K) u = F on the free nodes, 0 on the pinned ones; the singular system is solved with node 0 pinned
        (F must sum to zero) and the mean is left to the caller"""
        import scipy.sparse.linalg as spla
        free = ~self.pinned
        if self.singular:
            free = free.copy()
            free[0] = False
        idx = np.flatnonzero(free)
        u = np.zeros(self.n)
        u[idx] = spla.spsolve(self.K[idx][:, idx].tocsc(), np.asarray(F)[idx])
        return u

    def corrector(self, xi):
        """v with (lam M + K) v = -int sigma xi . grad phi on the free nodes; mean-free only where the system is singular"""
        if self.a.ndim == 2 and self.singular:                           # (the bits this statement had before tensors and pins)
            F = np.bincount(self.ids, weights=self.T.load(self.a, xi), minlength=self.n)
        else:
            F = self.load(xi)
        v = self.solve(F)
        return v - v.mean() if self.singular else v

    def gradients(self, v, xi):
        return np.einsum("kid,ki->kd", self.T.grad, v[self.ids][self.T.elements]) + np.asarray(xi, dtype=np.float64)[None, :]

    def energy(self, v, xi, eta=None, w=None):
        """int sigma grad(xi.x + v) . grad(eta.x + w) / |Omega|"""
        eta = xi if eta is None else eta
        w = v if w is None else w
        gu, gw = self.gradients(v, xi), self.gradients(w, eta)
        if self.a.ndim == 2:
            return float(np.sum(self.T.vol[:, None] * self.a * gu * gw) / self.volume)
        return float(np.sum(self.T.vol * np.einsum("kd,kde,ke->k", gu, self.a, gw)) / self.volume)

    def flux(self, v, xi):
        """int sigma grad(xi.x + v) / |Omega|: the row Sigma xi"""
        gu = self.gradients(v, xi)
        s = self.a * gu if self.a.ndim == 2 else np.einsum("kde,ke->kd", self.a, gu)
        return (self.T.vol[:, None] * s).sum(axis=0) / self.volume

    def index(self, pos):
        """this system's node numbers of positions given modulo the period"""
        k = keys(pos, self.period, self.m, self.den)
        at = np.searchsorted(self.uniq, k)
        assert np.array_equal(self.uniq[at], k)
        return at

    def gather(self, g, level, x):
        """nodal vector of a level vector (Nf, Ne) whose copies agree, in this system's numbering"""
        nodes, _ = vtk.construct_full_grid(g, level)
        u = np.zeros(self.n)
        u[self.index(nodes)] = np.asarray(x).T.ravel()
        return u
