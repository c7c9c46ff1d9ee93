"""The statements behind the periodic-grid tests, in numpy / scipy.  None of the C++ under test takes part (the table builder,
cell_edge_vectors, the level-1 projection); what they do rest on is the Python twin of the unwrap rule, `api.Mesh.cell_corners`,
and `vtk.construct_full_grid`, which places the fine nodes on those corners.  tests/test_periodic_host.py holds `cell_corners` to
the cells of the checkerboard box of the same shape (test_the_synthesiser).

A mesh on a torus is restated as DISJOINT SIMPLICES: every cell gets d + 1 nodes of its own, placed at its unwrapped corners
(`api.Mesh.cell_corners`: the cell's first corner plus the minimal images of the others) and numbered ascending in the cell's
own order.  That is an ordinary mesh without a single shared entity, so the oracle's cell-local operators and the textbook
elements of tests/_textbook_fem.py apply to it as they stand.  What makes it a torus again is said by POSITION: two nodes --
coarse or fine -- are the same node iff their positions agree modulo the period.  On the unit-cube tori of the tests every
position is a multiple of 1 / m, m = 2^(level - 1), so position * m modulo period * m is an exact integer key.
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


def keys(pos, period, m):
    """one integer per position: (position * m) modulo (period * m), axis by axis; asserts that the positions are such multiples"""
    q = np.asarray(pos, dtype=np.float64) * m
    k = np.rint(q).astype(np.int64)
    assert np.array_equal(k.astype(np.float64), q), "positions are no multiples of 1 / m"
    P = np.rint(np.asarray(period, dtype=np.float64) * m).astype(np.int64)
    k %= P
    out = k[:, 0].copy()
    for a in range(1, k.shape[1]):
        out = out * P[a] + k[:, a]
    return out


def coarse_ids(mesh):
    """torus node id (0-based row of mesh.nodes) of every node of the disjoint simplices, found by position"""
    nodes, _ = disjoint(mesh)
    tk = keys(mesh.nodes, mesh.period, 1)
    order = np.argsort(tk)
    assert np.unique(tk).size == tk.size, "two torus nodes at one position"
    pos = np.searchsorted(tk[order], keys(nodes, mesh.period, 1))
    assert np.array_equal(tk[order][pos], keys(nodes, mesh.period, 1))
    return order[pos]


def fine_ids(g, level):
    """(ids (Nf, Ne), n): the torus fine node behind entry (hierarchical node, cell) of a level vector, and their number.  The
    positions are vtk.construct_full_grid's: slot_ijk / hier2slot on the unwrapped corners."""
    nodes, _ = vtk.construct_full_grid(g, level)
    uniq, inv = np.unique(keys(nodes, g.base.period, 2 ** (level - 1)), return_inverse=True)
    n = int(np.prod(np.asarray(g.base.period))) * (2 ** (level - 1)) ** g.base.dim
    assert uniq.size == n, (uniq.size, n)
    return inv.reshape(g.ncells(), g.nf(level)).T, n


def node_sum(a, ids, n):
    """u[node] = sum of all copies"""
    return np.bincount(ids.ravel(), weights=a.ravel(), minlength=n)


def broadcast(a, ids, n):
    """a with every copy of a torus node replaced by the sum of its copies"""
    return np.asfortranarray(node_sum(a, ids, n)[ids])


def stiffness(T, a_cell, ids, n, lam=0.0):
    """(lam M + K_a) of TextbookP1 T with the diagonal conductivity a_cell per cell, its nodes identified by ids: n x n CSR"""
    nv = T.elements.shape[1]
    ag = T.grad * a_cell[:, None, :]
    loc = np.einsum("kid,kjd->kij", ag, T.grad) * T.vol[:, None, None]
    loc = loc + lam * (np.ones((nv, nv)) + np.eye(nv))[None, :, :] * (T.vol / (nv * (nv + 1)))[:, None, None]
    el = ids[T.elements]
    rows = np.repeat(el, nv, axis=1).ravel()
    cols = np.tile(el, (1, nv)).ravel()
    return sp.csr_matrix((loc.ravel(), (rows, cols)), shape=(n, n))


class TorusSystem:
    """The torus problem on the explicitly refined disjoint simplices: K u = F_xi with the constants in K's kernel."""

    def __init__(self, O, mesh, cond, refinements):
        nodes, elements = disjoint(mesh)
        fine = O.refine_uniformly(O.Mesh(nodes, elements), times=refinements)
        self.m = 2 ** refinements
        self.T = TextbookP1(fine.nodes, fine.elements)
        per_cell = fine.elements.shape[0] // elements.shape[0]              # (children of a cell are consecutive)
        self.a = np.repeat(np.asarray(cond, dtype=np.float64), per_cell, axis=0)
        uniq, self.ids = np.unique(keys(fine.nodes, mesh.period, self.m), return_inverse=True)
        self.n = uniq.size
        self.uniq = uniq
        self.K = stiffness(self.T, self.a, self.ids, self.n)
        self.volume = float(self.T.vol.sum())

    def corrector(self, xi):
        """v with K v = -int sigma xi . grad phi, pinned to zero at node 0, then mean-free"""
        import scipy.sparse.linalg as spla
        F = np.bincount(self.ids, weights=self.T.load(self.a, xi), minlength=self.n)
        v = np.zeros(self.n)
        v[1:] = spla.spsolve(self.K[1:][:, 1:].tocsc(), F[1:])
        return v - v.mean()

    def energy(self, v, xi, eta=None, w=None):
        """int sigma grad(xi.x + v) . grad(eta.x + w) / |Omega|"""
        eta = xi if eta is None else eta
        w = v if w is None else w
        gu = np.einsum("kid,ki->kd", self.T.grad, v[self.ids][self.T.elements]) + np.asarray(xi)[None, :]
        gw = np.einsum("kid,ki->kd", self.T.grad, w[self.ids][self.T.elements]) + np.asarray(eta)[None, :]
        return float(np.sum(self.T.vol[:, None] * self.a * gu * gw) / self.volume)

    def gather(self, g, level, x):
        """nodal vector of a level vector (Nf, Ne) whose copies agree, in this system's numbering"""
        nodes, _ = vtk.construct_full_grid(g, level)
        k = keys(nodes, g.base.period, self.m)
        pos = np.searchsorted(self.uniq, k)
        assert np.array_equal(self.uniq[pos], k)
        u = np.zeros(self.n)
        u[pos] = np.asarray(x).T.ravel()
        return u
