"""The level-1 solve of the V-cycle (src/multigrid.jl:74-93) stated in numpy / scipy from the tables a grid exports -- none of
the library's kernels takes part:

    A        = (lambda M + K_sigma)[interior, interior]      coarse_rowptr / coarse_colidx / coarse_val
               (tests/test_host_tables.py::test_coarse_matrix holds it against the textbook matrix)
    u[node]  = sum of all copies of b1 at that node
    x        = A^-1 u[interior]                              scipy.sparse.linalg.splu, float64
    x1[:, c] = the nodal vector (x on interior nodes, 0 on constrained ones) at cell c's nodes

Cells are 0-based (ncells, dim + 1) arrays in the node order the grid was built with; a level-1 matrix is (dim + 1, ncells).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


# The base meshes of tests/test_coarse_solve_host.py (premises, CPU) and tests/test_gpu_coarse_solve.py (device):
#   name -> (kind, dim, arguments), n = number of unknowns, longest row of the level-1 matrix
MESHES = {
    "sq1": ("cube", 2, 1), "sq2": ("cube", 2, 2), "sq3": ("cube", 2, 3), "sq4": ("cube", 2, 4), "sq16": ("cube", 2, 16),
    "sq514": ("cube", 2, 514),
    "cu2": ("cube", 3, 2), "cu3": ("cube", 3, 3), "cu4": ("cube", 3, 4), "cu6": ("cube", 3, 6),
    "del2_18": ("delaunay", 2, 18, 3), "del2_19": ("delaunay", 2, 19, 3), "del2_20": ("delaunay", 2, 20, 3),
    "del2_21": ("delaunay", 2, 21, 3),
    "del3_60": ("delaunay", 3, 60, 103),       # the mesh of tests/test_gpu_parity.py::test_unstructured_delaunay_mesh
    "del3_120": ("delaunay", 3, 120, 103),
    "fan2": ("fan", 2, 50, 24, 1), "fan3": ("fan", 3, 40, 60, 4),
}
UNKNOWNS = {"sq1": 0, "sq2": 1, "sq3": 4, "sq4": 9, "sq16": 225, "sq514": 263169, "cu2": 1, "cu3": 8, "cu4": 27, "cu6": 125,
            "del2_18": 11, "del2_19": 12, "del2_20": 13, "del2_21": 14, "del3_60": 38, "del3_120": 90, "fan2": 51, "fan3": 41}
LATTICES = [k for k, v in MESHES.items() if v[0] == "cube"]


def mesh(O, name):
    import _meshes
    kind, dim, *args = MESHES[name]
    if kind == "cube":
        return O.hypercube(dim, *args)
    return (_meshes.delaunay_mesh if kind == "delaunay" else _meshes.fan_mesh)(O, dim, *args)


def two_valued(m, seed, values=(1.0, 9.0)):
    """one of two conductivities per cell and direction, as the checkerboard drivers draw them"""
    return np.random.default_rng(seed).choice(list(values), size=(m.nelements(), m.dim))


def matrix(g):
    """(A, interior) of the grid's current level-1 system (after coarse_setup)."""
    interior = g.interior_nodes().astype(np.int64)
    n = interior.size
    rowptr, colidx, val = g.table_i32("coarse_rowptr"), g.table_i32("coarse_colidx"), g.table_f64("coarse_val")
    if n == 0:
        return sp.csr_matrix((0, 0)), interior
    assert rowptr.size == n + 1 and rowptr[0] == 0 and rowptr[-1] == colidx.size == val.size
    return sp.csr_matrix((val, colidx, rowptr), shape=(n, n)), interior


def row_lengths(A):
    return np.diff(A.indptr)


def node_sum(cells, nnodes, b1):
    """u[node] = sum of all copies of b1 at that node"""
    u = np.zeros(nnodes)
    np.add.at(u, cells.T, b1)
    return u


def distribute(cells, u):
    """x1[:, c] = u at cell c's nodes"""
    return np.asfortranarray(u[cells.T])


def broadcast(cells, nnodes, b1):
    """b1 with every copy of a node replaced by the sum of its copies (what the solve leaves in b1)"""
    return distribute(cells, node_sum(cells, nnodes, b1))


def gather(cells, nnodes, x1):
    """The nodal vector of a level-1 matrix whose copies agree (first copy wins; callers check that they agree)."""
    u = np.zeros(nnodes)
    u[cells.T[::-1].ravel()] = x1[::-1].ravel()
    return u


class Direct:
    """splu of A, once per matrix"""

    def __init__(self, A, interior, cells, nnodes):
        self.A, self.interior, self.cells, self.nnodes = A.tocsr(), interior, cells, nnodes
        self.n = interior.size
        self.lu = spla.splu(self.A.tocsc()) if self.n else None

    def rhs(self, b1):
        return node_sum(self.cells, self.nnodes, b1)[self.interior]

    def solve_interior(self, b1):
        return self.lu.solve(self.rhs(b1)) if self.n else np.zeros(0)

    def nodal(self, x):
        u = np.zeros(self.nnodes)
        u[self.interior] = x
        return u

    def solve(self, b1):
        return distribute(self.cells, self.nodal(self.solve_interior(b1)))

    def interior_of(self, x1):
        return gather(self.cells, self.nnodes, x1)[self.interior]

    def residual(self, b1, x):
        """|| u_I - A x ||_2 / || u_I ||_2 of a candidate x (interior values), accumulated in long double"""
        return true_residual(self.A, self.rhs(b1), x)


def true_residual(A, u, x):
    A = A.tocsr()
    xl, ul = np.asarray(x, dtype=np.longdouble), np.asarray(u, dtype=np.longdouble)
    prod = A.data.astype(np.longdouble) * xl[A.indices]
    Ax = np.zeros(A.shape[0], dtype=np.longdouble)
    np.add.at(Ax, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), prod)
    r = ul - Ax
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(ul * ul)))


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def jacobi_cg(A, u, rtol=1e-13, maxiter=20000):
    """float64 Jacobi-preconditioned scipy CG to a relative recurrence residual of rtol: the yardstick of what a CG of this
    precision reaches on this matrix.  Returns (x, iterations)."""
    d = A.diagonal()
    M = spla.LinearOperator(A.shape, matvec=lambda v: v / d, dtype=np.float64)
    it = [0]

    def count(_):
        it[0] += 1

    x, info = spla.cg(A, u, rtol=rtol, atol=0.0, maxiter=maxiter, M=M, callback=count)
    assert info == 0, info
    return x, it[0]
