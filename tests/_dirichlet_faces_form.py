"""Yardsticks for a constrained set given as a list of faces (hmg_grid_set_dirichlet_faces), none of which calls the library:

  closure()            the closure rule in numpy: per-cell entity bitmasks and the constrained base nodes
  oracle_constraint()  the oracle's ZeroDirichletConstraint for the set, from the oracle's own helpers
  oracle_base_level()  the oracle's BaseLevel on the set's interior nodes
  FaceSetForm          tests/_global_form.py's GlobalForm with `inner` masks from the set: a node of a refined mesh is
                       constrained iff it lies on a chosen face (geometry only -- no entity list takes part)

Faces are (nfaces, dim) arrays of 0-based node ids here (3D: triangles, 2D: edges), ascending within a face; `one_based` makes
what the library takes."""
import numpy as np

from _global_form import GlobalForm

TET_FACES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
TRI_EDGES = ((0, 1), (0, 2), (1, 2))


def one_based(faces):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int64) + 1)


def all_faces(elements):
    """every face (3D) / edge (2D) of the cells once, lexicographic, and the number of cells that contain it"""
    el = np.sort(np.asarray(elements, dtype=np.int64), axis=1)
    tuples = TET_FACES if el.shape[1] == 4 else TRI_EDGES
    f = np.concatenate([el[:, list(t)] for t in tuples])
    return np.unique(f, axis=0, return_counts=True)


def default_faces(elements):
    f, n = all_faces(elements)
    return f[n == 1]


def interior_faces(elements):
    f, n = all_faces(elements)
    return f[n == 2]


def plane_faces(nodes, elements, axis, value):
    f, _ = all_faces(elements)
    return f[np.all(np.abs(np.asarray(nodes)[f][:, :, axis] - value) <= 1e-12, axis=1)]


def sides(m, axis):
    x = m.nodes[:, axis]
    return np.concatenate([plane_faces(m.nodes, m.elements, axis, x.min()), plane_faces(m.nodes, m.elements, axis, x.max())])


def mid_plane_and_sides(m):
    """an internal plane normal to the first axis -- every face of it lies between two cells -- and the two outer sides normal to
    the last: most of the outer boundary is free"""
    lo, hi = m.nodes[:, 0].min(), m.nodes[:, 0].max()
    return np.concatenate([plane_faces(m.nodes, m.elements, 0, 0.5 * (lo + hi)), sides(m, m.dim - 1)])


def block_boundary_faces(nodes, elements, block):
    """faces on the planes x_a = min_a + j * block of every axis a (the outer boundary among them)"""
    nodes = np.asarray(nodes, dtype=np.float64)
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    out = [plane_faces(nodes, elements, a, v) for a in range(nodes.shape[1]) for v in np.arange(lo[a], hi[a] + 0.5, block)]
    return np.unique(np.concatenate(out), axis=0)


def closure(elements, faces, nnodes):
    """(dmask (Ne,) int, constrained (nnodes,) bool): bit order faces (3D only), edges, nodes -- a chosen face sets its bit in
    every cell that contains it, its edges and nodes theirs in every cell around them"""
    el = np.sort(np.asarray(elements, dtype=np.int64), axis=1)
    dim = el.shape[1] - 1
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, dim)
    fset = {tuple(f) for f in faces}
    eset = {(f[a], f[b]) for f in faces for a in range(dim) for b in range(a + 1, dim)} if dim == 3 else set(fset)
    nset = {int(v) for v in faces.reshape(-1)}
    face_t = TET_FACES if dim == 3 else ()
    edge_t = TET_EDGES if dim == 3 else TRI_EDGES
    dmask = np.zeros(el.shape[0], dtype=np.int64)
    for c, e in enumerate(el):
        bit = 0
        for t in face_t:
            dmask[c] |= (tuple(e[list(t)]) in fset) << bit
            bit += 1
        for t in edge_t:
            dmask[c] |= ((e[t[0]], e[t[1]]) in eset) << bit
            bit += 1
        for l in range(dim + 1):
            dmask[c] |= (int(e[l]) in nset) << bit
            bit += 1
    constrained = np.zeros(nnodes, dtype=bool)
    constrained[sorted(nset)] = True
    return dmask, constrained


def oracle_constraint(O, mesh, faces):
    """O.ZeroDirichletConstraint of the closure of `faces`, by the steps of O.list_boundary_nodes_edges_faces with the chosen
    faces in the place of the faces that occur once"""
    dim = mesh.dim
    faces = np.unique(np.asarray(faces, dtype=np.int64).reshape(-1, dim), axis=0)
    empty = O.compress(np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    bn = np.unique(faces.reshape(-1))[:, None]
    nodes = O.compress(*O._intersect(*O._sorted_list(mesh, [(i,) for i in range(dim + 1)]), bn))
    if dim == 3:
        be = np.unique(np.concatenate([faces[:, [0, 1]], faces[:, [0, 2]], faces[:, [1, 2]]]), axis=0)
        edges = O.compress(*O._intersect(*O._sorted_list(mesh, O.TET_EDGES), be))
        return O.ZeroDirichletConstraint(nodes, edges, O.compress(*O._intersect(*O._sorted_list(mesh, O.TET_FACES), faces)))
    return O.ZeroDirichletConstraint(nodes, O.compress(*O._intersect(*O._sorted_list(mesh, O.TRI_EDGES), faces)), empty)


def free_nodes(mesh, faces):
    con = np.zeros(mesh.nnodes(), dtype=bool)
    con[np.asarray(faces, dtype=np.int64).reshape(-1)] = True
    return np.flatnonzero(~con)


def oracle_base_level(O, mesh, sig, lam, faces):
    interior = free_nodes(mesh, faces)
    A = O.assemble_checkerboard(mesh, sig, lam).tocsr()[interior][:, interior]
    return O.BaseLevel.create(O._SpluSolver(A), mesh.nnodes(), interior)


def on_faces(points, nodes, faces):
    """which points lie on one of the faces (simplices of dim - 1 with their boundary): barycentric coordinates by least squares"""
    points, nodes = np.asarray(points, dtype=np.float64), np.asarray(nodes, dtype=np.float64)
    hit = np.zeros(points.shape[0], dtype=bool)
    for f in np.asarray(faces, dtype=np.int64):
        v0 = nodes[f[0]]
        E = (nodes[f[1:]] - v0).T                                        # dim x (dim - 1)
        lam, *_ = np.linalg.lstsq(E, (points - v0).T, rcond=None)
        res = np.abs(E @ lam - (points - v0).T).max(axis=0)
        hit |= (res <= 1e-10) & np.all(lam >= -1e-10, axis=0) & (lam.sum(axis=0) <= 1.0 + 1e-10)
    return hit


class FaceSetForm(GlobalForm):
    """GlobalForm whose constrained nodes, on every refined mesh, are those lying on a chosen face of the base mesh"""

    def __init__(self, O, base, sgrid, lam, implicit, grids, dim, faces, cond=None):
        super().__init__(O, base, sgrid, lam, implicit, grids, dim, cond=cond)
        self.inner = [~on_faces(m.nodes, base.nodes, faces) for m in self.meshes]
