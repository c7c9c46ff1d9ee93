"""The statement behind sampling on a periodic grid (hmg_grid_set_periodic_sampling), in numpy, sharing no code with the library.

`TorusFineMesh` is `_sample_form.FineMesh` with the coarse corners taken from `Mesh.cell_corners()` -- the unwrapped corners, the
ones `vtk.construct_full_grid` places the fine nodes on --, so a cell that wraps comes out in one piece, possibly past the far
side of the box, and interior points by construction may lie outside the box.  What makes it a torus is said by POSITION
(`_periodic_form.keys`, `fine_ids`): two nodes are the same node iff their positions agree modulo the period.  The meshes are
`_periodic_form.general_torus` (jitter, stretch (2, 1/2, 1), optionally representatives moved by whole periods): every number is
a dyadic rational, positions are multiples of 1 / (16 m), so the keys and whole-period shifts are exact.

Tolerances are `_sample_form`'s formulas (T_w, T_value, T_gradient) with X the largest absolute value among the unwrapped corners,
the period and the query points as given (`scope`): a point three periods away carries the rounding of its own size.

`brute_force_cells` is the search the locator's lists are held to: every cell, the minimal image of x - X0, barycentric
coordinates in extended precision; it also returns the smallest |barycentric coordinate| met, so that a test can require its
points to stay away from every face.
"""
import copy

import numpy as np

from homogenization_jl_amd import vtk

import _periodic_form as P
import _sample_form as F

EPS = F.EPS
CASES = {"torus2": ((4, 3), 5, (1, 3, 5)), "torus3": ((3, 3, 3), 3, (1, 3))}      # name -> shape, levels of the grid, levels tested
SEED = {"torus2": 21, "torus3": 22}


def mesh(name, shift=False):
    return P.general_torus(CASES[name][0], SEED[name], shift=shift)


class TorusFineMesh(F.FineMesh):
    """Explicit fine mesh of one level of a periodic grid, on the unwrapped corners of its cells.  explicit = False (the largest
    levels: 42 million fine elements on 3D level 7) leaves the element list unformed: the fine nodes come from
    construct_full_grid's own formula, the elements of `interior_points` from the reference cell's list."""

    def __init__(self, implicit, level, explicit=True):
        self.level = level
        self.dim = d = implicit.base.dim
        self.m = 2 ** (level - 1)
        self.nf = implicit.nf(level)
        self.ne = implicit.ncells()
        self.period = np.asarray(implicit.base.period, dtype=np.float64)
        Xc = np.asarray(implicit.base.cell_corners(), dtype=np.float64)[:self.ne]       # (ne, d + 1, d), unwrapped
        self.Xc = Xc
        h2s = implicit.table_i32("hier2slot", level)
        self.ref = implicit.table_i32("slot_ijk", level).reshape(-1, 3)[h2s][:, :d].astype(np.float64) / self.m
        self.ref_cells = implicit.table_i32("ref_cells", level).reshape(-1, d + 1).astype(np.int64)
        self.nel = self.ref_cells.shape[0]
        if explicit:
            self.nodes, self.cells = vtk.construct_full_grid(implicit, level)
        else:
            self.nodes = (Xc[:, :1, :] + np.einsum("na,eac->enc", self.ref, Xc[:, 1:, :] - Xc[:, :1, :])).reshape(-1, d)
            self.cells = None
        self.coarse_grads = F.p1_gradients(Xc)
        self.h_min = float((1.0 / np.linalg.norm(self.coarse_grads, axis=2)).min())
        self.h_max = float(np.max(np.linalg.norm(Xc[:, :, None, :] - Xc[:, None, :, :], axis=3))) / self.m
        self.X = max(float(np.abs(Xc).max()), float(self.period.max()))
        self.elements = np.asarray(implicit.base.elements, dtype=np.int64)[:self.ne]    # torus node ids, 1-based

    def scope(self, x):
        """this mesh with X grown to the query points as given: the tolerances of a call that takes them"""
        fm = copy.copy(self)
        fm.X = max(self.X, float(np.abs(x[np.isfinite(x)]).max()))
        return fm

    def interior_points(self, n, seed):
        if self.cells is not None:
            return super().interior_points(n, seed)
        rng = np.random.default_rng(seed)
        d = self.dim
        cell = rng.integers(0, self.ne, size=n)
        elem = rng.integers(0, self.nel, size=n)
        lam = rng.random((n, d + 1)) + 1e-3
        lam = F.MARGIN + (1.0 - (d + 1) * F.MARGIN) * lam / lam.sum(axis=1, keepdims=True)
        hier = self.ref_cells[elem]
        Xv = self.nodes[hier + (cell * self.nf)[:, None]]
        Xe = self.vertices_extended(cell, hier)
        assert float(np.abs(Xe - Xv).max()) <= 16.0 * EPS * self.X
        return {"x": np.ascontiguousarray(np.einsum("nk,nkc->nc", lam, Xv)), "cell": cell.astype(np.int32),
                "nodes": hier.astype(np.int32), "weights": lam, "grads": F.p1_gradients(Xe)}

    def fine_ids(self):
        """(ids (nf, ne), n): `_periodic_form.fine_ids` from this mesh's node positions"""
        uniq, inv = np.unique(self.node_keys(), return_inverse=True)
        n = int(np.unique(self.elements).size) * self.m ** self.dim
        assert uniq.size == n, (uniq.size, n)
        return inv.reshape(self.ne, self.nf).T, n

    def node_keys(self):
        return P.keys(self.nodes, self.period, self.m, P.DEN)

    def node_points(self):
        """Every fine node position (one per coarse-cell copy, unwrapped) and the lowest coarse cell that has a node at that
        position modulo the period."""
        _, inv = np.unique(self.node_keys(), return_inverse=True)
        inv = inv.ravel()
        owner = np.repeat(np.arange(self.ne), self.nf)
        lowest = np.full(inv.max() + 1, self.ne, dtype=np.int64)
        np.minimum.at(lowest, inv, owner)
        return self.nodes, lowest[inv].astype(np.int32)

    def coarse_face_points(self, per_face, seed):
        """Random points inside the faces of the coarse cells, from every cell's own unwrapped copy of the face -- across the seam
        the two copies of a face are whole periods apart --, and the lower id of the two cells that share the face (on a torus
        every face has two; a face is its set of torus nodes)."""
        rng = np.random.default_rng(seed)
        d = self.dim
        faces = {}
        for c in range(self.ne):
            for skip in range(d + 1):
                faces.setdefault(tuple(sorted(np.delete(self.elements[c], skip))), []).append(c)
        assert all(len(v) == 2 for v in faces.values())
        pts, want = [], []
        for skip in range(d + 1):
            Fc = np.delete(self.Xc, skip, axis=1)                                   # (ne, d, d)
            lam = rng.random((self.ne, per_face, d)) + 0.05
            lam /= lam.sum(axis=2, keepdims=True)
            pts.append(np.einsum("epk,ekc->epc", lam, Fc).reshape(-1, d))
            low = np.array([min(faces[tuple(sorted(np.delete(self.elements[c], skip)))]) for c in range(self.ne)])
            want.append(np.repeat(low, per_face))
        return np.ascontiguousarray(np.concatenate(pts)), np.concatenate(want).astype(np.int32)

    def brute_force_cells(self, x, chunk=5000):
        """(cell, margin): the lowest cell whose barycentric coordinates of the minimal image of x - X0 are all >= 0, by a search
        over all cells, and the smallest |barycentric coordinate| of any point in any cell."""
        X0 = self.Xc[:, 0, :].astype(np.longdouble)                                 # (ne, d)
        G = self.coarse_grads[:, 1:, :].astype(np.longdouble)                       # (ne, d, d): rows g_1 .. g_d
        per = self.period.astype(np.longdouble)
        cell = np.full(x.shape[0], -1, dtype=np.int32)
        margin = np.inf
        for s in range(0, x.shape[0], chunk):
            dx = x[s:s + chunk, None, :].astype(np.longdouble) - X0[None, :, :]     # (n, ne, d)
            dx -= per * np.rint(dx / per)
            lam = np.einsum("ekc,nec->nek", G, dx)
            lam = np.concatenate([1.0 - lam.sum(axis=2, keepdims=True), lam], axis=2)
            margin = min(margin, float(np.abs(lam).min()))
            inside = (lam >= 0).all(axis=2)
            assert inside.any(axis=1).all()                                         # the torus has no outside
            cell[s:s + chunk] = inside.argmax(axis=1)
        return cell, margin

    def nodal_vector(self, seed):
        """An (nf, ne) host matrix laid out by position: one independent normal value per torus fine node, so the copies agree."""
        ids, n = self.fine_ids()
        return np.asfortranarray(np.random.default_rng(seed).standard_normal(n)[ids])


def quantized(x, bits=40):
    """x rounded to multiples of 2^-bits: adding a whole number of (dyadic) periods to such a point is exact"""
    return np.round(x * 2.0 ** bits) / 2.0 ** bits


def whole_period_shifts(x, period, seed, reach=3):
    """x (quantized) moved by a random whole number of periods in [-reach, reach] per point and axis, exactly"""
    k = np.random.default_rng(seed).integers(-reach, reach + 1, size=x.shape).astype(np.float64)
    xs = x + k * period
    assert np.array_equal(xs - k * period, x)
    return np.ascontiguousarray(xs)


# ---- an ordinary grid's locate, as the commit before this feature answered it (tests/golden/ordinary_locate_parent.npz) ----------
def ordinary_locate(name):
    """the points and hmg_grid_locate's four arrays on an ordinary grid of tests/_periodic_golden.py, level 3"""
    import homogenization_jl_amd as hmg
    from _periodic_golden import ordinary_mesh
    m, _ = ordinary_mesh(name)
    g = hmg.ImplicitFineGrid(None, m, 3)
    try:
        lo, hi = m.nodes.min(axis=0), m.nodes.max(axis=0)
        x = lo - 0.05 + np.random.default_rng(31).random((400, m.dim)) * (hi - lo + 0.1)      # some outside
        x = np.ascontiguousarray(np.concatenate([x, m.nodes]))                              # ... and every coarse node: ties
        cell, nodes, w, gw = hmg.locate(g, 3, x)
        return {"x": x, "cell": cell, "nodes": nodes, "weights": w, "gweights": gw}
    finally:
        g.close()
