"""Grids on a torus, host side (hmg_grid_create_periodic with a NULL context, hmg_periodic_mesh, hmg_grid_set_mean_free): the
topology the existing table builder derives from torus node ids, the geometry through the minimal-image rule, the level-1 matrix
with the constants in its kernel, every refusal with its message -- and that an ordinary grid keeps the bits it had.
The statements are those of tests/_periodic_form.py: the torus as disjoint simplices, nodes identified by position."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

import _coarse_form as CF
import _tensor_sigma_form as TS
from _periodic_form import DEN, TorusSystem, coarse_ids, disjoint, general_torus, keys, stiffness
from _periodic_golden import ordinary_mesh, ordinary_tables
from _textbook_fem import TextbookP1

SHAPES = [(3, 3), (4, 3), (3, 3, 3), (3, 4, 5)]
TET_FACES = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
TRI_EDGES = [(0, 1), (0, 2), (1, 2)]


def torus(shape):
    return driver.periodic_mesh(hmg.Tet64 if len(shape) == 3 else hmg.Tri64, shape)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    mesh = torus(request.param)
    g = hmg.ImplicitFineGrid(None, mesh, 2)
    yield request.param, mesh, g
    g.close()


def test_the_synthesiser(case):
    """node ids with the last coordinate fastest, modulo shape; tuples ascending; cube q owns its cells in the checkerboard
    synthesiser's order: the unwrapped cells are those of the box of the same shape, translated"""
    shape, mesh, _ = case
    d = len(shape)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, d)
    np.testing.assert_array_equal(mesh.nodes, idx.astype(np.float64))
    np.testing.assert_array_equal(mesh.period, np.asarray(shape, dtype=np.float64))
    assert np.all(np.diff(mesh.elements, axis=1) > 0) and mesh.elements.min() == 1 and mesh.elements.max() == len(idx)
    box = driver.checkerboard_mesh(hmg.Tet64 if d == 3 else hmg.Tri64, shape, origin=np.zeros(d), transposed_lookup=False, ordered=False)
    per = 6 if d == 3 else 2
    assert mesh.elements.shape == box.elements.shape == (per * len(idx), d + 1)
    X, B = mesh.cell_corners(), box.nodes[box.elements - 1]
    # the same point set cell by cell (the tuple order differs where a cube wraps), up to whole periods
    shift = X.min(axis=1) - B.min(axis=1)
    assert np.array_equal(np.mod(shift, np.asarray(shape)), np.zeros_like(shift))
    rows = lambda P: np.sort(np.ascontiguousarray(P).view([("", float)] * d).reshape(len(P), d + 1), axis=1)
    assert np.array_equal(rows(X - shift[:, None, :]), rows(B))
    np.testing.assert_array_equal(hmg.fields.cell_volumes(mesh), hmg.fields.cell_volumes(box))


def test_topology(case):
    shape, mesh, g = case
    d, el = len(shape), mesh.elements - 1
    nface, nedge = (4, 6) if d == 3 else (0, 3)
    assert not g.table_i32("dmask").any()
    assert g.dirichlet_faces().shape == (0, d)
    assert g.interior_nodes().size == mesh.nodes.shape[0]
    mult = g.table_i32("mult").reshape(-1, 16)
    edges = np.unique(np.concatenate([el[:, list(e)] for e in (TET_EDGES if d == 3 else TRI_EDGES)]), axis=0)
    if d == 3:
        assert np.all(mult[:, :nface] == 2)
        assert g.table_i32("face_pairs").size // 3 == 2 * el.shape[0]
        faces = np.unique(np.concatenate([el[:, list(f)] for f in TET_FACES]), axis=0)
        assert mesh.nodes.shape[0] - len(edges) + len(faces) - el.shape[0] == 0
    else:
        assert np.all(mult[:, :nedge] == 2)                               # (2D: the edges are the faces)
        assert mesh.nodes.shape[0] - len(edges) + el.shape[0] == 0
    assert np.all(mult[:, nface + nedge:nface + nedge + d + 1] == (24 if d == 3 else 6))
    assert np.all(np.bincount(el.ravel()) == (24 if d == 3 else 6))


def ordinary_twin(mesh):
    nodes, elements = disjoint(mesh)
    return hmg.Mesh(nodes, elements + 1)


def test_geometry_is_that_of_the_disjoint_simplices_bit_for_bit(case):
    """detj and jinv reach the tables as the coefficient rows |J| J^-1 sigma J^-T, |J|: with sigma = 1, and with a sigma that
    separates the entries of J^-1, they are the bits of an ordinary grid made of the same cells as disjoint simplices"""
    shape, mesh, g = case
    twin = hmg.ImplicitFineGrid(None, ordinary_twin(mesh), 2)
    rng = np.random.default_rng(1)
    for sig in (np.ones((mesh.elements.shape[0], mesh.dim)), rng.choice([1.0, 9.0], size=(mesh.elements.shape[0], mesh.dim)),
                rng.random((mesh.elements.shape[0], mesh.dim)) + 0.5):
        g.set_operator(sig, 0.0)
        twin.set_operator(sig, 0.0)
        a, b = g.table_f64("coef"), twin.table_f64("coef")
        assert a.size == 8 * mesh.elements.shape[0] and np.array_equal(a.view(np.int64), b.view(np.int64))
    twin.close()


@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_level_1_matrix(case, lam):
    """the exported matrix against a scipy assembly from TextbookP1 on the disjoint simplices, nodes identified by position"""
    shape, mesh, g = case
    rng = np.random.default_rng(2)
    sig = rng.choice([1.0, 9.0], size=(mesh.elements.shape[0], mesh.dim))
    g.set_operator(sig, lam)
    g.coarse_setup()
    A, interior = CF.matrix(g)
    n = mesh.nodes.shape[0]
    np.testing.assert_array_equal(interior, np.arange(n))
    ids = coarse_ids(mesh)
    np.testing.assert_array_equal(ids, (mesh.elements - 1).ravel())       # (position says what the connectivity says)
    nodes, elements = disjoint(mesh)
    want = stiffness(TextbookP1(nodes, elements), sig, ids, n, lam).toarray()
    got = A.toarray()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())
    assert np.array_equal(got, got.T)
    if lam == 0.0:
        assert np.abs(got.sum(axis=1)).max() <= 1e-13 * np.abs(got).max()


def test_mean_free_defaults_and_the_singular_matrix():
    mesh = torus((3, 3))
    g = hmg.ImplicitFineGrid(None, mesh, 2)
    assert g.mean_free() is True
    g.set_operator(np.ones((18, 2)), 0.0)
    g.coarse_setup()                                                     # assembled, not refused
    g.set_mean_free(False)
    assert g.mean_free() is False
    with pytest.raises(HmgError, match="no node is constrained"):
        g.coarse_setup()
    g.set_lambda(0.5)
    g.coarse_setup()                                                     # regular: the flag does not matter
    g.close()
    base = driver.hypercube(hmg.Tri64, 3)
    o = hmg.ImplicitFineGrid(None, base, 2)
    assert o.mean_free() is False
    o.set_operator(np.ones((base.elements.shape[0], 2)), 0.0)
    o.set_dirichlet_faces(np.zeros((0, 2), dtype=np.int64))
    with pytest.raises(HmgError, match="no node is constrained"):
        o.coarse_setup()
    o.set_mean_free(True)
    o.coarse_setup()                                                     # the natural-boundary problem, on the complement of the constants
    A, _ = CF.matrix(o)
    assert np.abs(A.toarray().sum(axis=1)).max() <= 1e-13 * np.abs(A.toarray()).max()
    o.close()


def expected_dmask(mesh, faces):
    """the closure rule: a chosen face sets its bit in the cells that contain it, its edges / nodes theirs in every cell around"""
    d, el = mesh.dim, mesh.elements
    fs = {tuple(f) for f in faces}
    es = {tuple(sorted((f[i], f[j]))) for f in faces for i in range(d) for j in range(i + 1, d)}
    ns = {int(v) for f in faces for v in f}
    out = np.zeros(el.shape[0], dtype=np.int64)
    nface, edges = (4, TET_EDGES) if d == 3 else (0, TRI_EDGES)
    for c, t in enumerate(el):
        m = 0
        if d == 3:
            for l, f in enumerate(TET_FACES):
                m |= (tuple(t[list(f)]) in fs) << l
        for l, e in enumerate(edges):
            m |= (tuple(t[list(e)]) in es) << (nface + l)
        for l in range(d + 1):
            m |= (int(t[l]) in ns) << (nface + len(edges) + l)
        out[c] = m
    return out


def test_a_plane_of_fixed_potential_inside_the_torus(case):
    shape, mesh, g = case
    faces = driver.faces_on_plane(mesh, 0, 1.0)
    assert faces.shape[0] == int(np.prod(shape[1:])) * (2 if mesh.dim == 3 else 1)
    g.set_dirichlet_faces(faces)
    np.testing.assert_array_equal(g.dirichlet_faces(), faces)
    np.testing.assert_array_equal(g.table_i32("dmask"), expected_dmask(mesh, faces))
    on = np.flatnonzero(mesh.nodes[:, 0] == 1.0)
    np.testing.assert_array_equal(np.setdiff1d(np.arange(mesh.nodes.shape[0]), g.interior_nodes()), on)
    g.set_operator(np.ones((mesh.elements.shape[0], mesh.dim)), 0.0)
    g.coarse_setup()                                                     # regular
    g.set_dirichlet_faces(None)                                          # the default set of a torus is the empty set
    assert not g.table_i32("dmask").any() and g.dirichlet_faces().shape[0] == 0


def raises_creating(mesh, match):
    with pytest.raises(HmgError, match=match):
        hmg.ImplicitFineGrid(None, mesh, 2)


def test_refusals_at_creation():
    m = torus((3, 3))
    for bad in (0.0, -3.0, np.inf, np.nan):
        raises_creating(hmg.Mesh(m.nodes, m.elements, np.array([3.0, bad])), "period of axis 1 must be positive and finite")
    with pytest.raises(ValueError, match="one entry per axis"):
        hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements, np.array([3.0])), 2)
    # two cubes per axis: every edge spans half the period -- the synthesiser refuses, and so does the grid for a mesh made by hand
    with pytest.raises(HmgError, match="at least 3 cubes"):
        torus((3, 2))
    idx = np.stack(np.meshgrid(np.arange(2), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 2)
    node = lambda i, j: (i % 2) * 2 + (j % 2) + 1
    cells = []
    for i, j in idx:
        c = [node(i, j), node(i + 1, j), node(i, j + 1), node(i + 1, j + 1)]
        cells += [sorted(c[:3]), sorted(c[1:])]
    raises_creating(hmg.Mesh(idx.astype(float), np.array(cells), np.array([2.0, 2.0])), r"cell 0 has an edge that spans half the period")
    # a cell stretched over half the box of a 4 x 3 torus
    m43 = torus((4, 3))
    el = m43.elements.copy()
    el[5] = np.sort([el[5][0], (el[5][0] - 1 + 2 * 3) % 12 + 1, el[5][2]])   # a node two cubes away along the first axis
    assert len(set(el[5])) == 3
    raises_creating(hmg.Mesh(m43.nodes, el, m43.period), r"cell 5 has an edge that spans half the period of axis 0")
    # a face shared by three cells: one more copy of a cell
    el = np.concatenate([m.elements, m.elements[7:8]])
    raises_creating(hmg.Mesh(m.nodes, el, m.period), r"shared by more than two triangles \(cell 18\)")
    m3 = torus((3, 3, 3))
    el = np.concatenate([m3.elements, m3.elements[7:8]])
    raises_creating(hmg.Mesh(m3.nodes, el, m3.period), r"a face is shared by more than two cells \(cell 162\)")
    # a degenerate cell: three nodes in a row
    m44 = torus((5, 5))
    nodes = m44.nodes.copy()
    nodes[6] = [1.0, 2.0]                                                # node (1, 1) onto (1, 2)'s place: cells with both collapse
    collapsed = np.flatnonzero(hmg.fields.cell_volumes(hmg.Mesh(nodes, m44.elements, m44.period)) == 0.0)
    assert collapsed.size > 0
    with pytest.raises(HmgError, match=rf"degenerate cell {collapsed[0]}$"):
        hmg.ImplicitFineGrid(None, hmg.Mesh(nodes, m44.elements, m44.period), 2)
    with pytest.raises(HmgError, match="strictly ascending"):
        hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements[:, ::-1].copy(), m.period), 2)


def test_refusals_on_a_periodic_grid(case):
    shape, mesh, g = case
    with pytest.raises(HmgError, match="hmg_grid_shrink: a periodic grid"):
        g.shrink(2, mesh.nodes.shape[0])
    with pytest.raises(HmgError, match="hmg_grid_locate: periodic grids"):
        hmg.locate(g, 1, np.zeros((1, mesh.dim)) + 0.25)


def test_an_ordinary_grid_keeps_its_bits():
    """period = 0 through the helper: two builds agree, and the tables are those the commit before periodic grids built
    (tests/golden/ordinary_tables_parent.npz, recorded with tests/_periodic_golden.py)"""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordinary_tables_parent.npz"))
    for name in ("tri", "tet"):
        a, b = ordinary_tables(name), ordinary_tables(name)
        for k, v in a.items():
            assert np.array_equal(v, b[k]), (name, k)
            w = gold[f"{name}_{k}"]
            assert v.dtype == w.dtype and np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v,
                                                         w.view(np.int64) if w.dtype == np.float64 else w), (name, k)
    mesh, _ = ordinary_mesh("tri")
    assert mesh.period is None and np.array_equal(mesh.cell_corners(), mesh.nodes[mesh.elements - 1])


def test_vtu_writers_duplicate_the_corners_of_a_torus(tmp_path):
    mesh = torus((3, 3))
    path = hmg.vtk.export_cell_fields(mesh, {"q": np.arange(18.0)}, str(tmp_path / "t"))
    f = hmg.vtk.read_vtu(path)
    assert f["points"].shape == (54, 3) and np.array_equal(f["connectivity"], np.arange(54))
    pts = f["points"][:, :2].reshape(18, 3, 2)
    assert np.ptp(pts, axis=1).max() == 1.0                              # no cell is drawn across the box
    np.testing.assert_array_equal(pts, mesh.cell_corners())
    box = driver.hypercube(hmg.Tri64, 3)
    g = hmg.vtk.read_vtu(hmg.vtk.export_cell_fields(box, {"q": np.arange(18.0)}, str(tmp_path / "b")))
    assert g["points"].shape[0] == box.nodes.shape[0]                    # an ordinary mesh is written as before


def test_element_points_on_a_torus():
    """fields.element_points goes through the unwrapped corners: on level 2 the six nodes of every triangle are its three corners
    and the midpoints of its edges, in one piece (no coordinate differs by more than one cube), and at the torus positions of the
    cell's nodes modulo the period"""
    mesh = torus((4, 3))
    g = hmg.ImplicitFineGrid(None, mesh, 2)
    ne = mesh.elements.shape[0]
    cells = np.repeat(np.arange(ne), 2)
    nodes = np.tile(np.array([[0, 1, 2], [3, 4, 5]]), (ne, 1))
    P = hmg.fields.element_points(g, 2, cells, nodes).reshape(ne, 6, 2)
    X = P[:, :3]
    assert np.ptp(P, axis=1).max() == 1.0
    np.testing.assert_array_equal(np.mod(X, mesh.period), mesh.nodes[mesh.elements - 1])
    mids = np.stack([0.5 * (X[:, a] + X[:, b]) for a, b in TRI_EDGES], axis=1)
    rows = lambda Q: np.sort(np.ascontiguousarray(Q).view([("", float)] * 2).reshape(len(Q), 3), axis=1)
    assert np.array_equal(rows(P[:, 3:]), rows(mids))
    wraps = np.ptp(mesh.nodes[mesh.elements - 1], axis=1).max(axis=1) > 1.0
    assert wraps.any() and (np.abs(hmg.fields.element_centroids(g, 2, cells, nodes).reshape(ne, 2, 2).mean(axis=1)
                                   - X.mean(axis=1)) <= 1e-15).all()
    g.close()


# ---- general tori: moved, stretched and re-represented nodes (tests/_periodic_form.py: general_torus) ---------------------------
def _rot90(dim, axis=0):
    """a rotation by 90 degrees: in 2D of the plane, in 3D about `axis` -- a signed permutation, so a box stays a box"""
    Q = np.zeros((dim, dim))
    if dim == 2:
        Q[0, 1], Q[1, 0] = -1.0, 1.0
        return Q
    a, b = [k for k in range(3) if k != axis]
    Q[axis, axis], Q[a, b], Q[b, a] = 1.0, -1.0, 1.0
    return Q


@pytest.mark.parametrize("shape,refinements", [((4, 3), 2), ((3, 3, 3), 1)], ids=["4x3", "3x3x3"])
def test_the_extended_statement(oracle, shape, refinements):
    """general_torus without jitter or stretch is driver.periodic_mesh, and TorusSystem on it the matrix it was, bit for bit; the
    count of distinct fine positions of a moved and stretched torus is shape m^d; the full-tensor K is symmetric with the
    constants -- and nothing else -- in its kernel; and for sigma = Q D Q^T with one Q in every cell it is the diagonal
    statement on the mesh x -> Q^T x (the pattern of tests/test_tensor_sigma_statement.py), at 1e-13"""
    d = len(shape)
    plain = general_torus(shape, 3, jitter=False, scale=(1.0, 1.0, 1.0))
    old = torus(shape)
    assert np.array_equal(plain.nodes, old.nodes) and np.array_equal(plain.elements, old.elements) and np.array_equal(plain.period, old.period)
    rng = np.random.default_rng(5)
    ne = old.elements.shape[0]
    D = rng.choice([1.0, 9.0], size=(ne, d))
    a, b = TorusSystem(oracle, old, D, refinements), TorusSystem(oracle, plain, D, refinements, den=DEN)
    assert a.n == b.n and np.array_equal(a.ids, b.ids)
    A, B = a.K.tocsr(), b.K.tocsr()
    A.sum_duplicates(), B.sum_duplicates()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert np.array_equal(A.data.view(np.int64), B.data.view(np.int64))
    assert np.array_equal(a.corrector(np.eye(d)[0]).view(np.int64), b.corrector(np.eye(d)[0]).view(np.int64))

    mesh = general_torus(shape, 3)
    sig = TS.random_spd(rng, ne, d)
    full = TorusSystem(oracle, mesh, sig, refinements, den=DEN)
    assert full.n == int(np.prod(shape)) * full.m ** d
    K = full.K.toarray()
    assert np.abs(K - K.T).max() <= 1e-13 * np.abs(K).max()
    assert np.abs(K.sum(axis=1)).max() <= 1e-13 * np.abs(K).max()
    w = np.linalg.eigvalsh(0.5 * (K + K.T))
    assert abs(w[0]) <= 1e-12 * w[-1] and w[1] > 1e-6 * w[-1]
    # the load of full tensors against the diagonal one where both exist
    diag = TorusSystem(oracle, mesh, D, refinements, den=DEN)
    as_full = TorusSystem(oracle, mesh, D[:, :, None] * np.eye(d)[None], refinements, den=DEN)
    xi = rng.standard_normal(d)
    F = np.bincount(diag.ids, weights=diag.T.load(diag.a, xi), minlength=diag.n)
    np.testing.assert_allclose(as_full.load(xi), F, rtol=0, atol=1e-13 * np.abs(F).max())
    np.testing.assert_allclose(as_full.K.toarray(), diag.K.toarray(), rtol=0, atol=1e-13 * np.abs(K).max())

    for axis in range(d if d == 3 else 1):
        Q = _rot90(d, axis)
        rot = hmg.Mesh(np.ascontiguousarray(mesh.nodes @ Q), mesh.elements.copy(), np.abs(mesh.period @ Q))
        want = TorusSystem(oracle, rot, D, refinements, lam=0.7, den=DEN)
        got = TorusSystem(oracle, mesh, np.einsum("ij,cj,kj->cik", Q, D, Q), refinements, lam=0.7, den=DEN)
        at = want.index(np.mod(got.pos @ Q, want.period))
        assert np.array_equal(np.sort(at), np.arange(want.n))
        W = want.K.toarray()[at][:, at]
        err = np.abs(got.K.toarray() - W).max() / np.abs(W).max()
        v, vw = got.corrector(xi), want.corrector(Q.T @ xi)
        e_v = np.abs(v - vw[at]).max() / np.abs(vw).max()
        e_e = abs(got.energy(v, xi) - want.energy(vw, Q.T @ xi)) / abs(want.energy(vw, Q.T @ xi))
        print(f"{shape}, rotation about axis {axis}: K {err:.2e}  corrector {e_v:.2e}  energy {e_e:.2e}")
        assert err <= 1e-13 and e_e <= 1e-13 and e_v <= 1e-11            # (the corrector passes through a solve: kappa eps)


GENERAL = [dict(jitter=False, scale=(1.0, 1.0, 1.0)), dict()]


def _host_tables(mesh, sig, lam=0.0):
    g = hmg.ImplicitFineGrid(None, mesh, 2)
    g.set_operator(sig, lam)
    g.coarse_setup()
    out = {"coef": g.table_f64("coef"), "dmask": g.table_i32("dmask"), "mult": g.table_i32("mult"),
           "rowptr": g.table_i32("coarse_rowptr"), "colidx": g.table_i32("coarse_colidx"), "val": g.table_f64("coarse_val"),
           "volumes": hmg.fields.cell_volumes(mesh)}
    g.close()
    return out


@pytest.mark.parametrize("kw", GENERAL, ids=["plain", "moved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_representatives_do_not_matter(shape, kw):
    """a node stored whole periods away is the same node: every table that reads a coordinate keeps its bits"""
    a, b = general_torus(shape, 11, **kw), general_torus(shape, 11, shift=True, **kw)
    assert np.array_equal(a.elements, b.elements) and not np.array_equal(a.nodes, b.nodes)
    assert np.array_equal(np.mod(a.nodes, a.period), np.mod(b.nodes, b.period))
    rng = np.random.default_rng(12)
    ne, d = a.elements.shape[0], a.dim
    for sig in (rng.random((ne, d)) + 0.5, TS.random_spd(rng, ne, d)):
        ta, tb = _host_tables(a, sig), _host_tables(b, sig)
        for k, v in ta.items():
            assert v.size > 0 and v.dtype == tb[k].dtype and v.tobytes() == tb[k].tobytes(), (shape, k)
    np.testing.assert_array_equal(a.cell_corners() - a.cell_corners()[:, :1], b.cell_corners() - b.cell_corners()[:, :1])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_general_geometry_is_that_of_the_disjoint_simplices_bit_for_bit(shape):
    """test_geometry_is_that_of_the_disjoint_simplices_bit_for_bit on a moved, stretched torus, diagonal and full tensors"""
    mesh = general_torus(shape, 13)
    g, twin = hmg.ImplicitFineGrid(None, mesh, 2), hmg.ImplicitFineGrid(None, ordinary_twin(mesh), 2)
    rng = np.random.default_rng(1)
    ne, d = mesh.elements.shape[0], mesh.dim
    for sig in (np.ones((ne, d)), rng.choice([1.0, 9.0], size=(ne, d)), rng.random((ne, d)) + 0.5, TS.random_spd(rng, ne, d)):
        g.set_operator(sig, 0.0)
        twin.set_operator(sig, 0.0)
        a, b = g.table_f64("coef"), twin.table_f64("coef")
        assert a.size == 8 * ne and np.array_equal(a.view(np.int64), b.view(np.int64))
    np.testing.assert_array_equal(hmg.fields.cell_volumes(mesh).view(np.int64),
                                  hmg.fields.cell_volumes(ordinary_twin(mesh)).view(np.int64))
    twin.close()
    g.close()


@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_general_level_1_matrix_with_full_tensors(shape, lam):
    """test_level_1_matrix on a moved, stretched torus with a full SPD tensor per cell"""
    mesh = general_torus(shape, 14)
    rng = np.random.default_rng(2)
    ne, n = mesh.elements.shape[0], mesh.nodes.shape[0]
    sig = TS.random_spd(rng, ne, mesh.dim)
    g = hmg.ImplicitFineGrid(None, mesh, 2)
    g.set_operator(sig, lam)
    g.coarse_setup()
    A, interior = CF.matrix(g)
    g.close()
    np.testing.assert_array_equal(interior, np.arange(n))
    ids = coarse_ids(mesh, DEN)
    np.testing.assert_array_equal(ids, (mesh.elements - 1).ravel())
    nodes, elements = disjoint(mesh)
    want = stiffness(TextbookP1(nodes, elements), sig, ids, n, lam).toarray()
    got = A.toarray()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())
    # entries (i, j) and (j, i) add their cells' parts in different orders: equal bits on the integer positions of
    # driver.periodic_mesh only; here the bound tests/test_coarse_solve_host.py sets for every level-1 matrix
    assert np.abs(got - got.T).max() <= 1e-14 * np.abs(got).max()
    if lam == 0.0:
        assert np.abs(got.sum(axis=1)).max() <= 1e-13 * np.abs(got).max()


def test_a_jitter_that_reaches_half_a_period_is_refused():
    """3 x 3 cubes stretched to a 6 x 1.5 box: node (0, 0) moved by half a cube along axis 0 makes its edges to the nodes of the
    next column 1.5 cubes long, half the period; the first cell that has such an edge is named"""
    mesh = general_torus((3, 3), 15, jitter=False)
    nodes = mesh.nodes.copy()
    nodes[0, 0] -= 0.5 * 2.0
    X = hmg.Mesh(nodes, mesh.elements, mesh.period).cell_corners()
    spans = np.abs(X[:, :, None, 0] - X[:, None, :, 0]).max(axis=(1, 2)) >= 0.5 * mesh.period[0]
    assert spans.any() and not spans.all()
    first = int(np.flatnonzero(spans)[0])
    raises_creating(hmg.Mesh(nodes, mesh.elements, mesh.period), rf"cell {first} has an edge that spans half the period of axis 0")
    nodes[0, 0] += 0.125 * 2.0                                           # three eighths of a cube: inside, accepted
    hmg.ImplicitFineGrid(None, hmg.Mesh(nodes, mesh.elements, mesh.period), 2).close()
