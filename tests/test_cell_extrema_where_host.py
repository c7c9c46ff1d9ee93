"""Host side of the located per-cell extrema (include/hmg.h: hmg_cell_extrema_where, hmg_grid_element_vertices), without a GPU,
on host-only grids: the decode of element codes slot(p) * 8 + k into vertices -- every valid code of a level, against the
oracle's element list and the Kuhn statement of tests/_cell_extrema_form.py; the order of the vertices; the codes it refuses --,
the refusals of the device call that need no device, and the numpy layer on top (fields.py: points, centroids, hot spots)."""
import ctypes

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import fields

import _cell_extrema_form as F

LEVELS = {2: 5, 3: 4}
CASES = [(2, lv) for lv in range(1, 6)] + [(3, lv) for lv in range(1, 5)]
_grids = {}


@pytest.fixture(scope="module")
def host(oracle):
    def get(dim):
        if dim not in _grids:
            base = oracle.hypercube(dim, 1)
            _grids[dim] = (hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), LEVELS[dim]),
                           oracle.ImplicitFineGrid.create(base, LEVELS[dim]))
        return _grids[dim]
    yield get
    for g, _ in _grids.values():
        g.close()
    _grids.clear()


def valid_codes(g, dim, level):
    mask = g.table_i32("elem_mask", level)
    nperm = 6 if dim == 3 else 2
    return np.array([s * 8 + k for s in range(mask.shape[0]) for k in range(nperm) if (mask[s] >> k) & 1], dtype=np.int32)


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("hmg_cell_extrema_where", "hmg_grid_element_vertices"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["hmg_cell_extrema_where"] == (L.c_int, [L.vp, L.vp, L.p_f64, L.p_f64, L.c_int, L.p_f64, L.p_f64, L.p_i32])
    assert L.SIGNATURES["hmg_grid_element_vertices"] == (L.c_int, [L.vp, L.c_int, L.c_i64, L.p_i32, L.p_i32])
    assert callable(hmg.cell_extrema_where) and callable(hmg.element_vertices)


@pytest.mark.parametrize("dim,level", CASES)
def test_every_valid_code_decodes_to_an_element_of_the_level(host, dim, level):
    g, implicit = host(dim)
    codes = valid_codes(g, dim, level)
    nodes = hmg.element_vertices(g, level, codes)
    assert nodes.shape == (codes.shape[0], dim + 1) and nodes.dtype == np.int32
    ref = implicit.reference.levels[level - 1]
    got = sorted(tuple(sorted(int(x) for x in row)) for row in nodes)
    assert len(set(got)) == len(got) == hmg.fine_elements(g, level) == F.fine_elements(dim, level)
    assert got == sorted(tuple(sorted(int(x) for x in t)) for t in ref.elements)
    assert set(got) == F.kuhn_elements(ref.nodes, level)


@pytest.mark.parametrize("dim,level", CASES)
def test_vertices_come_in_the_elements_own_order(host, dim, level):
    """p first (the slot of the code), then one basis vector of "elem_dirs" per step, in the order of the permutation bit k names"""
    import itertools
    g, _ = host(dim)
    codes = valid_codes(g, dim, level)
    nodes = hmg.element_vertices(g, level, codes)
    ijk = g.table_i32("slot_ijk", level).reshape(-1, 3)[:, :dim].astype(np.int64)
    dirs = g.table_i32("elem_dirs", level).reshape(dim, dim).astype(np.int64)
    h2s = g.table_i32("hier2slot", level)
    perms = list(itertools.permutations(range(dim)))                  # lexicographic: k
    X = ijk[h2s[nodes]]                                               # (n, d + 1, d) lattice coordinates of the vertices
    np.testing.assert_array_equal(h2s[nodes[:, 0]], codes >> 3)
    want = np.array([[dirs[b] for b in perms[k]] for k in (codes & 7)])
    np.testing.assert_array_equal(X[:, 1:] - X[:, :-1], want)
    # p is the lexicographically lowest vertex in slot_ijk's (k, j, i) significance and the last vertex is p + s
    np.testing.assert_array_equal(X[:, -1] - X[:, 0], np.broadcast_to(dirs.sum(axis=0), X[:, 0].shape))


def test_codes_that_name_no_element_are_refused(host):
    lib = L.load()
    for dim in (2, 3):
        g, _ = host(dim)
        for level in (1, 2, LEVELS[dim]):
            mask = g.table_i32("elem_mask", level)
            nf, nperm = mask.shape[0], (6 if dim == 3 else 2)
            good = valid_codes(g, dim, level)[:1]
            clear = [s * 8 + k for s in range(nf) for k in range(8) if not (mask[s] >> k) & 1]
            assert any(c & 7 < nperm for c in clear) and any(c & 7 >= nperm for c in clear)
            for bad in (clear[0], clear[-1], next(c for c in clear if c & 7 >= nperm), nf * 8, nf * 8 + 1, -1, -8, 2 ** 31 - 1):
                with pytest.raises(RuntimeError) as e:
                    hmg.element_vertices(g, level, np.concatenate([good, [bad], [nf * 8 + 5]]))
                msg = str(e.value)
                assert "hmg_grid_element_vertices" in msg and f"code {bad} " in msg and "entry 1" in msg, msg
                assert ("bit" in msg) == (0 <= bad < nf * 8), msg
        for bad_level in (0, LEVELS[dim] + 1):
            with pytest.raises(RuntimeError):
                hmg.element_vertices(g, bad_level, [0])
        assert hmg.element_vertices(g, 1, []).shape == (0, dim + 1)
        one = np.zeros(1, dtype=np.int32)
        assert lib.hmg_grid_element_vertices(g.h, 1, 1, None, one.ctypes.data_as(L.p_i32)) != 0
        assert lib.hmg_grid_element_vertices(g.h, 1, 1, one.ctypes.data_as(L.p_i32), None) != 0
        assert lib.hmg_grid_element_vertices(g.h, 1, -1, one.ctypes.data_as(L.p_i32), one.ctypes.data_as(L.p_i32)) != 0
    assert lib.hmg_grid_element_vertices(None, 1, 0, None, None) != 0


def test_refusals_of_the_device_call_that_need_no_device(host):
    lib = L.load()
    g, _ = host(2)
    out = np.zeros((g.ncells(), 2))
    where = np.zeros((g.ncells(), 2, 3), dtype=np.int32)
    po, pw = out.ctypes.data_as(L.p_f64), where.ctypes.data_as(L.p_i32)
    assert lib.hmg_cell_extrema_where(g.h, None, None, None, 0, None, po, pw) != 0
    msg = lib.hmg_last_error().decode()
    assert "hmg_cell_extrema_where" in msg and "without a device context" in msg
    assert lib.hmg_cell_extrema_where(g.h, None, None, None, 0, None, None, pw) != 0
    assert "hmg_cell_extrema_where: null output" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema_where(g.h, None, None, None, 0, None, po, None) != 0
    assert "hmg_cell_extrema_where: null where" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema_where(None, None, None, None, 0, None, po, pw) != 0 and lib.hmg_last_error().decode()


@pytest.mark.parametrize("dim,level", [(2, 1), (2, 4), (3, 1), (3, 3)])
def test_element_points_are_the_full_grids_rows_of_those_vertices(oracle, dim, level):
    """fields.element_points forms the named vertices only; the statement is the whole fine grid (construct_full_grid)"""
    base = F.perturbed_cube(oracle, dim, 2)
    implicit = oracle.ImplicitFineGrid.create(base, level)
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), level)
    try:
        rng = np.random.default_rng(3)
        codes = valid_codes(g, dim, level)
        pick = rng.integers(0, codes.shape[0], size=20)
        nodes = hmg.element_vertices(g, level, codes[pick])
        cells = rng.integers(0, g.ncells(), size=20)
        X = implicit.construct_full_grid(level)                       # (Ne, nf, d)
        want = X[cells[:, None], nodes, :]
        pts = fields.element_points(g, level, cells, nodes)
        assert pts.shape == (20, dim + 1, dim)
        np.testing.assert_allclose(pts, want, rtol=0, atol=1e-14 * np.abs(X).max())
        np.testing.assert_allclose(fields.element_centroids(g, level, cells, nodes), want.mean(axis=1), rtol=0,
                                   atol=1e-14 * np.abs(X).max())
        nodes[3] = -1                                                 # a cell without a location: NaN
        pts = fields.element_points(g, level, cells, nodes)
        assert np.isnan(pts[3]).all() and not np.isnan(np.delete(pts, 3, axis=0)).any()
        with pytest.raises(ValueError):
            fields.element_points(g, level, cells[:5], nodes)
    finally:
        g.close()


def test_hot_spots_rank_cells_by_value_then_by_cell(oracle):
    base = oracle.hypercube(2, 2)
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 3)
    try:
        ne = g.ncells()
        assert ne == 8
        qmax = np.array([1.0, 7.0, 3.0, 7.0, np.nan, 0.5, 7.0, 2.0])
        codes = valid_codes(g, 2, 3)
        nodes = hmg.element_vertices(g, 3, codes[:ne])
        nodes[4] = -1
        cells, values, points = fields.hot_spots(qmax, nodes, g, 3, k=5)
        assert cells.tolist() == [1, 3, 6, 2, 7]                      # equal values by cell id; the NaN cell last, here cut off
        np.testing.assert_array_equal(values, qmax[cells])
        np.testing.assert_array_equal(points, fields.element_centroids(g, 3, cells, nodes[cells]))
        cells, values, points = fields.hot_spots(qmax, nodes, g, 3, k=100)
        assert cells.tolist() == [1, 3, 6, 2, 7, 0, 5, 4] and np.isnan(values[-1]) and np.isnan(points[-1]).all()
    finally:
        g.close()


def test_export_points_writes_a_point_cloud(tmp_path):
    from homogenization_jl_amd import vtk
    pts = np.array([[0.5, 1.0], [np.nan, np.nan], [2.0, 0.25], [1.5, 1.5]])
    q = np.array([3.0, np.nan, 1.0, 2.0])
    path = vtk.export_points(str(tmp_path / "peaks"), pts, {"peak_energy_density": q, "cell": np.arange(4)})
    assert path.endswith("peaks.vtu")
    r = vtk.read_vtu(path)
    np.testing.assert_array_equal(r["points"], [[0.5, 1.0, 0.0], [2.0, 0.25, 0.0], [1.5, 1.5, 0.0]])   # the NaN point is left out
    np.testing.assert_array_equal(r["connectivity"], [0, 1, 2])
    np.testing.assert_array_equal(r["offsets"], [1, 2, 3])
    np.testing.assert_array_equal(r["types"], [1, 1, 1])              # VTK_VERTEX
    np.testing.assert_array_equal(r["point_data"]["peak_energy_density"], [3.0, 1.0, 2.0])
    np.testing.assert_array_equal(r["point_data"]["cell"], [0.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        vtk.export_points(str(tmp_path / "bad"), pts, {"q": q[:3]})
    with pytest.raises(ValueError):
        vtk.export_points(str(tmp_path / "bad"), pts[:, :1])
