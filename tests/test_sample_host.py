"""Host side of point sampling (include/hmg.h: hmg_grid_locate, hmg_sample, hmg_sample_raster), without a GPU, on host-only grids:
the locator and the Kuhn decomposition against the numpy statement of tests/_sample_form.py (interior points by construction: cell
and vertex set exactly, weights and gradient weights within bounds derived there), the closed domain and its ties, the locator
after a shrink, the refusals that need no device, the bindings, and the numpy layer on top (fields.py, vtk.write_vts)."""
import base64
import ctypes
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import fields, vtk

import _sample_form as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hmg_grid_locate", "hmg_sample", "hmg_sample_raster")
_grids = {}
_fine = {}


@pytest.fixture(scope="module")
def host(oracle):
    def get(name):
        if name not in _grids:
            _grids[name] = hmg.ImplicitFineGrid(None, F.base_mesh(oracle, name), F.GRID_LEVELS[name])
        return _grids[name]
    yield get
    for g in _grids.values():
        g.close()
    _grids.clear()
    _fine.clear()


def fine(g, name, level):
    if (name, level) not in _fine:
        _fine[(name, level)] = F.FineMesh(g, level)
    return _fine[(name, level)]


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    jl = open(os.path.join(ROOT, "julia", "HomogenizationHIP.jl")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"ccall\(\(:%s,\s*LIB\)" % name, jl), name
    assert L.SIGNATURES["hmg_grid_locate"] == (L.c_int, [L.vp, L.c_int, L.c_i64, L.p_f64, L.p_i32, L.p_i32, L.p_f64, L.p_f64])
    assert callable(hmg.locate) and callable(hmg.sample) and callable(hmg.sample_raster)


def test_the_path_of_the_decomposition_is_the_element_tables(host):
    """The basis the evaluation hard-codes is the one `elem_dirs` exports, and the cumulative sums of the issue's hint invert it."""
    for name, dim in (("cube3x2", 3), ("square4", 2)):
        g = host(name)
        dirs = g.table_i32("elem_dirs", 3).reshape(dim, dim)
        want = [(0, 0, 1), (0, 1, -1), (1, -1, 0)] if dim == 3 else [(0, 1), (1, -1)]
        assert dirs.tolist() == [list(w) for w in want]
        t = np.random.default_rng(0).random(dim)
        Y = np.cumsum(t)[::-1]                                  # (t_i + t_j + t_k, t_i + t_j, t_i)
        assert np.allclose(Y @ dirs, t)                         # sum_a Y_a basis_a = t


@pytest.mark.parametrize("name,level", F.LOCATE_CASES)
def test_locate_against_the_statement(host, name, level):
    g = host(name)
    fm = fine(g, name, level)
    d = fm.dim
    pts = fm.interior_points(200, seed=100 + level)
    cell, nodes, w, gw = hmg.locate(g, level, pts["x"])
    assert np.array_equal(cell, pts["cell"])
    # the vertex set exactly: sort both by node id and carry weights and gradients along
    o_lib, o_ref = np.argsort(nodes, axis=1), np.argsort(pts["nodes"], axis=1)
    assert np.array_equal(np.take_along_axis(nodes, o_lib, 1), np.take_along_axis(pts["nodes"], o_ref, 1))
    w_lib, w_ref = np.take_along_axis(w, o_lib, 1), np.take_along_axis(pts["weights"], o_ref, 1)
    err_w = np.abs(w_lib - w_ref).max()
    g_lib = np.take_along_axis(gw, o_lib[:, :, None], 1)
    g_ref = np.take_along_axis(pts["grads"], o_ref[:, :, None], 1)
    err_g = np.abs(g_lib - g_ref).max()
    print(f"{name} level {level}: weights {err_w:.3e} (bound {fm.T_w():.3e}), gweights {err_g:.3e} (bound {fm.T_gradient(1.0):.3e})")
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() <= 4 * F.EPS
    assert err_w <= fm.T_w()
    assert err_g <= fm.T_gradient(1.0)
    if not name.startswith("delaunay"):
        # the gradients taken from construct_full_grid's own (rounded) nodes: on the cubes the same bound holds for them
        g_exp = np.take_along_axis(pts["grads_explicit"], o_ref[:, :, None], 1)
        assert np.abs(g_lib - g_exp).max() <= fm.T_gradient(1.0)
    assert w.shape == (200, d + 1) and gw.shape == (200, d + 1, d)


@pytest.mark.parametrize("name,level", [("cube3x2", 3), ("square4", 4)])
def test_closed_domain_and_ties(host, name, level):
    g = host(name)
    fm = fine(g, name, level)
    x, lowest = fm.node_points()
    cell, nodes, w, gw = hmg.locate(g, level, x)
    assert (cell >= 0).all()
    assert np.array_equal(cell, lowest)                         # the lowest-numbered coarse cell that has the node
    assert (np.abs(w.max(axis=1) - 1.0) <= fm.T_w()).all()      # one vertex carries the point
    assert (nodes >= 0).all() and (nodes < fm.nf).all()
    assert (w >= 0).all() and np.isfinite(gw).all()
    # ... and that vertex is the node: its hierarchical id is the row of the point in its cell
    top = np.take_along_axis(nodes, w.argmax(axis=1)[:, None], 1)[:, 0]
    pos = fm.nodes.reshape(fm.ne, fm.nf, fm.dim)[cell, top]
    assert np.abs(pos - x).max() <= 8 * F.EPS * fm.X
    # outside the box, NaN and inf
    lo, hi = fm.nodes.min(axis=0), fm.nodes.max(axis=0)
    bad = np.array([hi + 0.5, lo - 0.5, 0.5 * (lo + hi), 0.5 * (lo + hi), 0.5 * (lo + hi)])
    bad[0, 1:] = 0.5 * (lo + hi)[1:]                            # outside along one axis only
    bad[2, 0] = np.nan
    bad[3, -1] = np.inf
    bad[4, 0] = -np.inf
    cell, nodes, w, gw = hmg.locate(g, level, bad)
    assert (cell == -1).all() and (nodes == -1).all() and np.isnan(w).all() and np.isnan(gw).all()


def test_ties_take_one_element_by_the_written_rule(host):
    """A point on a fine face gets weight exactly 0 at the opposite vertex, which is reported as the element's first vertex; the
    same point gives the same answer every time."""
    g = host("square4")
    level = 3
    fm = fine(g, "square4", level)
    c = fm.cells[5]
    x = 0.5 * (fm.nodes[c[0]] + fm.nodes[c[1]])[None, :]         # midpoint of a fine edge: dyadic, exact
    a = hmg.locate(g, level, x)
    b = hmg.locate(g, level, x)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    cell, nodes, w, gw = a
    assert sorted(np.round(w[0], 12).tolist()) == [0.0, 0.5, 0.5]
    k = int(np.argmin(w[0]))
    assert w[0, k] == 0.0 and nodes[0, k] == nodes[0, 0]


def test_after_shrink(oracle):
    base = oracle.order_nodes_and_elements_by_magnitude(oracle.hypercube(3, 2, origin=(-1.0, -1.0, -1.0)))
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 3)
    try:
        fm = F.FineMesh(g, 3)
        pts = fm.interior_points(300, seed=5)
        builds = hmg.locator_counter("sample_locator_builds")
        before = hmg.locate(g, 3, pts["x"])
        assert hmg.locator_counter("sample_locator_builds") == builds + 1
        hmg.locate(g, 3, pts["x"])
        assert hmg.locator_counter("sample_locator_builds") == builds + 1          # built once
        assert np.array_equal(before[0], pts["cell"])
        keep = 24                                                # a prefix of the cells, all nodes kept
        g.shrink(keep, base.nodes.shape[0])
        after = hmg.locate(g, 3, pts["x"])
        assert hmg.locator_counter("sample_locator_builds") == builds + 2
        assert hmg.locator_counter("sample_locator_bytes") > 0 and hmg.locator_counter("sample_locator_max_candidates") >= 1
        gone = pts["cell"] >= keep
        assert gone.any() and (~gone).any()
        assert (after[0][gone] == -1).all()
        for p, q in zip(before, after):
            assert np.array_equal(p[~gone], q[~gone])
    finally:
        g.close()


def test_refusals_of_a_host_only_grid(host):
    lib = L.load()
    g = host("square4")
    d = 2
    x = np.array([[1.5, 1.5]])
    cell = np.zeros(1, dtype=np.int32)
    val = np.zeros(1)
    pc, pv, px = cell.ctypes.data_as(L.p_i32), val.ctypes.data_as(L.p_f64), x.ctypes.data_as(L.p_f64)
    builds = hmg.locator_counter("sample_locator_builds")

    def refused(rc, *words):
        assert rc != 0
        msg = lib.hmg_last_error().decode()
        for w in words:
            assert w in msg, msg

    refused(lib.hmg_grid_locate(None, 1, 1, px, pc, None, None, None), "null grid")
    refused(lib.hmg_grid_locate(g.h, 0, 1, px, pc, None, None, None), "hmg_grid_locate", "level")
    refused(lib.hmg_grid_locate(g.h, 9, 1, px, pc, None, None, None), "hmg_grid_locate", "level")
    refused(lib.hmg_grid_locate(g.h, 2, 1, None, pc, None, None, None), "hmg_grid_locate", "null points")
    refused(lib.hmg_grid_locate(g.h, 2, 1, px, None, None, None, None), "hmg_grid_locate", "output")
    refused(lib.hmg_grid_locate(g.h, 2, 2 ** 31, px, pc, None, None, None), "hmg_grid_locate", "2^31")
    refused(lib.hmg_grid_locate(g.h, 2, -1, px, pc, None, None, None), "hmg_grid_locate")
    cell[0] = 77
    assert lib.hmg_grid_locate(g.h, 2, 0, None, pc, None, None, None) == 0 and cell[0] == 77       # 0 points: success, nothing written
    # the device calls on a grid without a context
    refused(lib.hmg_sample(g.h, 2, None, None, 1, px, pv, None, None), "hmg_sample", "without a device context")
    refused(lib.hmg_sample_raster(g.h, 2, None, None, px, px, px, 1, 1, pv, None, None), "hmg_sample_raster", "without a device context")
    refused(lib.hmg_sample(g.h, 12, None, None, 1, px, pv, None, None), "hmg_sample", "level")
    assert hmg.locator_counter("sample_locator_builds") == builds      # no refusal built anything
    with pytest.raises(ValueError):
        hmg.locate(g, 2, np.zeros((3, d + 1)))


def test_a_partitioned_grid_is_refused():
    """A rank's share of a partition (host-only here) is refused by all three entry points with a message, and no locator is
    built: its cell ids would be rank-local."""
    from homogenization_jl_amd import dist as hdist, driver
    lib = L.load()
    world, dim, width = 4, 2, 4
    origin = (-width / 2.0,) * dim
    base = driver.order_nodes_and_elements_by_magnitude(driver.hypercube(hmg.Tri64, width, origin=origin))
    owner = hdist.block_owner(base, hdist.block_shape(world, dim), width / 2.0, origin)
    g = hdist.PartitionedGrid(None, base, 3, owner, 1, world)
    try:
        x = np.array([[0.25, 0.25]])
        cell, val = np.zeros(1, dtype=np.int32), np.zeros(1)
        pc, pv, px = cell.ctypes.data_as(L.p_i32), val.ctypes.data_as(L.p_f64), x.ctypes.data_as(L.p_f64)
        builds = hmg.locator_counter("sample_locator_builds")
        calls = {"hmg_grid_locate": lambda: lib.hmg_grid_locate(g.h, 2, 1, px, pc, None, None, None),
                 "hmg_sample": lambda: lib.hmg_sample(g.h, 2, None, None, 1, px, pv, None, None),
                 "hmg_sample_raster": lambda: lib.hmg_sample_raster(g.h, 2, None, None, px, px, px, 1, 1, pv, None, None)}
        for name, call in calls.items():
            assert call() != 0, name
            msg = lib.hmg_last_error().decode()
            assert name in msg and "partitioned" in msg, msg
        assert hmg.locator_counter("sample_locator_builds") == builds
        with pytest.raises(L.HmgError, match="partitioned"):
            hmg.locate(g, 2, x)
    finally:
        g.close()


def test_sample_flux_and_energy_density():
    rng = np.random.default_rng(3)
    n, d = 50, 3
    cell = rng.integers(-1, 6, size=n).astype(np.int32)
    grad = rng.standard_normal((n, d))
    diag = rng.random((6, d)) + 0.5
    A = rng.standard_normal((6, d, d))
    full = A @ np.swapaxes(A, 1, 2) + np.eye(d)
    ok = cell >= 0
    for cond, mat in ((diag, np.einsum("ca,ab->cab", diag, np.eye(d))), (full, full)):
        flux = fields.sample_flux(cond, cell, grad)
        dens = fields.sample_energy_density(cond, cell, grad)
        assert flux.shape == (n, d) and dens.shape == (n,)
        assert np.isnan(flux[~ok]).all() and np.isnan(dens[~ok]).all()
        assert np.allclose(flux[ok], np.einsum("nab,nb->na", mat[cell[ok]], grad[ok]), rtol=1e-14, atol=0)
        assert np.allclose(dens[ok], np.einsum("na,nab,nb->n", grad[ok], mat[cell[ok]], grad[ok]), rtol=1e-13, atol=0)
    # raster-shaped input keeps its shape
    flux = fields.sample_flux(diag, cell.reshape(5, 10), grad.reshape(5, 10, d))
    assert flux.shape == (5, 10, d)
    p = fields.line_points([0.0, 1.0, 2.0], [1.0, 1.0, 0.0], 5)
    assert p.shape == (5, 3) and np.array_equal(p[0], [0, 1, 2]) and np.array_equal(p[-1], [1, 1, 0]) and np.allclose(p[2], [0.5, 1, 1])


def test_write_vts_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    nv, nu = 3, 5
    pts = rng.random((nv, nu, 3))
    data = {"value": rng.random((nv, nu)), "gradient": rng.random((nv, nu, 3)), "cell": rng.integers(-1, 9, size=(nv, nu)).astype(np.int32)}
    path = vtk.write_vts(str(tmp_path / "slice"), pts, data)
    assert path.endswith(".vts")
    root = ET.parse(path).getroot()
    assert root.get("type") == "StructuredGrid" and root.get("header_type") == "UInt64"
    sg = root.find("StructuredGrid")
    assert sg.get("WholeExtent") == f"0 {nu - 1} 0 {nv - 1} 0 0"
    piece = sg.find("Piece")
    assert piece.get("Extent") == sg.get("WholeExtent")
    dt = {"Float64": np.float64, "Int32": np.int32}

    def decode(el):
        raw = base64.b64decode(el.text.strip())
        n = int(np.frombuffer(raw[:8], dtype="<u8")[0])
        assert n == len(raw) - 8
        a = np.frombuffer(raw[8:], dtype=dt[el.get("type")])
        c = el.get("NumberOfComponents")
        return a.reshape(-1, int(c)) if c else a

    assert np.array_equal(decode(piece.find("Points/DataArray")), pts.reshape(-1, 3))
    got = {el.get("Name"): decode(el) for el in piece.find("PointData")}
    assert np.array_equal(got["value"], data["value"].ravel())
    assert np.array_equal(got["gradient"], data["gradient"].reshape(-1, 3))
    assert np.array_equal(got["cell"], data["cell"].ravel()) and got["cell"].dtype == np.int32
    # a 2D slice: points padded with z = 0, vectors with a zero third component
    path = vtk.export_slice(str(tmp_path / "s2"), [0.0, 0.0], [0.5, 0.0], [0.0, 0.25],
                            {"value": np.zeros((2, 4)), "gradient": np.ones((2, 4, 2)), "cell": np.zeros((2, 4), dtype=np.int32)})
    piece = ET.parse(path).getroot().find("StructuredGrid/Piece")
    P = decode(piece.find("Points/DataArray"))
    assert P.shape == (8, 3) and np.array_equal(P[5], [0.5, 0.25, 0.0])
