"""
VTK (.vtu) export of the checkerboard and of a level of the implicit grid -- the reference's `save` option
(src/examples/homogenized_coefficients.jl:69-87, 219, 303; construct_full_grid: src/implicit_fine_grid.jl:41-78).
Output side of the path only: level vectors are read back once per exported level.

Files are VTK XML UnstructuredGrid, inline base64 ("binary") arrays with a UInt64 length header, no compression;
ParaView / VTK / meshio read them.  Raster slices sampled on the device (api.sample_raster) go out as VTK XML StructuredGrid
(.vts: write_vts, export_slice) with the same arrays.
"""
from __future__ import annotations

import base64

import numpy as np

_VTK_TYPE = {1: 1, 3: 5, 4: 10}     # vertex, triangle, tetrahedron
_NAMES = {np.dtype("float64"): "Float64", np.dtype("int64"): "Int64", np.dtype("uint8"): "UInt8",
          np.dtype("int32"): "Int32"}


def _array(f, name, a, ncomp=None):
    a = np.ascontiguousarray(a)
    raw = a.tobytes()
    head = np.array([len(raw)], dtype="<u8").tobytes()
    comp = f' NumberOfComponents="{ncomp}"' if ncomp else ""
    f.write(f'<DataArray type="{_NAMES[a.dtype]}" Name="{name}"{comp} format="binary">\n')
    f.write(base64.b64encode(head + raw).decode("ascii"))
    f.write("\n</DataArray>\n")


def write_vtu(path, points, cells, point_data=None, cell_data=None):
    """points (N, dim), cells (M, dim+1) 0-based; *_data: name -> (N,) / (N, c) array."""
    points = np.asarray(points, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    p3 = np.zeros((points.shape[0], 3))
    p3[:, : points.shape[1]] = points
    nv = cells.shape[1]
    if not path.endswith(".vtu"):
        path += ".vtu"
    with open(path, "w") as f:
        f.write('<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" '
                'header_type="UInt64">\n<UnstructuredGrid>\n')
        f.write(f'<Piece NumberOfPoints="{p3.shape[0]}" NumberOfCells="{cells.shape[0]}">\n<Points>\n')
        _array(f, "Points", p3, 3)
        f.write("</Points>\n<Cells>\n")
        _array(f, "connectivity", cells.ravel())
        _array(f, "offsets", np.arange(1, cells.shape[0] + 1, dtype=np.int64) * nv)
        _array(f, "types", np.full(cells.shape[0], _VTK_TYPE[nv], dtype=np.uint8))
        f.write("</Cells>\n")
        for tag, data in (("PointData", point_data), ("CellData", cell_data)):
            if data:
                f.write(f"<{tag}>\n")
                for name, a in data.items():
                    a = np.asarray(a, dtype=np.float64)
                    _array(f, name, a, a.shape[1] if a.ndim == 2 else None)
                f.write(f"</{tag}>\n")
        f.write("</Piece>\n</UnstructuredGrid>\n</VTKFile>\n")
    return path


def read_vtu(path):
    """Minimal reader for files written by write_vtu (used by the tests)."""
    import xml.etree.ElementTree as ET
    types = {v: k for k, v in _NAMES.items()}
    root = ET.parse(path).getroot()
    out = {"point_data": {}, "cell_data": {}}

    def decode(el):
        raw = base64.b64decode(el.text.strip())
        n = int(np.frombuffer(raw[:8], dtype="<u8")[0])
        a = np.frombuffer(raw[8:8 + n], dtype=types[el.get("type")])
        c = el.get("NumberOfComponents")
        return a.reshape(-1, int(c)) if c else a

    piece = root.find("UnstructuredGrid/Piece")
    out["points"] = decode(piece.find("Points/DataArray"))
    for el in piece.find("Cells"):
        out[el.get("Name")] = decode(el)
    for tag, key in (("PointData", "point_data"), ("CellData", "cell_data")):
        node = piece.find(tag)
        if node is not None:
            for el in node:
                out[key][el.get("Name")] = decode(el)
    return out


def _corners(base, ne):
    """corners (ne, dim + 1, dim) of the first ne cells; the cells of a torus (api.Mesh.period) unwrapped"""
    if getattr(base, "period", None) is not None:
        return base.cell_corners(np.arange(ne))
    return base.nodes[base.elements[:ne] - 1]


def _points_and_cells(base, ne):
    """The first ne cells of a base mesh as write_vtu takes them.  A mesh on a torus goes out with its corners duplicated per cell,
    each cell unwrapped (api.Mesh.cell_corners): with shared points a cell that straddles the box would be drawn across it."""
    if getattr(base, "period", None) is None:
        return base.nodes, base.elements[:ne] - 1
    X = _corners(base, ne)
    return X.reshape(-1, X.shape[2]), np.arange(X.shape[0] * X.shape[1], dtype=np.int64).reshape(X.shape[0], X.shape[1])


def construct_full_grid(implicit, level: int):
    """All cells of refinement level `level` as one explicit mesh; interface nodes are duplicated per coarse cell
    (node n of coarse cell e has index e * Nf + n, n in the reference's hierarchical order).
    ref: src/implicit_fine_grid.jl:41-78"""
    base = implicit.base
    dim = base.dim
    nf = implicit.nf(level)
    m = 2 ** (level - 1)
    h2s = implicit.table_i32("hier2slot", level)
    ijk = implicit.table_i32("slot_ijk", level).reshape(-1, 3)[h2s][:, :dim].astype(np.float64) / m   # (nf, dim)
    ref_cells = implicit.table_i32("ref_cells", level).reshape(-1, dim + 1).astype(np.int64)
    ne = implicit.ncells()                                  # (a shrunk domain is a prefix of the base cells)
    X = _corners(base, ne)                                  # (ne, dim+1, dim); a torus: unwrapped
    J = X[:, 1:, :] - X[:, :1, :]                           # rows: X_a - X_0
    nodes = (X[:, :1, :] + np.einsum("na,eac->enc", ijk, J)).reshape(-1, dim)
    cells = (ref_cells[None, :, :] + (np.arange(ne, dtype=np.int64) * nf)[:, None, None]).reshape(-1, dim + 1)
    return nodes, cells


def export_domain(base, cond, name="checkerboard"):
    """ref: src/examples/homogenized_coefficients.jl:69-79 -- cell data "a" = the diagonal of the conductivity; full tensors
    (ncells, dim, dim): their dim (dim + 1) / 2 components by rows of the upper triangle (3D: 11, 12, 13, 22, 23, 33)."""
    a = np.asarray(cond, dtype=np.float64)
    if a.ndim == 3:
        iu = np.triu_indices(a.shape[1])
        a = np.ascontiguousarray(a[:, iu[0], iu[1]])
    return write_vtu(name, *_points_and_cells(base, base.elements.shape[0]), cell_data={"a": a})


def export_cell_fields(base, fields: dict, name="cell_fields"):
    """The coarse mesh with one value set per cell: fields maps a name to (Ne,), (Ne, c) or (Ne, d, d) -- symmetric tensors such as
    api.cell_moments' gram go out as their d (d + 1) / 2 components by rows of the upper triangle.  The mesh is cut to the cells
    the arrays cover (a shrunk domain is a prefix)."""
    data = {}
    ne = None
    for key, a in fields.items():
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 3:
            iu = np.triu_indices(a.shape[1])
            a = np.ascontiguousarray(a[:, iu[0], iu[1]])
        if ne is None:
            ne = a.shape[0]
        if a.shape[0] != ne or a.ndim > 2:
            raise ValueError(f"cell field {key!r}: {a.shape} does not fit {ne} cells")
        data[key] = a
    if ne is None:
        raise ValueError("no cell field given")
    if ne > base.elements.shape[0]:
        raise ValueError(f"{ne} values for {base.elements.shape[0]} cells")
    return write_vtu(name, *_points_and_cells(base, ne), cell_data=data)


def export_unknown(implicit, x, k: int, level: int, name=None, field="v"):
    """ref: src/examples/homogenized_coefficients.jl:81-87 -- point data "v" = x[1:nnodes(level), :][:] on the full
    grid of `level`.  `x` is a DeviceMatrix of the finest level or a host (Nf, Ne) array in hierarchical order."""
    nodes, cells = construct_full_grid(implicit, level)
    xh = x.to_host() if hasattr(x, "to_host") else np.asarray(x)
    nfl = implicit.nf(level)
    v = np.ascontiguousarray(xh[:nfl, :].T).ravel()
    return write_vtu(name or f"ahom_{k}", nodes, cells, point_data={field: v})


def write_vts(path, points, point_data=None):
    """A VTK XML StructuredGrid of nv x nu points (one layer): points (nv, nu, dim) -- a raster slice of any orientation, index
    [b, a] --, point_data: name -> (nv, nu) or (nv, nu, c) arrays (float64; int32 stays int32).  Same inline base64 arrays as
    write_vtu.  2D points get z = 0 and 2-component vectors a zero third component, so that ParaView takes them as vectors."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 3 or points.shape[2] not in (2, 3):
        raise ValueError(f"points must have shape (nv, nu, dim), not {points.shape}")
    nv, nu, dim = points.shape
    p3 = np.zeros((nv * nu, 3))
    p3[:, :dim] = points.reshape(-1, dim)
    if not path.endswith(".vts"):
        path += ".vts"
    ext = f"0 {nu - 1} 0 {nv - 1} 0 0"
    with open(path, "w") as f:
        f.write('<?xml version="1.0"?>\n<VTKFile type="StructuredGrid" version="1.0" byte_order="LittleEndian" '
                'header_type="UInt64">\n')
        f.write(f'<StructuredGrid WholeExtent="{ext}">\n<Piece Extent="{ext}">\n<Points>\n')
        _array(f, "Points", p3, 3)
        f.write("</Points>\n")
        if point_data:
            f.write("<PointData>\n")
            for name, a in point_data.items():
                a = np.asarray(a)
                a = a.astype(np.int32) if a.dtype == np.int32 else a.astype(np.float64)
                if a.shape[:2] != (nv, nu) or a.ndim > 3:
                    raise ValueError(f"point data {name!r}: {a.shape} does not fit {nv} x {nu} points")
                if a.ndim == 3 and a.shape[2] == 2:
                    a = np.concatenate([a, np.zeros((nv, nu, 1), dtype=a.dtype)], axis=2)
                _array(f, name, a.reshape(nv * nu, -1) if a.ndim == 3 else a.ravel(), a.shape[2] if a.ndim == 3 else None)
            f.write("</PointData>\n")
        f.write("</Piece>\n</StructuredGrid>\n</VTKFile>\n")
    return path


def export_slice(name, origin, du, dv, sampled):
    """A raster slice as api.sample_raster returns it (a dict of (nv, nu[, c]) arrays), written with the pixel positions
    origin + a du + b dv: opens in ParaView whatever the slice's orientation."""
    origin, du, dv = (np.asarray(x, dtype=np.float64) for x in (origin, du, dv))
    first = next(iter(sampled.values()))
    nv, nu = np.asarray(first).shape[:2]
    a = np.arange(nu, dtype=np.float64)[None, :, None]
    b = np.arange(nv, dtype=np.float64)[:, None, None]
    return write_vts(name, origin + a * du + b * dv, sampled)


def export_points(name, points, point_data=None):
    """A point cloud as a .vtu of vertex cells: points (n, dim), point_data name -> (n,) / (n, c).  The peaks of
    api.cell_extrema_where (fields.element_centroids) open in ParaView next to export_cell_fields' mesh.  Points with a NaN
    coordinate (cells without a location) are left out, with their data."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] not in (2, 3):
        raise ValueError(f"points must have shape (n, dim), not {points.shape}")
    keep = ~np.isnan(points).any(axis=1)
    data = {}
    for key, a in (point_data or {}).items():
        a = np.asarray(a, dtype=np.float64)
        if a.shape[0] != points.shape[0] or a.ndim > 2:
            raise ValueError(f"point data {key!r}: {a.shape} does not fit {points.shape[0]} points")
        data[key] = a[keep]
    pts = points[keep]
    return write_vtu(name, pts, np.arange(pts.shape[0], dtype=np.int64)[:, None], point_data=data)
