"""
Host-side mirror of the reference's level-3 interface (the part of Homogenization.jl that operates on
level vectors), driving libhmg_hip.so through its C ABI.  Names, argument order and meaning follow the
reference (bang-less: `mul!` -> `mul`), so parity tests read like the reference's own tests:

    ImplicitFineGrid(base, levels)            src/implicit_fine_grid.jl:13-18
    ZeroDirichletConstraint                   src/implicit_fine_grid.jl:80-84 (derived by the library)
    L2PlusDivAGrad(..., lam, sigmas)          src/build_local_operators.jl:26-32
    LevelState(ncells, nnodes)                src/multigrid.jl:7-25
    mul / local_residual                      src/apply_local_operators.jl:7-27, 85-133
    apply_constraint / broadcast_interfaces / zero_out_all_but_one / copy_to_base / distribute
                                              src/implicit_fine_grid.jl:94-386
    restrict_to / interpolate_and_sum_to      src/interpolation.jl:52-74
    smoothing_steps / vcycle / BaseLevel      src/multigrid.jl:30-119

Level vectors live in HBM (FP64, entity-major storage order); `DeviceMatrix` is the
`AbstractMatrix` stand-in: `.to_host()` / `.from_host()` speak the reference's Nf x Ne column-major
hierarchical layout.  There is no CPU implementation behind these calls.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass

import numpy as np

from . import _lib as L

Tri64 = "Tri64"   # element-type tags (src/grid.jl:29-37)
Tet64 = "Tet64"

SMOOTHERS = {"cg": 0, "jacobi": 1, "chebyshev": 2}   # hmg_grid_set_smoother, hmg_grid_set_smoother_chebyshev


def _dim_of(tag):
    return {Tri64: 2, Tet64: 3, 2: 2, 3: 3}[tag]


@dataclass
class Mesh:
    """Base mesh (src/grid.jl:19-22). nodes: (Nn, dim) float64; elements: (Ne, dim+1) int64, 1-based,
    each row ascending (src/implicit_fine_grid.jl:14)."""
    nodes: np.ndarray
    elements: np.ndarray
    period: np.ndarray | None = None
    """box length per axis of a mesh on a torus (hmg_grid_create_periodic): the elements name torus nodes, `nodes` holds one
    representative position each; None: an ordinary mesh"""

    @property
    def dim(self):
        return self.nodes.shape[1]

    def cell_corners(self, cells=None):
        """Corner positions of the cells (all, or those of an index array), (n, dim + 1, dim).  On a torus the corners are unwrapped
        relative to the cell's first corner by the minimal image, p0 + (p - p0 - period rint((p - p0) / period)) -- the library's
        rule --, so a cell that straddles the box comes out in one piece, possibly past the far side."""
        el = np.asarray(self.elements, dtype=np.int64)
        if cells is not None:
            el = el[cells if isinstance(cells, slice) else np.asarray(cells)]
        x = np.asarray(self.nodes, dtype=np.float64)[el - 1]
        if self.period is None:
            return x
        per = np.asarray(self.period, dtype=np.float64)
        d = x - x[:, :1, :]
        d -= per * np.rint(d / per)
        return x[:, :1, :] + d


def pack_sigmas(sigmas, ncells, dim):
    """Per-cell conductivities as the library takes them: (ncells, dim) -- diagonal tensors -- stays as it is; (ncells, dim, dim)
    must be symmetric (ValueError otherwise) and is packed to the upper triangle by rows, (ncells, dim (dim + 1) / 2): 3D 11, 12, 13,
    22, 23, 33; 2D 11, 12, 22 (hmg_grid_set_operator_tensor).  Returns (array, is_tensor)."""
    s = np.asarray(sigmas, dtype=np.float64)
    if s.shape == (ncells, dim):
        return np.ascontiguousarray(s), False
    if s.shape != (ncells, dim, dim):
        raise ValueError(f"sigmas must have shape ({ncells}, {dim}) or ({ncells}, {dim}, {dim}), not {s.shape}")
    st = np.swapaxes(s, 1, 2)
    asym = (s != st) & ~(np.isnan(s) & np.isnan(st))       # (what is not finite is the library's to refuse)
    if asym.any():
        raise ValueError(f"the tensor of cell {int(np.argwhere(asym)[0][0])} is not symmetric")
    iu = np.triu_indices(dim)
    return np.ascontiguousarray(s[:, iu[0], iu[1]]), True


def cell_faces(base: Mesh):
    """Every face of every cell of a base mesh (3D: triangles, 2D: edges) as an (Ne * (dim + 1), dim) array of 1-based node ids,
    ascending within a face, cell by cell."""
    el = np.sort(np.asarray(base.elements, dtype=np.int64), axis=1)
    n = el.shape[1]
    return np.concatenate([np.delete(el, l, axis=1)[:, None, :] for l in range(n)], axis=1).reshape(-1, n - 1)


def boundary_faces(base: Mesh):
    """The default constrained set of an ImplicitFineGrid: the faces that belong to one cell, (nfaces, dim), 1-based node ids,
    ascending within a face, faces in lexicographic order (what `ImplicitFineGrid.dirichlet_faces()` answers on a fresh grid)."""
    faces, count = np.unique(cell_faces(base), axis=0, return_counts=True)
    return np.ascontiguousarray(faces[count == 1])


class Context:
    """One GPU + one HIP stream. stream: a raw hipStream_t (int) such as
    torch.cuda.current_stream().cuda_stream, or None for a library-owned stream."""

    def __init__(self, device: int = 0, stream=None):
        self._lib = L.load()
        h = ctypes.c_void_p()
        if stream is None:
            L.check(self._lib.hmg_ctx_create(device, None, ctypes.byref(h)))
        else:   # a raw handle; 0 is torch's default stream
            L.check(self._lib.hmg_ctx_create_on_stream(device, ctypes.c_void_p(int(stream)), ctypes.byref(h)))
        self.h = h
        self.device = device
        self._keepalive = []      # caller-side memory the library points into (e.g. a scalar bank tensor)
        self._fin = weakref.finalize(self, self._lib.hmg_ctx_destroy, h)
        for kv in filter(None, os.environ.get("HMG_OPTIONS", "").split(",")):   # dev knobs for A/B runs, e.g. HMG_OPTIONS=fold_x=0
            name, val = kv.split("=")
            self.set_option(name, int(val))

    def stream_handle(self) -> int:
        """The context's hipStream_t as an integer (0 = the null stream): foreign collectives must be issued on it."""
        return int(self._lib.hmg_ctx_stream(self.h) or 0)

    # -- in-library communicator (RCCL), see include/hmg.h ---------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        L.check(L.load().hmg_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, unique_id: bytes):
        assert len(unique_id) == 128
        L.check(self._lib.hmg_comm_init(self.h, nranks, rank, ctypes.c_char_p(unique_id)))

    def comm_stats(self):
        n = ctypes.c_int64()
        d = ctypes.c_int64()
        L.check(self._lib.hmg_comm_stats(self.h, ctypes.byref(n), ctypes.byref(d)))
        return n.value, d.value

    def comm_sum_host(self, *vals):
        """Sum of a few host doubles over the ranks of the in-library communicator (blocking)."""
        a = np.array(vals, dtype=np.float64)
        L.check(self._lib.hmg_comm_sum_host(self.h, a.ctypes.data_as(L.p_f64), a.size))
        return [float(v) for v in a]

    def sync(self):
        L.check(self._lib.hmg_ctx_sync(self.h))

    def release_memory(self):
        """Hand the pooled blocks of destroyed level vectors back to the device (hmg_ctx_release_memory)."""
        L.check(self._lib.hmg_ctx_release_memory(self.h))

    def set_option(self, name: str, value):
        if isinstance(value, float):
            L.check(self._lib.hmg_ctx_set_option_f64(self.h, name.encode(), value))
        else:
            L.check(self._lib.hmg_ctx_set_option(self.h, name.encode(), int(value)))

    def apply_timing_level(self, level: int):
        """(launches, total_ms, algorithmic_bytes) of the timed operator applies of one level (option "time_apply" = 1 times
        every level)."""
        n = ctypes.c_int64()
        ms = ctypes.c_double()
        by = ctypes.c_double()
        L.check(self._lib.hmg_ctx_apply_timing_level(self.h, int(level), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by)))
        return n.value, ms.value, by.value

    def counter(self, name: str) -> int:
        """Diagnostic counters of the library by name, as include/hmg.h lists them at hmg_ctx_counter ("wave_launches": launches of
        the one-wave-per-cell level-5 apply; "lazy_r_form" / "lazy_ap_form" / "lazy_x_form": what the last V-cycle left pending; "x_deferred" / "x_settled": V-cycles that
        left x-updates pending and those a later call had to finish (option "lazy_x"); "ap_rebuilt": pending
        r-updates that had to form their Ap again first; ...).  -1 for an unknown name."""
        return int(self._lib.hmg_ctx_counter(self.h, name.encode()))

    def apply_timing(self):
        """(launches, total_ms, algorithmic_bytes) of the operator applies timed since option
        "time_apply" was last set."""
        n = ctypes.c_int64()
        ms = ctypes.c_double()
        by = ctypes.c_double()
        L.check(self._lib.hmg_ctx_apply_timing(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by)))
        return n.value, ms.value, by.value

    def close(self):
        if self.h:
            self._fin()           # hmg_ctx_destroy, once
            self.h = None


class ImplicitFineGrid:
    """ImplicitFineGrid(base, levels) + the ZeroDirichletConstraint of the base mesh boundary (or of the faces given to
    `set_dirichlet_faces`).  ctx=None builds host tables only (no compute)."""

    def __init__(self, ctx: Context | None, base: Mesh, levels: int):
        self._lib = L.load()
        self.ctx = ctx
        self.base = base
        self.levels = levels
        nodes = np.ascontiguousarray(base.nodes, dtype=np.float64)
        cells = np.ascontiguousarray(base.elements, dtype=np.int64)
        h = ctypes.c_void_p()
        if getattr(base, "period", None) is not None:   # a grid on a torus (include/hmg.h: hmg_grid_create_periodic)
            per = np.ascontiguousarray(base.period, dtype=np.float64).reshape(-1)
            if per.size != base.dim:
                raise ValueError(f"period must have one entry per axis ({base.dim}), not {per.size}")
            L.check(self._lib.hmg_grid_create_periodic(ctx.h if ctx else None, base.dim, levels, nodes.shape[0],
                                                       nodes.ctypes.data_as(L.p_f64), cells.shape[0],
                                                       cells.ctypes.data_as(L.p_i64), per.ctypes.data_as(L.p_f64), ctypes.byref(h)))
        else:
            L.check(self._lib.hmg_grid_create(ctx.h if ctx else None, base.dim, levels, nodes.shape[0],
                                              nodes.ctypes.data_as(L.p_f64), cells.shape[0],
                                              cells.ctypes.data_as(L.p_i64), ctypes.byref(h)))
        self.h = h
        self._fin = weakref.finalize(self, self._lib.hmg_grid_destroy, h)   # (vectors keep the grid alive, the grid the ctx)

    # -- queries -----------------------------------------------------------------------------
    def nlevels(self):
        return self.levels

    def ncells(self):
        return int(self._lib.hmg_grid_ncells(self.h))

    def nnodes_base(self):
        return int(self._lib.hmg_grid_nnodes(self.h))

    def nf(self, level):
        return int(self._lib.hmg_grid_nf(self.h, level))

    def ld(self, level):
        return int(self._lib.hmg_grid_ld(self.h, level))

    def table_i32(self, which, level=1):
        n = ctypes.c_int64()
        L.check(self._lib.hmg_grid_table_i32(self.h, level, which.encode(), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        L.check(self._lib.hmg_grid_table_i32(self.h, level, which.encode(), out.ctypes.data_as(L.p_i32), n.value,
                                             ctypes.byref(n)))
        return out

    def table_f64(self, which, level=1):
        n = ctypes.c_int64()
        L.check(self._lib.hmg_grid_table_f64(self.h, level, which.encode(), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        L.check(self._lib.hmg_grid_table_f64(self.h, level, which.encode(), out.ctypes.data_as(L.p_f64), n.value,
                                             ctypes.byref(n)))
        return out

    def interior_nodes(self):
        """list_interior_nodes(base), 0-based (src/grid.jl:176-202)"""
        return self.table_i32("interior_nodes")

    # -- operator / domain -------------------------------------------------------------------
    def set_operator(self, sigmas, lam):
        """sigmas: (ncells, dim) diagonal tensors, or (ncells, dim, dim) full symmetric ones (pack_sigmas)."""
        s, tensor = pack_sigmas(sigmas, self.base.elements.shape[0], self.base.dim)
        entry = self._lib.hmg_grid_set_operator_tensor if tensor else self._lib.hmg_grid_set_operator
        L.check(entry(self.h, s.ctypes.data_as(L.p_f64), float(lam)))

    def set_lambda(self, lam):
        L.check(self._lib.hmg_grid_set_lambda(self.h, float(lam)))

    def shrink(self, ncells_prefix, nnodes_prefix):
        L.check(self._lib.hmg_grid_shrink(self.h, ncells_prefix, nnodes_prefix))

    def set_dirichlet_faces(self, faces=None):
        """The faces on which v = 0 holds (include/hmg.h: hmg_grid_set_dirichlet_faces): an (nfaces, dim) array of 1-based node
        ids of the base mesh (3D: triangles, 2D: edges; any order within a face), None for the default -- the faces that belong to
        one cell, `boundary_faces(base)` -- or an empty array for no constraint.  The constrained set is the closure of the faces.
        The level-1 system is due again afterwards (`coarse_setup`; a solve forms it if it is missing) and a FlexibleCG needs a
        new `start`.  Refused on a shrunk grid; `shrink` is refused while a set of the caller's is held."""
        if faces is None:
            L.check(self._lib.hmg_grid_set_dirichlet_faces(self.h, -1, None))
            return
        f = np.ascontiguousarray(faces, dtype=np.int64)
        if f.size == 0:
            f = f.reshape(0, self.base.dim)
        if f.ndim != 2 or f.shape[1] != self.base.dim:
            raise ValueError(f"faces must have shape (nfaces, {self.base.dim}), not {f.shape}")
        L.check(self._lib.hmg_grid_set_dirichlet_faces(self.h, f.shape[0], f.ctypes.data_as(L.p_i64)))

    def dirichlet_faces(self):
        """The current set as an (nfaces, dim) array: 1-based ids, ascending within a face, faces in lexicographic order."""
        n = int(self._lib.hmg_grid_dirichlet_faces(self.h, None, 0))
        if n < 0:
            raise L.HmgError(self._lib.hmg_last_error().decode())
        out = np.zeros((n, self.base.dim), dtype=np.int64)
        self._lib.hmg_grid_dirichlet_faces(self.h, out.ctypes.data_as(L.p_i64), out.size)
        return out

    def set_mean_free(self, on=True):
        """Solve a level-1 system that has the constants in its kernel -- lambda = 0 and no constrained node -- on their complement
        instead of refusing it (include/hmg.h: hmg_grid_set_mean_free): the mean leaves the right-hand side before the level-1 PCG
        and the solution after it, on the device.  A solution is then fixed up to a constant.  Default: on for periodic grids
        only.  The level-1 system is due again afterwards and a FlexibleCG needs a new `start`."""
        L.check(self._lib.hmg_grid_set_mean_free(self.h, 1 if on else 0))

    def mean_free(self) -> bool:
        return int(self._lib.hmg_grid_mean_free(self.h)) == 1

    def set_periodic_sampling(self, on=True):
        """Let `locate`, `sample` and `sample_raster` serve this periodic grid (include/hmg.h: hmg_grid_set_periodic_sampling;
        default off: they refuse it).  Points are taken modulo the period, xi . x at the point as given, so a raster over several
        periods tiles.  Drops the locator; launches nothing.  Refused on a grid that is not periodic."""
        L.check(self._lib.hmg_grid_set_periodic_sampling(self.h, 1 if on else 0))

    def periodic_sampling(self) -> bool:
        on = ctypes.c_int()
        L.check(self._lib.hmg_grid_periodic_sampling(self.h, ctypes.byref(on)))
        return on.value == 1

    def reserve_spare(self, enable=True):
        """The sixth finest-level vector of the default V-cycle form (include/hmg.h: hmg_grid_reserve_spare): True reserves it now
        and raises if the memory is not there, False releases it (the reference's five vectors per level)."""
        L.check(self._lib.hmg_grid_reserve_spare(self.h, 1 if enable else 0))

    def set_smoother(self, kind="cg", ratio=None, lambda_hi=None):
        """The smoother of smoothing_steps / vcycle / FlexibleCG on this grid (include/hmg.h: hmg_grid_set_smoother,
        hmg_grid_set_smoother_chebyshev): "cg" is the reference's (default), "jacobi" is CG preconditioned by the inverse diagonal
        of the assembled operator, "chebyshev" a Chebyshev polynomial in that diagonal times the operator on
        [lambda_hi / ratio, lambda_hi] (no dot products).  "jacobi" and "chebyshev" reserve one vector per level >= 2 and raise if
        the memory is not there; set it before the level vectors are created.
        ratio, lambda_hi ("chebyshev" only): None for the library's default ratio and its own rigorous bounds, or a ratio > 1 and
        one bound per level (entry l - 1 for level l; <= 0: formed).  A partitioned grid needs a bound > 0 for every level >= 2."""
        if kind not in SMOOTHERS:
            raise ValueError(f"smoother must be one of {sorted(SMOOTHERS)}, not {kind!r}")
        if kind != "chebyshev":
            if ratio is not None or lambda_hi is not None:
                raise ValueError('ratio and lambda_hi belong to smoother "chebyshev"')
            L.check(self._lib.hmg_grid_set_smoother(self.h, SMOOTHERS[kind]))
            return
        hi = None
        if lambda_hi is not None:
            hi = np.ascontiguousarray(lambda_hi, dtype=np.float64).reshape(-1)
            if hi.size != self.levels:
                raise ValueError(f"lambda_hi must have one entry per level ({self.levels}), not {hi.size}")
        L.check(self._lib.hmg_grid_set_smoother_chebyshev(self.h, 0.0 if ratio is None else float(ratio),
                                                          hi.ctypes.data_as(L.p_f64) if hi is not None else None))

    def smoother(self) -> str:
        k = int(self._lib.hmg_grid_smoother(self.h))
        return {v: n for n, v in SMOOTHERS.items()}[k]

    def smoother_bounds(self, level):
        """(lambda_lo, lambda_hi) of a level as the "chebyshev" smoother uses them, formed first if stale (synchronises)."""
        lo, hi = ctypes.c_double(), ctypes.c_double()
        L.check(self._lib.hmg_grid_smoother_bounds(self.h, level, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def coarse_setup(self):
        L.check(self._lib.hmg_coarse_setup(self.h))

    def close(self):
        if self.h:
            self._fin()
            self.h = None


class DeviceMatrix:
    """A level vector: the reference's `Nf x Ne` matrix, resident in HBM.  `device_ptr` wraps caller-owned memory of ld * Ne
    doubles (hmg_vec_wrap): device_ptr must be 16-byte aligned -- the vector kernels move pairs of doubles --; any other pointer is
    refused."""

    def __init__(self, implicit: ImplicitFineGrid, level: int, device_ptr=None):
        self._lib = L.load()
        self.implicit = implicit
        self.level = level
        h = ctypes.c_void_p()
        if device_ptr is None:
            L.check(self._lib.hmg_vec_create(implicit.h, level, ctypes.byref(h)))
        else:
            L.check(self._lib.hmg_vec_wrap(implicit.h, level, ctypes.c_void_p(device_ptr), ctypes.byref(h)))
        self.h = h
        # HBM goes back when the object is collected (or close()d); `implicit` is referenced above, so the grid and its
        # context outlive every vector
        self._fin = weakref.finalize(self, self._lib.hmg_vec_destroy, h)

    @property
    def shape(self):
        return (self.implicit.nf(self.level), self.implicit.ncells())

    def from_host(self, a):
        a = np.asfortranarray(a, dtype=np.float64)
        assert a.shape == self.shape, (a.shape, self.shape)
        L.check(self._lib.hmg_vec_upload(self.h, a.ctypes.data_as(L.p_f64)))
        return self

    def to_host(self):
        out = np.zeros(self.shape, dtype=np.float64, order="F")
        L.check(self._lib.hmg_vec_download(self.h, out.ctypes.data_as(L.p_f64)))
        return out

    def fill(self, v):                       # fill!
        L.check(self._lib.hmg_vec_fill(self.h, float(v)))
        return self

    def rand(self, seed, cell_offset=0):     # rand! (seeded, layout independent)
        L.check(self._lib.hmg_vec_fill_random(self.h, int(seed), int(cell_offset)))
        return self

    def copyto(self, src):                   # copyto!(self, src)
        L.check(self._lib.hmg_vec_copy(self.h, src.h))
        return self

    def similar(self):                       # similar(x)
        return DeviceMatrix(self.implicit, self.level)

    def copy(self):                          # copy(x)
        return self.similar().copyto(self)

    def device_ptr(self):
        return int(self._lib.hmg_vec_device_ptr(self.h) or 0)

    def close(self):
        if self.h:
            self._fin()
            self.h = None


def host_random(shape, seed, cell_offset=0):
    """numpy twin of hmg_vec_fill_random (hash of (seed, cell, hierarchical node id))."""
    nf, ne = shape
    with np.errstate(over="ignore"):
        idx = ((np.arange(ne, dtype=np.uint64) + np.uint64(cell_offset)) << np.uint64(20))[None, :] | \
            np.arange(nf, dtype=np.uint64)[:, None]
        z = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return np.asfortranarray((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0))


# BLAS-1 generics used on state vectors (src/multigrid.jl:54,64-68)
def dot(x: DeviceMatrix, y: DeviceMatrix) -> float:
    out = ctypes.c_double()
    L.check(L.load().hmg_vec_dot(x.h, y.h, ctypes.byref(out)))
    return out.value


def norm(x: DeviceMatrix) -> float:
    """norm(x) over the raw storage: shared DOFs counted once per copy, like BLAS on the reference's Matrix."""
    return float(np.sqrt(dot(x, x)))


def axpy(alpha, x: DeviceMatrix, y: DeviceMatrix):
    L.check(L.load().hmg_vec_axpy(float(alpha), x.h, y.h))


def xpby(r: DeviceMatrix, beta, p: DeviceMatrix):
    """p .= r .+ beta .* p"""
    L.check(L.load().hmg_vec_xpby(r.h, float(beta), p.h))


def norm_unique(r: DeviceMatrix) -> float:
    """norm(r) after zero_out_all_but_one!(r) -- without destroying r."""
    out = ctypes.c_double()
    L.check(L.load().hmg_vec_norm_unique(r.h, ctypes.byref(out)))
    return out.value


class _Operator:
    """The library keeps ONE operator (per-cell tensors + lambda) per grid; operator objects re-bind themselves
    when they are used after another one (the reference passes the operator to every call instead)."""

    def _bind(self):
        g = self.implicit
        if getattr(g, "_bound_op", None) is not self:
            g.set_operator(self.sigmas, self._lam)
            g._bound_op = self


class L2PlusDivAGrad(_Operator):
    """lam*I - div(sigma grad), sigma constant per coarse cell; carries the Dirichlet constraint
    (held by the grid).  Mutable lam like the reference's struct.  ref: src/build_local_operators.jl:26-32
    sigmas: (ncells, dim), the diagonals of diagonal tensors as in the reference, or (ncells, dim, dim), full symmetric
    tensors (ValueError if one is not symmetric; the library refuses one that is not positive definite)."""

    def __init__(self, implicit: ImplicitFineGrid, lam: float, sigmas):
        self.implicit = implicit
        self._lam = float(lam)
        self.sigmas = np.ascontiguousarray(sigmas, dtype=np.float64)
        self._bind()                 # (set_operator packs, and checks symmetry, before the library is called)

    @property
    def lam(self):
        return self._lam

    @lam.setter
    def lam(self, v):
        self._lam = float(v)
        if getattr(self.implicit, "_bound_op", None) is self:
            self.implicit.set_lambda(self._lam)


class SimpleDiffusion(_Operator):
    """-a * Laplacian with a scalar coefficient, no mass term (src/build_local_operators.jl:14-24,
    src/apply_local_operators.jl:40-72): the same kernels with sigma = (a, ..., a) in every cell and lambda = 0."""

    def __init__(self, implicit: ImplicitFineGrid, a: float = 1.0):
        self.implicit = implicit
        self.a = float(a)
        self._lam = 0.0
        self.sigmas = np.full((implicit.base.elements.shape[0], implicit.base.dim), self.a)
        self._bind()


class LevelState:
    """x, b, r, p, Ap of one level (src/multigrid.jl:7-25)."""

    def __init__(self, implicit: ImplicitFineGrid, level: int):
        self.level = level
        self.x = DeviceMatrix(implicit, level)
        self.b = DeviceMatrix(implicit, level)
        self.r = DeviceMatrix(implicit, level)
        self.p = DeviceMatrix(implicit, level)
        self.Ap = DeviceMatrix(implicit, level)

    def handles(self):
        return [self.x.h, self.b.h, self.r.h, self.p.h, self.Ap.h]

    def close(self):
        for v in (self.x, self.b, self.r, self.p, self.Ap):
            v.close()


def mul(alpha, implicit: ImplicitFineGrid, A, x: DeviceMatrix, y: DeviceMatrix):
    """y <- alpha*A*x + y   (mul!(alpha, base, A, x, y); A: L2PlusDivAGrad or SimpleDiffusion)"""
    A._bind()
    L.check(L.load().hmg_apply(implicit.h, x.level, float(alpha), x.h, y.h))


def apply_ex(alpha, implicit: ImplicitFineGrid, x: DeviceMatrix, src, out: DeviceMatrix, constrain=False):
    """out = (src or 0) + alpha*A*x, optionally followed by the Dirichlet constraint (one fused kernel)."""
    L.check(L.load().hmg_apply_ex(implicit.h, x.level, float(alpha), x.h, src.h if src is not None else None, out.h,
                                  1 if constrain else 0))


def local_residual(implicit, A, curr: LevelState, k: int):
    A._bind()
    L.check(L.load().hmg_residual(implicit.h, k, curr.x.h, curr.b.h, curr.r.h))


def apply_constraint(x: DeviceMatrix, level: int, implicit: ImplicitFineGrid):
    L.check(L.load().hmg_constraint(implicit.h, level, x.h))


def broadcast_interfaces(x: DeviceMatrix, implicit: ImplicitFineGrid, level: int):
    L.check(L.load().hmg_interface_sum(implicit.h, level, x.h))


def zero_out_all_but_one(x: DeviceMatrix, implicit: ImplicitFineGrid, level: int):
    L.check(L.load().hmg_zero_duplicates(implicit.h, level, x.h))


def restrict_to(y_coarse: DeviceMatrix, implicit: ImplicitFineGrid, x_fine: DeviceMatrix):
    """restrict_to!(y, P, x) with P = interops[x.level - 1]"""
    L.check(L.load().hmg_restrict(implicit.h, x_fine.level, x_fine.h, y_coarse.h))


def interpolate_and_sum_to(y_fine: DeviceMatrix, implicit: ImplicitFineGrid, x_coarse: DeviceMatrix):
    L.check(L.load().hmg_prolong_add(implicit.h, y_fine.level, x_coarse.h, y_fine.h))


def copy_to_base(implicit: ImplicitFineGrid, v1: DeviceMatrix):
    u = np.zeros(implicit.nnodes_base())
    L.check(L.load().hmg_gather_base(implicit.h, v1.h, u.ctypes.data_as(L.p_f64)))
    return u


def distribute(v1: DeviceMatrix, u, implicit: ImplicitFineGrid):
    u = np.ascontiguousarray(u, dtype=np.float64)
    L.check(L.load().hmg_scatter_base(implicit.h, u.ctypes.data_as(L.p_f64), v1.h))


def rhs_axi_grad_v(b: DeviceMatrix, implicit: ImplicitFineGrid, xi):
    """rhs_a xi grad v!(b, dphis, implicit, sigmas, xi): b[i, el] = dot(dphi_i, -|J| J^-1 (sigma .* xi))
    (src/examples/homogenized_coefficients.jl:449-474)"""
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    L.check(L.load().hmg_rhs_axi_grad(implicit.h, xi.ctypes.data_as(L.p_f64), b.h))


def local_rhs(b: DeviceMatrix, implicit: ImplicitFineGrid):
    """local_rhs!(b, implicit): unit load, b[:, e] = |det J_e| * int phi (src/implicit_fine_grid.jl:391-409)"""
    L.check(L.load().hmg_local_rhs(implicit.h, b.h))


def next_rhs(b: DeviceMatrix, x: DeviceMatrix, implicit: ImplicitFineGrid):
    """next_rhs!: b = lam*|J|*M*x  (src/examples/homogenized_coefficients.jl:695-713)"""
    L.check(L.load().hmg_next_rhs(implicit.h, x.h, b.h))


def _integrate(implicit, mode, v, vprev, nsub, xi):
    out = ctypes.c_double()
    xp = None
    if xi is not None:
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        xp = xi.ctypes.data_as(L.p_f64)
    L.check(L.load().hmg_integrate(implicit.h, mode, v.h if v is not None else None,
                                   vprev.h if vprev is not None else None, int(nsub), xp, ctypes.byref(out)))
    return out.value


def integrate_first_term(v0: DeviceMatrix, implicit: ImplicitFineGrid, nsubset: int, xi, b: DeviceMatrix = None) -> float:
    """sum over the first `nsubset` cells of |J| * v0.(dphi.P + M v0)  (src/examples/homogenized_coefficients.jl:592-632).
    dphi.P is the entry of rhs_a xi grad v! for the same xi: pass that vector as `b` (the driver's right-hand side of
    outer step 0); without it a temporary is filled."""
    if b is None:
        b = v0.similar()
        rhs_axi_grad_v(b, implicit, xi)
        try:
            return _integrate(implicit, 0, v0, b, nsubset, xi)
        finally:
            b.close()
    return _integrate(implicit, 0, v0, b, nsubset, xi)


def integrate_terms(vk: DeviceMatrix, vkm1: DeviceMatrix, implicit: ImplicitFineGrid, nsubset: int) -> float:
    """sum |J| * (vk + vkm1).(M vk)  (src/examples/homogenized_coefficients.jl:634-667)"""
    return _integrate(implicit, 1, vk, vkm1, nsubset, None)


def integrate_area(v: DeviceMatrix, implicit: ImplicitFineGrid, nsubset: int) -> float:
    """1' M 1 under the selected cells  (src/examples/homogenized_coefficients.jl:673-689)"""
    return _integrate(implicit, 2, v, None, nsubset, None)


def integrate_pair_mass(v: DeviceMatrix, w: DeviceMatrix, implicit: ImplicitFineGrid, nsubset: int) -> float:
    """Mq(v; w) = sum |J| * w.(M v) over the first `nsubset` cells: the bilinear form of two correctors behind the off-diagonal
    entries of the homogenized tensor (hmg_integrate mode 3).  w may be v; nothing is written.  With the two functions above:
    integrate_terms(v, w) = Mq(v; v) + Mq(v; w), integrate_first_term(v, b) = integrate_pair_load(v, b) + Mq(v; v).
    No counterpart in the reference."""
    return _integrate(implicit, 3, v, w, nsubset, None)


def integrate_pair_load(v: DeviceMatrix, s: DeviceMatrix, implicit: ImplicitFineGrid, nsubset: int) -> float:
    """Lq(v; s) = sum |J| * v.s over the first `nsubset` cells, s a load vector such as rhs_axi_grad_v's (hmg_integrate mode 4:
    a streaming pass of 16 B/DOF, the same bits in every run).  No counterpart in the reference."""
    return _integrate(implicit, 4, v, s, nsubset, None)


def cell_moments(v: DeviceMatrix, implicit: ImplicitFineGrid, xi=None):
    """Per coarse cell the mean gradient and the Gram tensor of the gradient of the level vector v -- with xi, of u = xi.x + v
    (hmg_cell_moments): mean (Ne, d) = (1/|c|) int_c grad u, gram (Ne, d, d) = int_c grad u (x) grad u.  The moments are of the
    vector as stored (no operator, no constraint); on a dist.PartitionedGrid Ne is the number of local cells.  Every level from 1
    is served whose cell fits the LDS (3D 1 to 6, 2D 1 to 8); levels whose cell exceeds it (3D level 7, 2D levels 9-11) are refused
    unless the context option "cell_moments_windows" is 1 (then they walk through a rolling LDS window: the pair kernel with v given
    twice, 8 B/DOF; 2: every level the window kernels can address does, an A/B knob).
    What to do with them: fields.py.  No counterpart in the reference."""
    lib = L.load()
    d = implicit.base.dim
    nmom = int(lib.hmg_cell_moments_count(implicit.h))
    out = np.zeros((implicit.ncells(), nmom), dtype=np.float64)
    xp = None
    if xi is not None:
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (d,):
            raise ValueError(f"xi must have {d} entries")
        xp = xi.ctypes.data_as(L.p_f64)
    L.check(lib.hmg_cell_moments(implicit.h, v.h, xp, out.ctypes.data_as(L.p_f64)))
    iu = np.triu_indices(d)
    gram = np.zeros((out.shape[0], d, d))
    gram[:, iu[0], iu[1]] = out[:, d:]
    gram[:, iu[1], iu[0]] = out[:, d:]
    return np.ascontiguousarray(out[:, :d]), gram


def cell_pair_moments(v: DeviceMatrix, w: DeviceMatrix, implicit: ImplicitFineGrid, xi_v=None, xi_w=None):
    """Per coarse cell the symmetrised cross moment of the gradients of two level vectors of one level -- with xi_v / xi_w (each
    may be None, meaning 0), of u = xi_v.x + v and z = xi_w.x + w (hmg_cell_pair_moments):
    S (Ne, d, d) = 1/2 int_c (grad u (x) grad z + grad z (x) grad u), exactly symmetric.  w may be v: then S is cell_moments' gram
    (to rounding; to the last bit where both go through the window kernels).  One pass of 16 B/DOF; the same vectors-as-stored
    rule, the same refused levels and the same context option "cell_moments_windows" as cell_moments.
    What to do with it: fields.pair_energy, fields.tensor_sensitivity, driver.dirichlet_homogenization_tensor.  No counterpart
    in the reference."""
    lib = L.load()
    d = implicit.base.dim
    nq = int(lib.hmg_cell_pair_moments_count(implicit.h))
    out = np.zeros((implicit.ncells(), nq), dtype=np.float64)
    xp = []
    for xi in (xi_v, xi_w):
        if xi is not None:
            xi = np.ascontiguousarray(xi, dtype=np.float64)
            if xi.shape != (d,):
                raise ValueError(f"xi_v and xi_w must have {d} entries")
        xp.append(xi)
    L.check(lib.hmg_cell_pair_moments(implicit.h, v.h, w.h, *[None if xi is None else xi.ctypes.data_as(L.p_f64) for xi in xp],
                                      out.ctypes.data_as(L.p_f64)))
    iu = np.triu_indices(d)
    S = np.zeros((out.shape[0], d, d))
    S[:, iu[0], iu[1]] = out
    S[:, iu[1], iu[0]] = out
    return S


def fine_elements(implicit: ImplicitFineGrid, level: int) -> int:
    """Fine elements per coarse cell on `level`: 2^(d (level - 1)) (hmg_grid_fine_elements; a host-only grid answers too)."""
    n = int(L.load().hmg_grid_fine_elements(implicit.h, int(level)))
    if n < 0:
        raise ValueError(f"level {level} is not a level of this grid")
    return n


def cell_extrema(v: DeviceMatrix, implicit: ImplicitFineGrid, xi=None, form=None, thresholds=None):
    """Per coarse cell, over its fine elements T, the extrema of q_T = grad u . Q_c grad u with u = xi.x + v (xi None: 0) and how
    many elements exceed each threshold (hmg_cell_extrema): qmax (Ne,), qmin (Ne,), counts (Ne, nthr) int64.  `form` is the
    symmetric Q_c per cell, (Ne, d, d), or (Ne, d) for diagonals; None is the identity, q = |grad u|^2 (fields.energy_form,
    fields.flux_form make the usual ones).  Up to 8 finite thresholds, the same for all cells.  The vector as stored; 3D levels
    1 to 6 and 2D levels 1 to 8; larger cells (3D level 7, 2D levels 9 to 11) are refused unless the context option
    "cell_extrema_windows" is 1 (then they walk through a rolling LDS window; 2 sends every level the window kernels address
    through them, with the same bits; "cell_moments_windows" has no say here, and the counter "cell_extrema_window_launches" counts
    the window launches).  One pass of 8 B/DOF; the same bits in every run.  On a dist.PartitionedGrid Ne is the number of LOCAL cells: `form` and all three results are per local cell
    (form = global_form[implicit.local_cells]; a form of global length is refused), while the operator's sigma is the global field.
    qmax and qmin of a cell are NaN exactly when q_T is NaN on one of its elements (a NaN in the cell's column, inf - inf); an
    infinite q_T is a value; a NaN element is counted for no threshold; other cells are untouched.
    What to do with the results: fields.exceedance_volume, fields.concentration; cell_extrema_where also says where the extrema
    sit.  No counterpart in the reference."""
    return _cell_extrema(v, implicit, xi, form, thresholds, False)


def cell_extrema_where(v: DeviceMatrix, implicit: ImplicitFineGrid, xi=None, form=None, thresholds=None):
    """cell_extrema, and which fine element holds each extremum (hmg_cell_extrema_where): (qmax, qmin, counts, where_max,
    where_min).  The first three are cell_extrema's for the same arguments, bit for bit.  where_max, where_min (Ne, d + 1) int32:
    the vertices of the element that attains the maximum (minimum) of the cell, as 0-based HIERARCHICAL node ids -- rows of
    `DeviceMatrix.to_host()`, the convention of `locate` -- in the element's own order p, p + pi1, p + pi1 + pi2, p + s.  Among
    elements of equal value (==) the one with the lowest code slot(p) * 8 + k is reported (slot: table "hier2slot"; k: the bit of
    table_i32 "elem_mask"), so the ints are the same for every launch shape, kernel family and run.  A cell whose extrema are NaN
    has -1 in both rows; an infinite value has a location.  The same single pass of 8 B/DOF; served and refused as cell_extrema
    (option "cell_extrema_windows", partitioned and shrunk grids).  Counters: "cell_extrema_where_launches",
    "cell_extrema_where_kernel_ns".  fields.element_centroids turns the vertices into points, fields.hot_spots ranks them."""
    return _cell_extrema(v, implicit, xi, form, thresholds, True)


def element_vertices(implicit: ImplicitFineGrid, level: int, codes):
    """The vertices of the fine elements of `level` named by codes slot(p) * 8 + k (hmg_grid_element_vertices; host only, a grid
    without a context too): (n, d + 1) int32, 0-based hierarchical node ids in the element's order p, p + pi1, p + pi1 + pi2, p + s.
    A code whose slot is out of range or whose bit k of the slot's "elem_mask" is clear is refused."""
    lib = L.load()
    d = implicit.base.dim
    c = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
    nodes = np.zeros((c.shape[0], d + 1), dtype=np.int32)
    L.check(lib.hmg_grid_element_vertices(implicit.h, int(level), c.shape[0], c.ctypes.data_as(L.p_i32), nodes.ctypes.data_as(L.p_i32)))
    return nodes


def _cell_extrema(v, implicit, xi, form, thresholds, located):
    lib = L.load()
    d = implicit.base.dim
    ne = implicit.ncells()
    xp = fp = tp = None
    if xi is not None:
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (d,):
            raise ValueError(f"xi must have {d} entries")
        xp = xi.ctypes.data_as(L.p_f64)
    if form is not None:
        q = np.asarray(form, dtype=np.float64)
        iu = np.triu_indices(d)
        if q.shape == (ne, d):
            full = np.zeros((ne, d, d))
            full[:, np.arange(d), np.arange(d)] = q
            q = full
        if q.shape != (ne, d, d):
            raise ValueError(f"form must have shape ({ne}, {d}, {d}) or ({ne}, {d}), not {q.shape}")
        if not np.array_equal(q, np.swapaxes(q, 1, 2)):
            raise ValueError("form must be symmetric in every cell")
        packed = np.ascontiguousarray(q[:, iu[0], iu[1]])
        fp = packed.ctypes.data_as(L.p_f64)
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
    if thr.ndim != 1:
        raise ValueError("thresholds must be a list of numbers")
    nthr = int(thr.shape[0])
    if nthr:
        tp = thr.ctypes.data_as(L.p_f64)
    out = np.zeros((ne, 2 + nthr), dtype=np.float64)
    if located:
        where = np.zeros((ne, 2, d + 1), dtype=np.int32)
        L.check(lib.hmg_cell_extrema_where(implicit.h, v.h, xp, fp, nthr, tp, out.ctypes.data_as(L.p_f64), where.ctypes.data_as(L.p_i32)))
    else:
        L.check(lib.hmg_cell_extrema(implicit.h, v.h, xp, fp, nthr, tp, out.ctypes.data_as(L.p_f64)))
    res = (np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1]), np.rint(out[:, 2:]).astype(np.int64))
    if located:
        res += (np.ascontiguousarray(where[:, 0]), np.ascontiguousarray(where[:, 1]))
    return res


def histogram_nbins(emin: int, emax: int, sub_bits: int = 3) -> int:
    """Bins of the floating-point buckets (hmg_histogram_nbins): nreg + 3 with nreg = (emax - emin) 2^sub_bits regular bins, one
    below 2^emin, one from 2^emax up, one for NaN.  -1022 <= emin < emax <= 1023, sub_bits 0 to 5; anything else is refused with
    a message naming the parameter.  (cell_histogram serves nreg <= 1024.)"""
    n = int(L.load().hmg_histogram_nbins(int(emin), int(emax), int(sub_bits)))
    if n < 0:
        raise L.HmgError(L.load().hmg_last_error().decode())
    return n


def histogram_edges(emin: int, emax: int, sub_bits: int = 3):
    """The nreg + 1 edges E_i = 2^(emin + i div 2^s) (1 + (i mod 2^s) / 2^s) of the regular bins (hmg_histogram_edges), every one an
    exact double: bin b = 1 .. nreg of cell_histogram is [E_(b-1), E_b)."""
    edges = np.zeros(histogram_nbins(emin, emax, sub_bits) - 2)
    L.check(L.load().hmg_histogram_edges(int(emin), int(emax), int(sub_bits), edges.ctypes.data_as(L.p_f64)))
    return edges


def histogram_bin(q, emin: int, emax: int, sub_bits: int = 3):
    """The bin of every entry of q (hmg_histogram_bin; host only, no grid): int32, the shape of q.  For a q that is no NaN the
    number of edges <= q -- np.searchsorted(histogram_edges(...), q, "right"): 0 below 2^emin (zeros, negatives, denormals),
    nreg + 1 from 2^emax up --, nreg + 2 for a NaN.  The text the kernel of cell_histogram runs."""
    x = np.ascontiguousarray(q, dtype=np.float64)
    bins = np.zeros(x.shape, dtype=np.int32)
    L.check(L.load().hmg_histogram_bin(x.size, x.ctypes.data_as(L.p_f64), int(emin), int(emax), int(sub_bits),
                                       bins.ctypes.data_as(L.p_i32)))
    return bins


def cell_histogram(v: DeviceMatrix, implicit: ImplicitFineGrid, xi=None, form=None, *, emin: int, emax: int, sub_bits: int = 3):
    """Per coarse cell the histogram, over its fine elements T, of q_T = grad u . Q_c grad u with u = xi.x + v (xi None: 0)
    (hmg_cell_histogram): counts (Ne, nbins) int64, nbins = histogram_nbins(emin, emax, sub_bits) <= 1027.  `xi` and `form` are
    cell_extrema's -- the symmetric Q_c per cell, (Ne, d, d), or (Ne, d) for diagonals; None is the identity -- and so are the
    values, bit for bit: counts[:, b:].sum(1) for an edge E_(b-1) equals cell_extrema's count for the threshold
    nextafter(E_(b-1), -inf).  Bins: histogram_edges / histogram_bin; column 0 is everything below 2^emin (zeros, negatives),
    column nreg + 1 everything from 2^emax up, the last column the NaN elements; a row sums to fine_elements.  The vector as
    stored; 3D levels 1 to 6 and 2D levels 1 to 8; larger cells (3D level 7, 2D levels 9 to 11) are refused whatever
    "cell_extrema_windows" says, unless the context option "cell_histogram_windows" -- this call's own, 0 by default -- is 1: then
    they walk through a rolling LDS window and give the same ints (2 sends every level the window kernels address through them;
    counter "cell_histogram_window_launches"; "cell_histogram_variant" has no say in the window kernels).  One pass of 8 B/DOF; integer counts, the same in every run and for every launch shape.  On a
    dist.PartitionedGrid Ne is the number of LOCAL cells, as in cell_extrema; shrunk and periodic grids are served.
    Counters: "cell_histogram_launches", "cell_histogram_kernel_ns".
    What to do with the result: fields.histogram_volume, fields.histogram_quantile, fields.histogram_tail.  No counterpart in
    the reference."""
    lib = L.load()
    d = implicit.base.dim
    ne = implicit.ncells()
    nbins = histogram_nbins(emin, emax, sub_bits)
    xi, xp = _vec_of(implicit, "xi", xi)
    fp = None
    if form is not None:
        packed = _packed_form(form, ne, d)
        fp = packed.ctypes.data_as(L.p_f64)
    counts = np.zeros((ne, nbins), dtype=np.int64)
    L.check(lib.hmg_cell_histogram(implicit.h, v.h, xp, fp, int(emin), int(emax), int(sub_bits), counts.ctypes.data_as(L.p_i64)))
    return counts


def histogram_group_sum(counts, group_of_cell, ngroups, weights):
    """The statement of hmg_cell_histogram_groups' FP64 sum in numpy, in the documented order: per group the cells by ascending
    cell id, s = 0.0, then s = s + w[c] * float(counts[c, b]) cell after cell -- the product rounded, then the sum (numpy never
    fuses them).  counts (Ne, nbins) integers, group_of_cell (Ne,) in -1 .. ngroups - 1, weights (Ne,): (ngroups, nbins) float64,
    the bits the device gives."""
    counts = np.asarray(counts)
    group_of_cell = np.asarray(group_of_cell)
    w = np.asarray(weights, dtype=np.float64)
    out = np.zeros((int(ngroups), counts.shape[1]), dtype=np.float64)
    for c in range(counts.shape[0]):                                  # ascending cell id
        k = int(group_of_cell[c])
        if k >= 0:
            out[k] = out[k] + w[c] * counts[c].astype(np.float64)
    return out


def cell_histogram_groups(v: DeviceMatrix, implicit: ImplicitFineGrid, labels, xi=None, form=None, weights=None, *, emin: int,
                          emax: int, sub_bits: int = 3):
    """cell_histogram summed over groups of cells ON THE DEVICE (hmg_cell_histogram_groups): returns (group_labels, counts,
    volume).  `labels` (Ne,) integers, one per cell; group_labels = np.unique of the labels that are >= 0, sorted -- a NEGATIVE
    label (or a masked entry of a numpy masked array) puts the cell into no group.  counts (G, nbins) int64: counts[k] =
    cell_histogram(...)[labels == group_labels[k]].sum(0), exactly.  `weights` (Ne,) finite floats (a cell's volume over
    fine_elements gives volumes per bin) or None: volume (G, nbins) float64 = sum_c weights[c] * counts_c, summed per group by
    ASCENDING CELL ID from 0.0 with product and sum rounded separately (histogram_group_sum is that order in numpy: the same
    bits, in every run and on every device), or None without weights.  G * nbins numbers come down instead of Ne * nbins.  The
    pass, its levels, options ("cell_histogram_windows") and counters are cell_histogram's; the group kernel's time is the counter
    "cell_histogram_groups_kernel_ns".  No labels >= 0 at all: G = 0 and empty arrays, nothing is launched.  On a
    dist.PartitionedGrid labels and weights go by LOCAL cell.  No counterpart in the reference."""
    lib = L.load()
    d = implicit.base.dim
    ne = implicit.ncells()
    nbins = histogram_nbins(emin, emax, sub_bits)
    lab = np.ma.asarray(labels)
    if lab.shape != (ne,) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"labels must be ({ne},) integers")
    lab = np.ma.filled(lab.astype(np.int64), -1)
    group_labels = np.unique(lab[lab >= 0])
    ngroups = int(group_labels.size)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (ne,):
            raise ValueError(f"weights must be ({ne},)")
    counts = np.zeros((ngroups, nbins), dtype=np.int64)
    volume = None if w is None else np.zeros((ngroups, nbins), dtype=np.float64)
    if ngroups == 0:
        return group_labels, counts, volume
    group_of_cell = np.where(lab >= 0, np.searchsorted(group_labels, lab), -1).astype(np.int32)
    xi, xp = _vec_of(implicit, "xi", xi)
    fp = None
    if form is not None:
        packed = _packed_form(form, ne, d)
        fp = packed.ctypes.data_as(L.p_f64)
    L.check(lib.hmg_cell_histogram_groups(implicit.h, v.h, xp, fp, int(emin), int(emax), int(sub_bits), ngroups,
                                          group_of_cell.ctypes.data_as(L.p_i32), None if w is None else w.ctypes.data_as(L.p_f64),
                                          counts.ctypes.data_as(L.p_i64), None if volume is None else volume.ctypes.data_as(L.p_f64)))
    return group_labels, counts, volume


def _packed_form(form, ne, d):
    """a symmetric form per cell, (ne, d, d) or (ne, d) diagonals, as the nq numbers per cell the C entry points take"""
    q = np.asarray(form, dtype=np.float64)
    iu = np.triu_indices(d)
    if q.shape == (ne, d):
        full = np.zeros((ne, d, d))
        full[:, np.arange(d), np.arange(d)] = q
        q = full
    if q.shape != (ne, d, d):
        raise ValueError(f"form must have shape ({ne}, {d}, {d}) or ({ne}, {d}), not {q.shape}")
    if not np.array_equal(q, np.swapaxes(q, 1, 2)):
        raise ValueError("form must be symmetric in every cell")
    return np.ascontiguousarray(q[:, iu[0], iu[1]])


def _points_of(implicit, points):
    d = implicit.base.dim
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim == 1 and p.shape[0] == d:
        p = p.reshape(1, d)
    if p.ndim != 2 or p.shape[1] != d:
        raise ValueError(f"points must have shape (npoints, {d}), not {p.shape}")
    return p


def _vec_of(implicit, name, x):
    if x is None:
        return None, None
    d = implicit.base.dim
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (d,):
        raise ValueError(f"{name} must have {d} entries")
    return x, x.ctypes.data_as(L.p_f64)


def locator_counter(name: str) -> int:
    """The process-wide counters of the sampling locator ("sample_locator_builds", "sample_locator_bytes",
    "sample_locator_max_candidates"): hmg_ctx_counter answers them without a context, so a host-only grid can be asked too."""
    return int(L.load().hmg_ctx_counter(None, name.encode()))


def locate(implicit: ImplicitFineGrid, level: int, points):
    """Where points of physical space lie in `level` of the grid (hmg_grid_locate; host only, a grid without a context too):
    (cell, nodes, weights, gweights) with cell (n,) int32 -- the lowest current coarse cell that contains the point up to a slack of
    2^-40 in barycentric coordinates, -1 for none or a coordinate that is not finite --, nodes (n, d + 1) int32 -- the vertices of
    the fine element the point is evaluated in, as 0-based HIERARCHICAL ids: rows of `DeviceMatrix.to_host()` --, weights (n, d + 1)
    -- its P1 weights there, >= 0 --, and gweights (n, d + 1, d) with gradient = sum_k x_host[nodes[k], cell] gweights[k].  A vertex
    whose weight is exactly 0 is reported as the element's first vertex (the gradient identity then needs the element's own
    vertices: it holds wherever all weights are positive).  The element of a point on a fine face, edge or node is fixed by the
    rule in include/hmg.h.  Points without a cell: nodes -1, weights and gweights NaN."""
    lib = L.load()
    d = implicit.base.dim
    p = _points_of(implicit, points)
    n = p.shape[0]
    cell = np.zeros(n, dtype=np.int32)
    nodes = np.zeros((n, d + 1), dtype=np.int32)
    w = np.zeros((n, d + 1))
    gw = np.zeros((n, d + 1, d))
    L.check(lib.hmg_grid_locate(implicit.h, int(level), n, p.ctypes.data_as(L.p_f64), cell.ctypes.data_as(L.p_i32),
                                nodes.ctypes.data_as(L.p_i32), w.ctypes.data_as(L.p_f64), gw.ctypes.data_as(L.p_f64)))
    return cell, nodes, w, gw


def sample(v: DeviceMatrix, implicit: ImplicitFineGrid, points, xi=None, gradient=True, value=True, cell=True):
    """u = xi.x + v and its gradient at points of physical space, evaluated on the device from the vector as stored (hmg_sample):
    a dict with "value" (n,), "gradient" (n, d) and "cell" (n,) int32 -- the entries switched off by gradient / value / cell =
    False are missing.  Per point: the coarse cell of `locate`, the P1 interpolant of v on one fine element of v's level, its
    constant gradient there; NaN / -1 where no cell contains the point.  Only the points go up and the results come down.
    The call reads the vector through `v.device_ptr()`, which settles a pending r-update of v and marks it exposed: sampling a
    LevelState's r, p or Ap keeps the eager tail of `vcycle` for that vector from then on; sampling x changes nothing.
    Not on partitioned grids.  Counters: "sample_launches", "sample_kernel_ns", "sample_download_ns"."""
    lib = L.load()
    d = implicit.base.dim
    p = _points_of(implicit, points)
    n = p.shape[0]
    xi, xp = _vec_of(implicit, "xi", xi)
    out = {}
    if value:
        out["value"] = np.zeros(n)
    if gradient:
        out["gradient"] = np.zeros((n, d))
    if cell:
        out["cell"] = np.zeros(n, dtype=np.int32)
    L.check(lib.hmg_sample(implicit.h, int(v.level), ctypes.c_void_p(v.device_ptr()), xp, n, p.ctypes.data_as(L.p_f64),
                           out["value"].ctypes.data_as(L.p_f64) if value else None,
                           out["gradient"].ctypes.data_as(L.p_f64) if gradient else None,
                           out["cell"].ctypes.data_as(L.p_i32) if cell else None))
    return out


def sample_raster(v: DeviceMatrix, implicit: ImplicitFineGrid, origin, du, dv, nu: int, nv: int, xi=None, gradient=True):
    """`sample` on the pixels x(a, b) = origin + a du + b dv, 0 <= a < nu, 0 <= b < nv, of a slice of any orientation
    (hmg_sample_raster): the points are formed on the device, fma(b, dv, fma(a, du, origin)) per component, nothing is uploaded.
    Returns a dict of arrays shaped (nv, nu): "value", "cell" (int32), and "gradient" (nv, nu, d) unless gradient = False.  Pixels
    outside the domain: NaN / -1."""
    lib = L.load()
    d = implicit.base.dim
    nu, nv = int(nu), int(nv)
    xi, xp = _vec_of(implicit, "xi", xi)
    o, op = _vec_of(implicit, "origin", np.asarray(origin, dtype=np.float64))
    u, up = _vec_of(implicit, "du", np.asarray(du, dtype=np.float64))
    w, wp = _vec_of(implicit, "dv", np.asarray(dv, dtype=np.float64))
    if nu < 0 or nv < 0:
        raise ValueError("nu and nv must not be negative")
    out = {"value": np.zeros((nv, nu)), "cell": np.zeros((nv, nu), dtype=np.int32)}
    if gradient:
        out["gradient"] = np.zeros((nv, nu, d))
    L.check(lib.hmg_sample_raster(implicit.h, int(v.level), ctypes.c_void_p(v.device_ptr()), xp, op, up, wp, nu, nv,
                                  out["value"].ctypes.data_as(L.p_f64),
                                  out["gradient"].ctypes.data_as(L.p_f64) if gradient else None,
                                  out["cell"].ctypes.data_as(L.p_i32)))
    return out


def smoothing_steps(steps, implicit, ops, curr: LevelState, k: int):
    ops._bind()
    L.check(L.load().hmg_smooth(implicit.h, k, steps, curr.x.h, curr.b.h, curr.r.h, curr.p.h, curr.Ap.h))


def set_smoother(implicit: ImplicitFineGrid, kind: str = "cg", **kw):
    """"cg" (the reference's smoother, default), "jacobi" (CG preconditioned by the inverse diagonal) or "chebyshev" (a Chebyshev
    polynomial in the inverse diagonal times the operator; keywords ratio, lambda_hi: ImplicitFineGrid.set_smoother)."""
    implicit.set_smoother(kind, **kw)


def smoother_bounds(implicit: ImplicitFineGrid, level: int):
    """(lambda_lo, lambda_hi) of the level's "chebyshev" smoother."""
    return implicit.smoother_bounds(level)


def smoother_diag(implicit: ImplicitFineGrid, level: int, out: DeviceMatrix = None) -> DeviceMatrix:
    """The level's inverse diagonal as the "jacobi" and "chebyshev" smoothers use it (0 on constrained nodes), formed first if it is
    stale."""
    out = DeviceMatrix(implicit, level) if out is None else out
    L.check(implicit._lib.hmg_grid_smoother_diag(implicit.h, level, out.h))
    return out


class BaseLevel:
    """Coarse-level solver handle: the library's device-resident CG on the assembled level-1 operator, preconditioned by
    four Chebyshev iterates of the Jacobi-scaled operator (27 iterations at config 3), replaces
    `cholesky(assemble_checkerboard(...)[interior, interior])`."""

    def __init__(self, implicit: ImplicitFineGrid):
        self.implicit = implicit
        implicit.coarse_setup()

    def last_iterations(self):
        """Iterations of the last level-1 solve (waits for it).  Raises if that solve did not converge."""
        n = int(L.load().hmg_coarse_last_iterations(self.implicit.h))
        if n < 0:
            raise L.HmgError(L.load().hmg_last_error().decode())
        return n

    def misses(self):
        """Budgeted level-1 solves that ran out of iterations so far (each was reported as an error, or dropped with
        the matrix it belonged to)."""
        return int(L.load().hmg_coarse_misses(self.implicit.h))


def vcycle(implicit: ImplicitFineGrid, base: BaseLevel, ops, levels, k: int, steps: int = 2, steps_coarse: int = 2):
    """vcycle!(implicit, base, ops, levels, k, steps).  steps_coarse = 2 reproduces the reference,
    which does not forward `steps` to the recursive call (src/multigrid.jl:109)."""
    ops[k - 1]._bind()
    L.check(L.load().hmg_vcycle(implicit.h, k, steps, steps_coarse, _state_handles(levels)))


def vcycle_tolerant(implicit: ImplicitFineGrid, base: BaseLevel, ops, levels, k: int, steps: int = 2, steps_coarse: int = 2):
    """vcycle! for driver loops: a budgeted level-1 solve that ran out of its blind iteration budget (the library reports it at the
    first synchronising call behind the V-cycle, include/hmg.h) does not end the run -- the V-cycle it belongs to used an inexact
    coarse-grid correction, which makes it a weaker but valid iterate of the outer iteration; the library has dropped the budget
    and counts the next solve again.  Returns False for such a cycle.  (The reference's CHOLMOD solve cannot miss,
    src/multigrid.jl:84; any other error is raised.)"""
    vcycle(implicit, base, ops, levels, k, steps, steps_coarse)
    try:
        implicit.ctx.sync()
    except L.HmgError as e:
        if "did not reach coarse_rtol" not in str(e):
            raise
        return False
    return True


class FlexibleCG:
    """Flexible CG with one retained direction, preconditioned by one vcycle! per iteration (include/hmg.h, hmg_fcg_*): the
    Krylov counterpart of repeating `vcycle`.  Owns p, q and R -- three vectors of level k's size, allocated here.  The iterate
    is a vector of the caller's that is none of levels[k-1]'s five; levels[k-1].x receives the preconditioned residual and
    levels[k-1].b is left alone.  `start` once per operator / domain / right-hand side (after a shrink or a change of lam a
    `step` without it raises), then one `step` per iteration; nothing in a step waits for the device."""

    def __init__(self, implicit: ImplicitFineGrid, base: BaseLevel, ops, levels, k: int, steps: int = 3, steps_coarse: int = 2):
        self._lib = L.load()
        self.implicit, self.ops, self.levels, self.k = implicit, ops, levels, k
        self.x = None
        ops[k - 1]._bind()
        h = ctypes.c_void_p()
        L.check(self._lib.hmg_fcg_create(implicit.h, k, int(steps), int(steps_coarse), ctypes.byref(h)))
        self.h = h
        self._fin = weakref.finalize(self, self._lib.hmg_fcg_destroy, h)

    def start(self, x: DeviceMatrix, b: DeviceMatrix):
        """R = b - A_loc x; x must be consistent and constrained (broadcast_interfaces / apply_constraint)."""
        self.ops[self.k - 1]._bind()
        L.check(self._lib.hmg_fcg_start(self.h, x.h, b.h, _state_handles(self.levels)))
        self.x = x
        return self

    def step(self):
        L.check(self._lib.hmg_fcg_step(self.h, self.x.h, _state_handles(self.levels)))

    def step_tolerant(self) -> bool:
        """`step` for driver loops, as `vcycle_tolerant`: False if the V-cycle inside used an inexact level-1 solve (the step is
        then a weaker but valid iterate: flexible CG tolerates a preconditioner that varies)."""
        self.step()
        try:
            self.implicit.ctx.sync()
        except L.HmgError as e:
            if "did not reach coarse_rtol" not in str(e):
                raise
            return False
        return True

    def residual_norm(self) -> float:
        """Norm of the true residual (interface-summed R, every node once); waits for the device."""
        out = ctypes.c_double()
        L.check(self._lib.hmg_fcg_residual_norm(self.h, _state_handles(self.levels), ctypes.byref(out)))
        return out.value

    def scalars(self):
        """(alpha, beta, p.q, p.R) of the last step; waits for the device."""
        out = (ctypes.c_double * 4)()
        L.check(self._lib.hmg_fcg_scalars(self.h, out))
        return tuple(out)

    def vec(self, which: str) -> np.ndarray:
        """Host copy of "p", "q" or "R" (Nf x Ne, hierarchical order)."""
        h = self._lib.hmg_fcg_vec(self.h, "pqR".index(which))
        shape = (self.implicit.nf(self.k), self.implicit.ncells())
        out = np.zeros(shape, dtype=np.float64, order="F")
        L.check(self._lib.hmg_vec_download(ctypes.c_void_p(h), out.ctypes.data_as(L.p_f64)))
        return out

    def close(self):
        if self.h:
            self._fin()
            self.h = None


def _state_handles(levels):
    arr = (ctypes.c_void_p * (5 * len(levels)))()
    for i, st in enumerate(levels):
        if st is None:
            continue
        for q, h in enumerate(st.handles()):
            arr[5 * i + q] = h
    return arr


def tune_placement(implicit: ImplicitFineGrid, ops, levels, k: int, steps: int = 3, trials: int = 8, extra: int = 2):
    """hmg_level_tune_placement: which memory block plays x, b, r, p, Ap of levels[k-1] is chosen by timing level k's share
    of a V-cycle (down + up half, levels[k-2] as the coarse side) per candidate assignment.  Call it on fresh states: the
    vectors of both levels come back zero-filled.  Returns (ms before, ms after)."""
    ops[k - 1]._bind()
    ms = (ctypes.c_double * 2)()
    L.check(L.load().hmg_level_tune_placement(implicit.h, k, int(steps), _state_handles(levels), int(extra), int(trials), ms))
    return ms[0], ms[1]


def vcycle_down(implicit: ImplicitFineGrid, ops, levels, k: int, steps: int = 2):
    """First half of one level of vcycle! (src/multigrid.jl:100-106): smoothing_steps!, local_residual!,
    restrict_to!(next.b, P, curr.r), fill!(next.x, 0).  Only levels[k-1] and levels[k-2] are touched (other entries
    may be None); p and Ap of level k are scratch afterwards."""
    ops[k - 1]._bind()
    L.check(L.load().hmg_vcycle_down(implicit.h, k, steps, _state_handles(levels)))


def vcycle_up(implicit: ImplicitFineGrid, ops, levels, k: int, steps: int = 2):
    """Second half (src/multigrid.jl:112-115): interpolate_and_sum_to!(curr.x, P, next.x), smoothing_steps!."""
    ops[k - 1]._bind()
    L.check(L.load().hmg_vcycle_up(implicit.h, k, steps, _state_handles(levels)))
