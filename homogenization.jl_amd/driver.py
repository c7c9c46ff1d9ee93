"""
Host-side driver pieces (level L4 of the reference: src/examples/homogenized_coefficients.jl) that sit
on either side of the hot path: base-mesh synthesis, the infinity-norm ordering that makes a domain
shrink a prefix operation, the checkerboard coefficient field and the `checkerboard_homogenization`
loop itself.  All level-vector work goes to the device through api.py; nothing here touches a level
vector on the host.
"""
from __future__ import annotations

import contextlib
import math
import os
import warnings

import numpy as np

from . import api, fields as cell_fields, vtk
from .api import Mesh, Tet64, Tri64

_CUBE_TETS = ((0, 1, 2, 6), (0, 1, 4, 6), (1, 3, 2, 6), (1, 3, 6, 7), (1, 5, 4, 6), (1, 5, 6, 7))


def hypercube(eltype, n: int, scale=1.0, origin=None) -> Mesh:
    """n^d unit cubes, each split into 6 tetrahedra (3D) / 2 triangles (2D); numbering as the reference's
    `hypercube` (src/tet/generate_grid.jl:6-45, src/tri/generate_grid.jl:6-35): node ids run with the last
    coordinate fastest, cell corners are looked up through a first-index-fastest id table."""
    dim = api._dim_of(eltype)
    origin = np.ones(dim) if origin is None else np.asarray(origin, dtype=np.float64)
    k = n + 1
    # node q (0-based) has multi-index (q // k^(d-1), ..., q % k): last coordinate fastest
    grid = np.indices((k,) * dim).reshape(dim, -1).T.astype(np.float64)
    nodes = scale * grid + origin
    # corner lookup: id(a, b, c) = a + k*b + k^2*c
    strides = k ** np.arange(dim)
    cube = np.indices((n,) * dim).reshape(dim, -1).T                      # first index slowest
    corner = np.array([[(c >> a) & 1 for a in range(dim)] for c in range(2 ** dim)])   # bit a -> +1 in axis a
    ids = (cube[:, None, :] + corner[None, :, :]) @ strides               # (ncubes, 2^dim)
    if dim == 3:
        cells = ids[:, np.array(_CUBE_TETS)].reshape(-1, 4)
    else:
        cells = ids[:, np.array(((0, 1, 2), (1, 2, 3)))].reshape(-1, 3)
    cells = np.sort(cells, axis=1) + 1                                     # 1-based, ascending tuples
    return Mesh(nodes, cells.astype(np.int64))


def box_mesh(eltype, shape, scale=1.0, origin=None) -> Mesh:
    """A box of shape[0] x shape[1] (x shape[2]) unit cubes, each split into 6 tetrahedra / 2 triangles around
    one diagonal like `hypercube` (node ids run with the last coordinate fastest).  Used for multi-GPU weak
    scaling, where the global domain is a brick of per-rank cubes; not a reference entry point."""
    dim = api._dim_of(eltype)
    shape = tuple(int(v) for v in shape)
    assert len(shape) == dim
    origin = np.ones(dim) if origin is None else np.asarray(origin, dtype=np.float64)
    k = np.array(shape) + 1
    grid = np.indices(tuple(k)).reshape(dim, -1).T.astype(np.float64)
    nodes = scale * grid + origin
    strides = np.concatenate([[1], np.cumprod(k[:-1])])
    cube = np.indices(shape).reshape(dim, -1).T
    corner = np.array([[(c >> a) & 1 for a in range(dim)] for c in range(2 ** dim)])
    ids = (cube[:, None, :] + corner[None, :, :]) @ strides
    # node ids run with the LAST coordinate fastest, the lookup table with the FIRST: translate
    lut = np.ravel_multi_index(np.unravel_index(np.arange(int(np.prod(k))), tuple(k), order="F"), tuple(k), order="C")
    ids = lut[ids]
    if dim == 3:
        cells = ids[:, np.array(_CUBE_TETS)].reshape(-1, 4)
    else:
        cells = ids[:, np.array(((0, 1, 2), (1, 2, 3)))].reshape(-1, 3)
    return Mesh(nodes, (np.sort(cells, axis=1) + 1).astype(np.int64))


def checkerboard_mesh(eltype, shape, origin=None, transposed_lookup=None, ordered: bool = True) -> Mesh:
    """`hypercube` / `box_mesh` (+ `order_nodes_and_elements_by_magnitude` if `ordered`) by the library's threaded host
    code (hmg_checkerboard_mesh): the same arrays as the numpy functions here, which stay as the readable statement
    of the rule and as the test reference.  transposed_lookup: None = like `hypercube` for cubes, like `box_mesh` else."""
    import ctypes
    from . import _lib as L
    lib = L.load()
    dim = api._dim_of(eltype)
    shape = np.ascontiguousarray([int(v) for v in (shape if np.ndim(shape) else (shape,) * dim)], dtype=np.int64)
    assert shape.size == dim
    origin = np.ones(dim) if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    if transposed_lookup is None:
        transposed_lookup = bool(np.all(shape == shape[0]))
    nn, nc = ctypes.c_int64(), ctypes.c_int64()
    L.check(lib.hmg_checkerboard_mesh_size(dim, shape.ctypes.data_as(L.p_i64), ctypes.byref(nn), ctypes.byref(nc)))
    nodes = np.empty((nn.value, dim), dtype=np.float64)
    cells = np.empty((nc.value, dim + 1), dtype=np.int64)
    L.check(lib.hmg_checkerboard_mesh(dim, shape.ctypes.data_as(L.p_i64), origin.ctypes.data_as(L.p_f64),
                                      1 if transposed_lookup else 0, 1 if ordered else 0,
                                      nodes.ctypes.data_as(L.p_f64), cells.ctypes.data_as(L.p_i64)))
    return Mesh(nodes, cells)


def _infnorm(a):
    return np.abs(a).max(axis=-1)


def _centers(mesh: Mesh):
    p = mesh.nodes[mesh.elements - 1]
    acc = p[:, 0, :].copy()
    for i in range(1, p.shape[1]):
        acc += p[:, i, :]
    return acc / p.shape[1]


def order_nodes_and_elements_by_magnitude(mesh: Mesh) -> Mesh:
    """Nodes and cells sorted by infinity-norm distance to the origin (stable), so that every centred
    sub-cube is a prefix.  ref: src/examples/homogenized_coefficients.jl:21-28"""
    perm = np.argsort(_infnorm(mesh.nodes), kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    cells = np.sort(inv[mesh.elements - 1], axis=1) + 1
    out = Mesh(mesh.nodes[perm], cells)
    order = np.argsort(_infnorm(_centers(out)), kind="stable")
    out.elements = np.ascontiguousarray(out.elements[order])
    return out


def find_elements_in_radius(mesh: Mesh, radius) -> int:
    return int(np.searchsorted(_infnorm(_centers(mesh)), radius, side="right"))


def find_nodes_in_radius(mesh: Mesh, radius) -> int:
    return int(np.searchsorted(_infnorm(mesh.nodes), radius + 10 * np.finfo(float).eps, side="right"))


def compute_boundary_layer(lam: float, n: int) -> int:
    return int(math.floor(4 * (n + 1) * lam ** -0.5))


def compute_box_radius(k: int, n: int, eps: float = 0.0) -> int:
    return int(math.floor(2.0 ** (n - k * (0.5 - eps))))


def generate_conductivity(dim: int, n: int, seed: int, values=(1.0, 9.0)):
    """One diagonal tensor per unit cube, every entry i.i.d. in `values` (p = 1/2).  The reference draws
    from the unseeded global RNG with values {1, 9} (src/examples/homogenized_coefficients.jl:485-488);
    here the field is seeded and the contrast is a parameter."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((n,) * dim + (dim,)) < 0.5, values[0], values[1])


def generate_polycrystal(dim: int, n: int, seed: int, principal=None):
    """One grain per unit cube: sigma = R diag(principal) R^T with one rotation R per cube -- 2D: the angle uniform in [0, pi);
    3D: a uniform random rotation (a unit quaternion from four normal deviates).  Shape (n,) * dim + (dim, dim), exactly
    symmetric: a `sigma_grid` for the drivers.  principal defaults to (1, 9) / (1, 9, 100)."""
    principal = np.asarray((1.0, 9.0, 100.0)[:dim] if principal is None else principal, dtype=np.float64)
    if principal.shape != (dim,):
        raise ValueError(f"principal must hold {dim} conductivities")
    rng = np.random.default_rng(seed)
    ncube = n ** dim
    if dim == 2:
        t = rng.random(ncube) * math.pi
        c, s = np.cos(t), np.sin(t)
        R = np.stack([np.stack([c, -s], axis=-1), np.stack([s, c], axis=-1)], axis=-2)
    else:
        q = rng.standard_normal((ncube, 4))
        w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=-1),
                      np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=-1),
                      np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)], axis=-2)
    S = np.einsum("cik,k,cjk->cij", R, principal, R)
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    return np.ascontiguousarray(S.reshape((n,) * dim + (dim, dim)))


def conductivity_per_element(mesh: Mesh, sigma_grid, offset, native: bool = True):
    """ref: src/examples/homogenized_coefficients.jl:494-503 (native: the library's threaded host code; False: numpy).  A grid of
    full tensors, shape (n,) * dim + (dim, dim) (generate_polycrystal), takes the numpy path and gives (ncells, dim, dim)."""
    if native and np.ndim(sigma_grid) == mesh.dim + 1:
        from . import _lib as L
        dim = mesh.dim
        nodes = np.ascontiguousarray(mesh.nodes, dtype=np.float64)
        cells = np.ascontiguousarray(mesh.elements, dtype=np.int64)
        sg = np.ascontiguousarray(sigma_grid, dtype=np.float64)
        assert sg.ndim == dim + 1 and sg.shape[-1] == dim
        gs = np.ascontiguousarray(sg.shape[:dim], dtype=np.int64)
        off = np.ascontiguousarray(offset, dtype=np.float64)
        out = np.empty((cells.shape[0], dim), dtype=np.float64)
        L.check(L.load().hmg_conductivity_per_element(dim, nodes.shape[0], nodes.ctypes.data_as(L.p_f64), cells.shape[0],
                                                      cells.ctypes.data_as(L.p_i64), gs.ctypes.data_as(L.p_i64),
                                                      sg.ctypes.data_as(L.p_f64), off.ctypes.data_as(L.p_f64),
                                                      out.ctypes.data_as(L.p_f64)))
        return out
    idx = np.trunc(_centers(mesh) + np.asarray(offset, dtype=np.float64)).astype(np.int64) - 1
    return np.ascontiguousarray(np.asarray(sigma_grid)[tuple(idx[:, a] for a in range(mesh.dim))])


def random_unit_vec(dim):
    v = np.ones(dim)
    return v / np.linalg.norm(v)


def checkerboard_problem(ctx, eltype, width: int, levels: int, seed: int = 0, values=(1.0, 9.0), lam: float = 1.0,
                         origin=None, ordered: bool = True):
    """Base mesh, coefficient field, implicit grid and operator for a width^d checkerboard."""
    dim = api._dim_of(eltype)
    if origin is None:
        origin = (-width / 2.0,) * dim
    base = checkerboard_mesh(eltype, width, origin=origin, transposed_lookup=True, ordered=ordered)
    sgrid = generate_conductivity(dim, width, seed, values)
    cond = conductivity_per_element(base, sgrid, tuple(1.0 - o for o in origin))
    implicit = api.ImplicitFineGrid(ctx, base, levels)
    op = api.L2PlusDivAGrad(implicit, lam, cond)
    return base, cond, implicit, op


def checkerboard_homogenization(n: int = 4, eltype=Tri64, refinements: int = 2, smoothing_steps: int = 3,
                                tolerance: float = 1e-4, xi=None, save=None, *, ctx=None, seed: int = 0,
                                values=(1.0, 9.0), sigma_grid=None, x0=None, max_cycles: int = 1000, log=None,
                                timings: dict | None = None, tune_placement: int = 0, accelerate: bool = False,
                                smoother: str = "cg"):
    """checkerboard_homogenization(n, type; refinements, smoothing_steps, tolerance, xi, save) -> sigma
    (src/examples/homogenized_coefficients.jl:174-343) with every level-vector operation on the device.

    Differences to the reference, all explicit: the coefficient field and the initial guess are seeded
    (`seed`, or passed in as `sigma_grid` / `x0`) instead of drawn from the global RNG; `save` (a level, as in the
    reference: checkerboard.vtu + one ahom_k.vtu per outer step, see vtk.py) may also be a (level, directory) pair;
    the level-1 solve is the library's PCG; a domain shrink keeps the level vectors in place
    (their columns are a prefix) instead of copying slices.  Returns (sigma, history) where history holds
    (k, cycle, norm(r), sigma + dsigma, |dsigma - dsigma_prev|) -- the three quantities the reference logs.
    `timings` (a dict) receives wall-clock seconds: "setup_s" (mesh, tables, level vectors, x0, right-hand side -- up to
    the first V-cycle), "solve_s" (everything after), "vcycles", "outer_steps", "cells", and "inexact_vcycles": V-cycles whose
    level-1 solve ran out of its iteration budget (each also raises a warning; 0 in every recorded run).
    `tune_placement` = T > 0: the finest level's five memory blocks are assigned to their roles by measurement
    (api.tune_placement, T candidates; pays off for long runs only -- about 0.1 s per candidate at config 3).
    `accelerate` = True: the V-cycle preconditions a flexible CG iteration (api.FlexibleCG) instead of being repeated as it is: one
    `start` per outer step, one `step` per cycle; the same integrals, stopping rule and history (entry 2 is the norm of the true
    residual), "vcycles" counts the iterations.  Four more vectors of the finest level's size: the iterate (the finest level's own
    x holds the preconditioned residual; its b keeps the right-hand side, which `integrate_first_term` reads at k = 0) and the
    method's p, q, R.  At tolerances far above rounding the two forms stop at iterates that differ by about the tolerance.
    `smoother` = "jacobi": the V-cycle's smoother is CG preconditioned by the inverse diagonal of the assembled operator
    (api.set_smoother; one more vector per level >= 2) instead of the reference's CG ("cg").  Fewer cycles at high contrast, about
    1.5 times the traffic per cycle; combines freely with `accelerate`; reported in timings["smoother"].
    `smoother` = "chebyshev": a Chebyshev polynomial in that inverse diagonal times the operator, with the library's own bound per
    level and its default ratio -- no dot products, one apply fewer per smoothing inside the V-cycle; the same memory as "jacobi"."""
    import time
    t_start = time.perf_counter()
    save_dir = "."
    if isinstance(save, tuple):
        save, save_dir = save
    dim = api._dim_of(eltype)
    own_ctx = ctx is None
    if own_ctx:
        ctx = api.Context(0)
    xi = random_unit_vec(dim) if xi is None else np.asarray(xi, dtype=np.float64)
    lam, sigma = 1.0, 0.0
    box_radius = compute_box_radius(0, n)
    boundary_layer = compute_boundary_layer(lam, n)
    total_radius = box_radius + boundary_layer
    width = 2 * total_radius
    base = checkerboard_mesh(eltype, width, origin=(-float(total_radius),) * dim, transposed_lookup=True)
    if sigma_grid is None:
        sigma_grid = generate_conductivity(dim, width, seed, values)
    cond = conductivity_per_element(base, sigma_grid, (total_radius + 1.0,) * dim)
    t_mesh = time.perf_counter()
    total_grids = refinements + 1
    if save is not None:
        if not 1 <= save <= total_grids:
            raise ValueError("save must be a level in 1..refinements+1")
        vtk.export_domain(base, cond, os.path.join(save_dir, "checkerboard"))
    implicit = api.ImplicitFineGrid(ctx, base, total_grids)
    implicit.set_smoother(smoother)                      # (before the level vectors: the "cg" forms reserve a spare one with them)
    op = api.L2PlusDivAGrad(implicit, lam, cond)
    ops = [op] * total_grids
    t_grid = time.perf_counter()
    states = [api.LevelState(implicit, i + 1) for i in range(total_grids)]
    top = states[-1]
    if tune_placement:
        tuned = api.tune_placement(implicit, ops, states, total_grids, smoothing_steps, trials=int(tune_placement))
        if timings is not None:
            timings["tune_ms"] = tuned
    xv = api.DeviceMatrix(implicit, total_grids) if accelerate else top.x      # the iterate
    fcg = api.FlexibleCG(implicit, None, ops, states, total_grids, smoothing_steps) if accelerate else None
    ctx.sync()
    t_alloc = time.perf_counter()
    if x0 is None:
        xv.rand(seed + 1)
    else:
        xv.from_host(x0)
    api.broadcast_interfaces(xv, implicit, total_grids)
    api.apply_constraint(xv, total_grids, implicit)
    api.rhs_axi_grad_v(top.b, implicit, xi)
    v_prev = None                                        # allocated at the first domain shrink (10 GB at config 3)
    cur = base
    history = []
    inexact = 0                                          # V-cycles whose budgeted level-1 solve missed coarse_rtol
    ctx.sync()
    t_setup = time.perf_counter()
    for k in range(n + 1):
        base_level = api.BaseLevel(implicit)             # level-1 operator for the current lam / domain
        dsig, dsig_prev = 0.0, 0.0
        if accelerate:
            fcg.start(xv, top.b)                         # new boundary, new lam, new right-hand side: a new residual
        for i in range(1, max_cycles + 1):
            if not (fcg.step_tolerant() if accelerate else
                    api.vcycle_tolerant(implicit, base_level, ops, states, total_grids, smoothing_steps)):
                # the level-1 solve ran out of its blind iteration budget: this cycle's coarse-grid correction was inexact (a weaker
                # but valid iterate; the library counts the next solve again).  The reference's CHOLMOD solve cannot miss -- say so.
                inexact += 1
                warnings.warn(f"checkerboard_homogenization: V-cycle {i} of outer step {k} used an inexact level-1 solve "
                              f"({inexact} so far)")
            nint = find_elements_in_radius(cur, box_radius)
            area = api.integrate_area(xv, implicit, nint)
            if k == 0:
                integral = api.integrate_first_term(xv, implicit, nint, xi, b=top.b)   # b = rhs_a.xi.grad(v) at k = 0
            else:
                integral = api.integrate_terms(xv, v_prev, implicit, nint)
            dsig = 2.0 ** k * integral / area
            rnorm = fcg.residual_norm() if accelerate else api.norm_unique(top.r)
            history.append((k, i, rnorm, sigma + dsig, abs(dsig - dsig_prev)))
            if log:
                log(history[-1])
            if abs(dsig - dsig_prev) < tolerance:
                break
            dsig_prev = dsig
        sigma += dsig
        if save is not None:                             # ref: ...homogenized_coefficients.jl:303
            vtk.export_unknown(implicit, xv, k, save, os.path.join(save_dir, f"ahom_{k}"))
        lam /= 2
        box_radius = compute_box_radius(k + 1, n)
        boundary_layer = compute_boundary_layer(lam, n)
        if box_radius + boundary_layer > total_radius:
            break
        total_radius = box_radius + boundary_layer
        nn_keep = find_nodes_in_radius(cur, total_radius)
        ne_keep = find_elements_in_radius(cur, total_radius)
        cur = Mesh(cur.nodes[:nn_keep], np.ascontiguousarray(cur.elements[:ne_keep]))
        implicit.shrink(ne_keep, nn_keep)                # new boundary; level vectors keep their storage
        api.apply_constraint(xv, total_grids, implicit)
        if v_prev is None:
            v_prev = api.DeviceMatrix(top.x.implicit, total_grids)
        v_prev.copyto(xv)
        op.lam = lam
        api.next_rhs(top.b, xv, implicit)
    ctx.sync()
    if timings is not None:
        timings.update(setup_s=t_setup - t_start, setup_mesh_s=t_mesh - t_start, setup_tables_s=t_grid - t_mesh,
                       setup_alloc_s=t_alloc - t_grid, setup_init_s=t_setup - t_alloc,
                       solve_s=time.perf_counter() - t_setup, vcycles=len(history),
                       outer_steps=len({h[0] for h in history}), cells=int(base.elements.shape[0]), width=int(width),
                       inexact_vcycles=inexact, smoother=smoother)
    # the level vectors go back now, not whenever the collector gets to them (71 GB at BASELINE config 3)
    if accelerate:
        fcg.close()
        xv.close()
    for st in states:
        st.close()
    if v_prev is not None:
        v_prev.close()
    implicit.close()
    if own_ctx:
        ctx.close()
    return sigma, history


def pair_increments(V, Vprev, k, nint, area, implicit, scratch, rank_sum=None):
    """The off-diagonal increments 2^k I_k^{ij} / area of the homogenized tensor from the correctors V[i] = v_k^i of one outer
    step (Vprev[i] = v_{k-1}^i under the step's constraint; unused at k = 0), as a symmetric matrix with a zero diagonal:

        k = 0    I^{ij} = 1/2 [Lq(v^i; b^j) + Lq(v^j; b^i)] + Mq(v^i; v^j),    b^j = rhs_a.e_j.grad(v), regenerated into `scratch`
        k >= 1   I^{ij} = Mq(v_k^i; v_k^j) + 1/2 [Mq(v_k^j; v_{k-1}^i) + Mq(v_k^i; v_{k-1}^j)]

    (Mq = api.integrate_pair_mass, Lq = api.integrate_pair_load; for i = j these are integrate_first_term / integrate_terms, which
    the cycle loops have formed already).  rank_sum: the sum over the ranks of a partitioned grid (one call for all pairs)."""
    dim = len(V)
    pairs = [(i, j) for i in range(dim) for j in range(i + 1, dim)]
    val = dict.fromkeys(pairs, 0.0)
    if k == 0:
        for j in range(dim):
            api.rhs_axi_grad_v(scratch, implicit, np.eye(dim)[j])
            for i in range(dim):
                if i != j:
                    val[min(i, j), max(i, j)] += 0.5 * api.integrate_pair_load(V[i], scratch, implicit, nint)
    for i, j in pairs:
        val[i, j] += api.integrate_pair_mass(V[i], V[j], implicit, nint)
        if k > 0:
            val[i, j] += 0.5 * (api.integrate_pair_mass(V[j], Vprev[i], implicit, nint) +
                                api.integrate_pair_mass(V[i], Vprev[j], implicit, nint))
    if rank_sum is not None and pairs:
        val = dict(zip(pairs, rank_sum(*[val[p] for p in pairs])))
    out = np.zeros((dim, dim))
    for (i, j), v in val.items():
        out[i, j] = out[j, i] = 2.0 ** k * v / area
    return out


def checkerboard_homogenization_tensor(n: int = 4, eltype=Tri64, refinements: int = 2, smoothing_steps: int = 3,
                                       tolerance: float = 1e-4, save=None, *, ctx=None, seed: int = 0, values=(1.0, 9.0),
                                       sigma_grid=None, x0=None, max_cycles: int = 1000, log=None,
                                       timings: dict | None = None, tune_placement: int = 0, accelerate: bool = False,
                                smoother: str = "cg"):
    """The full homogenized tensor from ONE run: -> (Sigma, history), Sigma a symmetric (dim, dim) array with
    xi' Sigma xi = what `checkerboard_homogenization(xi=xi)` returns once both have converged.  The keywords are those of
    `checkerboard_homogenization` without `xi` (`accelerate` and `smoother` included).

    The correctors are linear in the direction, so d corrector solves (e_1 .. e_d) are enough where polarising by hand takes
    d (d + 1) / 2 complete runs; the off-diagonal entries follow from cross integrals of the correctors (`pair_increments`:
    api.integrate_pair_mass / integrate_pair_load).  The radii and the shrink schedule do not depend on the direction, so all
    directions share the outer loop: base mesh, grid, operator, level states, the optional flexible-CG object and the BaseLevel
    of an outer step are built once.  Within outer step k, direction by direction: the right-hand side is rhs_a.e_i.grad(v) at
    k = 0 and next_rhs of v_{k-1}^i afterwards, the start vector the seeded x0 at k = 0 (the same for every direction) and
    v_{k-1}^i under the new constraint afterwards; cycle loop, stopping rule on the diagonal increment, the handling of an inexact
    level-1 solve and the residual norm are those of the scalar driver, and Sigma_ii accumulates exactly the increments that loop
    forms.  After the last direction the off-diagonal increments are formed, then the domain shrinks, the handles of v_k and
    v_{k-1} are exchanged and lam is halved.

    history rows: (k, direction, cycle, norm(r), Sigma_ii so far, |change of the increment|).  `timings` receives the scalar
    driver's entries plus "directions" and "pair_integrals_s"; `save` writes one ahom_<k>_<i>.vtu per step and direction.

    Memory beyond the scalar driver, in vectors of the finest level's size: d always (v_k^i), d more from the first shrink on
    (v_{k-1}^i; the scalar driver's v_prev is among them), none for b^j (the finest level's own b is free once the last direction
    of a step has converged).  At BASELINE config 3 (d = 3; outer step 0 is its only step) that is about 31 GB next to 61 GB of
    level vectors."""
    import time
    t_start = time.perf_counter()
    save_dir = "."
    if isinstance(save, tuple):
        save, save_dir = save
    dim = api._dim_of(eltype)
    own_ctx = ctx is None
    if own_ctx:
        ctx = api.Context(0)
    lam = 1.0
    Sigma = np.zeros((dim, dim))
    box_radius = compute_box_radius(0, n)
    boundary_layer = compute_boundary_layer(lam, n)
    total_radius = box_radius + boundary_layer
    width = 2 * total_radius
    base = checkerboard_mesh(eltype, width, origin=(-float(total_radius),) * dim, transposed_lookup=True)
    if sigma_grid is None:
        sigma_grid = generate_conductivity(dim, width, seed, values)
    cond = conductivity_per_element(base, sigma_grid, (total_radius + 1.0,) * dim)
    t_mesh = time.perf_counter()
    total_grids = refinements + 1
    if save is not None:
        if not 1 <= save <= total_grids:
            raise ValueError("save must be a level in 1..refinements+1")
        vtk.export_domain(base, cond, os.path.join(save_dir, "checkerboard"))
    implicit = api.ImplicitFineGrid(ctx, base, total_grids)
    implicit.set_smoother(smoother)                      # (before the level vectors: the "cg" forms reserve a spare one with them)
    op = api.L2PlusDivAGrad(implicit, lam, cond)
    ops = [op] * total_grids
    t_grid = time.perf_counter()
    states = [api.LevelState(implicit, i + 1) for i in range(total_grids)]
    top = states[-1]
    if tune_placement:
        tuned = api.tune_placement(implicit, ops, states, total_grids, smoothing_steps, trials=int(tune_placement))
        if timings is not None:
            timings["tune_ms"] = tuned
    xv = api.DeviceMatrix(implicit, total_grids) if accelerate else top.x      # the iterate
    fcg = api.FlexibleCG(implicit, None, ops, states, total_grids, smoothing_steps) if accelerate else None
    V = [api.DeviceMatrix(implicit, total_grids) for _ in range(dim)]          # v_k^i
    Vprev = None                                         # v_{k-1}^i: allocated at the first domain shrink
    ctx.sync()
    t_alloc = time.perf_counter()
    cur = base
    history = []
    inexact = 0                                          # V-cycles whose budgeted level-1 solve missed coarse_rtol
    t_pairs = 0.0
    t_setup = t_alloc                                    # (x0 and the right-hand sides belong to the directions' solves)
    for k in range(n + 1):
        base_level = api.BaseLevel(implicit)             # level-1 operator for the current lam / domain: one per outer step
        nint = find_elements_in_radius(cur, box_radius)
        for d in range(dim):
            if k == 0:
                if x0 is None:
                    xv.rand(seed + 1)
                else:
                    xv.from_host(x0)
                api.broadcast_interfaces(xv, implicit, total_grids)
                api.apply_constraint(xv, total_grids, implicit)
                api.rhs_axi_grad_v(top.b, implicit, np.eye(dim)[d])
            else:
                xv.copyto(Vprev[d])                      # v_{k-1}^i, the new constraint applied at the shrink
                api.next_rhs(top.b, xv, implicit)
            dsig, dsig_prev = 0.0, 0.0
            if accelerate:
                fcg.start(xv, top.b)
            for i in range(1, max_cycles + 1):
                if not (fcg.step_tolerant() if accelerate else
                        api.vcycle_tolerant(implicit, base_level, ops, states, total_grids, smoothing_steps)):
                    inexact += 1                         # (as in checkerboard_homogenization: counted and said)
                    warnings.warn(f"checkerboard_homogenization_tensor: V-cycle {i} of outer step {k}, direction {d}, used an "
                                  f"inexact level-1 solve ({inexact} so far)")
                area = api.integrate_area(xv, implicit, nint)
                if k == 0:
                    integral = api.integrate_first_term(xv, implicit, nint, np.eye(dim)[d], b=top.b)
                else:
                    integral = api.integrate_terms(xv, Vprev[d], implicit, nint)
                dsig = 2.0 ** k * integral / area
                rnorm = fcg.residual_norm() if accelerate else api.norm_unique(top.r)
                history.append((k, d, i, rnorm, Sigma[d, d] + dsig, abs(dsig - dsig_prev)))
                if log:
                    log(history[-1])
                if abs(dsig - dsig_prev) < tolerance:
                    break
                dsig_prev = dsig
            Sigma[d, d] += dsig
            V[d].copyto(xv)
            if save is not None:
                vtk.export_unknown(implicit, xv, k, save, os.path.join(save_dir, f"ahom_{k}_{d}"))
        t0 = time.perf_counter()
        Sigma += pair_increments(V, Vprev, k, nint, api.integrate_area(xv, implicit, nint), implicit, top.b)
        t_pairs += time.perf_counter() - t0
        lam /= 2
        box_radius = compute_box_radius(k + 1, n)
        boundary_layer = compute_boundary_layer(lam, n)
        if box_radius + boundary_layer > total_radius:
            break
        total_radius = box_radius + boundary_layer
        nn_keep = find_nodes_in_radius(cur, total_radius)
        ne_keep = find_elements_in_radius(cur, total_radius)
        cur = Mesh(cur.nodes[:nn_keep], np.ascontiguousarray(cur.elements[:ne_keep]))
        implicit.shrink(ne_keep, nn_keep)                # new boundary; level vectors keep their storage
        for v in V:
            api.apply_constraint(v, total_grids, implicit)
        if Vprev is None:
            Vprev = [api.DeviceMatrix(implicit, total_grids) for _ in range(dim)]
        V, Vprev = Vprev, V                              # the handles change places: nothing is copied
        op.lam = lam
    ctx.sync()
    if timings is not None:
        timings.update(setup_s=t_setup - t_start, setup_mesh_s=t_mesh - t_start, setup_tables_s=t_grid - t_mesh,
                       setup_alloc_s=t_alloc - t_grid, setup_init_s=t_setup - t_alloc,
                       solve_s=time.perf_counter() - t_setup, vcycles=len(history),
                       outer_steps=len({h[0] for h in history}), cells=int(base.elements.shape[0]), width=int(width),
                       inexact_vcycles=inexact, directions=dim, pair_integrals_s=t_pairs, smoother=smoother)
    if accelerate:
        fcg.close()
        xv.close()
    for st in states:
        st.close()
    for v in V + (Vprev or []):
        v.close()
    implicit.close()
    if own_ctx:
        ctx.close()
    return Sigma, history


def checkerboard_hypercube_multigrid(n: int, eltype=Tet64, refinements: int = 2, max_cycles: int = 5, save=None, *,
                                     ctx=None, seed: int = 1, sigma_grid=None, x0=None, smoother: str = "cg"):
    """checkerboard_hypercube_multigrid(n, elementtype, refinements, max_cycles, save) -> residual norms
    (src/examples/homogenized_coefficients.jl:509-571): -div(a grad u) = 1 with zero Dirichlet data (lambda = 0),
    `max_cycles` V-cycles with 3 smoothing steps; `refinements` is the number of grids.  Seeded like the other
    driver; `save` = level (or (level, directory)) writes checkerboard_full_<refinements>.vtu with point data "x";
    `smoother` = "cg" (the reference's), "jacobi" or "chebyshev" (api.set_smoother).
    Returns (rs, state of the finest level, implicit grid)."""
    dim = api._dim_of(eltype)
    own_ctx = ctx is None
    if own_ctx:
        ctx = api.Context(0)
    base = hypercube(eltype, n)
    if sigma_grid is None:
        sigma_grid = generate_conductivity(dim, n, seed)
    cond = conductivity_per_element(base, sigma_grid, (0.0,) * dim)
    implicit = api.ImplicitFineGrid(ctx, base, refinements)
    implicit.set_smoother(smoother)
    op = api.L2PlusDivAGrad(implicit, 0.0, cond)
    base_level = api.BaseLevel(implicit)
    states = [api.LevelState(implicit, i + 1) for i in range(refinements)]
    top = states[-1]
    if x0 is None:
        top.x.rand(seed + 1)
    else:
        top.x.from_host(x0)
    api.broadcast_interfaces(top.x, implicit, refinements)
    api.apply_constraint(top.x, refinements, implicit)
    api.local_rhs(top.b, implicit)
    rs = []
    for _ in range(max_cycles):
        api.vcycle(implicit, base_level, [op] * refinements, states, refinements, 3)
        rs.append(api.norm_unique(top.r))
    if save is not None:
        save_dir = "."
        if isinstance(save, tuple):
            save, save_dir = save
        vtk.export_unknown(implicit, top.x, 0, save, os.path.join(save_dir, f"checkerboard_full_{refinements}"),
                           field="x")
    if own_ctx:
        ctx.sync()
    return rs, top, implicit


def _dirichlet_solve(implicit, op, base_level, states, xv, fcg, xi, smoothing_steps, tolerance, max_cycles, who):
    """One corrector of the plain Dirichlet cell problem, the solve loop `dirichlet_homogenization` and
    `dirichlet_homogenization_tensor` share: the iterate `xv` starts at zero, the right-hand side of the finest state becomes
    rhs_a.xi.grad(v), and V-cycles (`fcg` None) or flexible-CG steps run until the first-copy norm of the residual has fallen by
    `tolerance` from its initial value or is rounding noise of the loads.  Returns (cycles, norm(r), initial norm(r))."""
    total_grids = len(states)
    ops = [op] * total_grids
    top = states[-1]
    accelerate = fcg is not None
    xv.fill(0.0)
    api.rhs_axi_grad_v(top.b, implicit, xi)

    def residual_norm():
        if accelerate:
            return fcg.residual_norm()
        api.local_residual(implicit, op, top, total_grids)                    # r = b - A_loc x, Dirichlet rows zero
        api.broadcast_interfaces(top.r, implicit, total_grids)
        return api.norm_unique(top.r)

    if accelerate:
        fcg.start(xv, top.b)
    r0 = residual_norm()
    noise = 1e-13 * api.norm(top.b)                  # the loads of a uniform medium cancel in the interface sum up to rounding
    rnorm, cycles = r0, 0
    while rnorm > max(tolerance * r0, noise) and cycles < max_cycles:
        ok = fcg.step_tolerant() if accelerate else api.vcycle_tolerant(implicit, base_level, ops, states, total_grids,
                                                                        smoothing_steps)
        if not ok:
            warnings.warn(f"{who}: cycle {cycles + 1} used an inexact level-1 solve")
        cycles += 1
        rnorm = residual_norm()
    if rnorm > max(tolerance * r0, noise):
        warnings.warn(f"{who}: residual {rnorm / r0:.3e} of its initial value after {cycles} cycles")
    return cycles, rnorm, r0


@contextlib.contextmanager
def _large_cells(ctx, on: bool):
    """Around the per-cell passes of the Dirichlet drivers: with `on`, the context options "cell_moments_windows",
    "cell_extrema_windows" and "cell_histogram_windows" are at least 1 inside (cells larger than the LDS -- 3D level 7, 2D levels
    9-11 -- go through the window kernels of the moments, of the extrema and of the histograms) and back at their previous values
    behind, also when a pass raises.  The context may be the caller's."""
    if not on:
        yield
        return
    names = ("cell_moments_windows", "cell_extrema_windows", "cell_histogram_windows")
    prev = {name: ctx.counter(name) for name in names}
    try:
        for name in names:
            if prev[name] == 0:
                ctx.set_option(name, 1)
        yield
    finally:
        for name in names:
            ctx.set_option(name, prev[name])


def _histogram_rule(histogram):
    """The `histogram` argument of dirichlet_homogenization as keywords of api.cell_histogram: None / False -> None, True -> the
    default rule, a dict of "emin", "emax" and, optionally, "sub_bits" -> itself, checked (api.histogram_nbins refuses parameters
    outside the rule, and the driver more bins than api.cell_histogram serves, before anything is solved)."""
    if histogram is None or histogram is False:
        return None
    if histogram is True:
        rule = {"emin": -24, "emax": 8, "sub_bits": 3}
    else:
        rule = dict(histogram)
        if not {"emin", "emax"} <= set(rule) <= {"emin", "emax", "sub_bits"}:
            raise ValueError('histogram must be True or a dict of "emin", "emax" and, optionally, "sub_bits"')
        rule = {"emin": int(rule["emin"]), "emax": int(rule["emax"]), "sub_bits": int(rule.get("sub_bits", 3))}
    if api.histogram_nbins(**rule) > 1027:
        raise ValueError("histogram: api.cell_histogram serves at most 1024 regular bins ((emax - emin) 2^sub_bits)")
    return rule


def dirichlet_homogenization(n: int, eltype=Tri64, refinements: int = 2, xi=None, *, ctx=None, sigma_grid=None, seed: int = 0,
                             values=(1.0, 9.0), tolerance: float = 1e-10, smoother: str = "cg", accelerate: bool = False,
                             fields: bool = False, save=None, cond=None, smoothing_steps: int = 3, max_cycles: int = 200,
                             large_cells: bool = False, extrema: bool = False, thresholds=None, slices=None,
                             locations: bool = False, histogram=None):
    """The plain Dirichlet cell problem on `hypercube(eltype, n)`: find v, zero on the boundary, with
    a(v, w) = -int sigma xi . grad w for all such w (lambda = 0), on `refinements` + 1 grids; then, from the per-cell gradient
    moments of u = xi.x + v (api.cell_moments), the row of the homogenized tensor in two forms:

        energy_form   sum_c sigma_c : G_u(c) / |Omega|           (= xi . Sigma xi)
        flux_form     sum_c |c| sigma_c m_u(c) / |Omega|         (= Sigma xi, a whole row from one corrector)

    They agree (energy_form = xi . flux_form) to the accuracy of the solve.  The right-hand side is `rhs_axi_grad_v`, the initial
    guess zero; V-cycles (or, `accelerate`, flexible-CG steps around them) run until the first-copy norm of the residual
    b - A v has fallen by `tolerance` from its initial value -- or at once if that is rounding noise of the loads (a uniform
    medium: v = 0).  `sigma_grid`: one tensor per unit cube, (n,) * dim + (dim,) diagonals or + (dim, dim) full tensors; default:
    the seeded checkerboard of `values`; `cond`: the conductivity per CELL instead, (Ne, dim) or (Ne, dim, dim), as a design or
    inverse loop moves it.  Returns a dict: "energy_form", "flux_form" (dim), "cycles", "residual" (relative),
    "volume"; with `fields` also "mean" (Ne, dim), "gram" (Ne, dim, dim), "flux", "energy", "volumes", "cond", "base".  `save` (a
    file name) writes the coarse mesh with those cell fields (vtk.export_cell_fields).  In this setting, and only in it,
    gram[c] is the exact sensitivity d(energy_form |Omega|) / d(sigma_c) (fields.sensitivity).  `large_cells`: the per-cell passes
    may run on a top level whose cell exceeds the LDS (3D level 7, 2D levels 9-11; context options "cell_moments_windows" and
    "cell_extrema_windows" = 1 around the passes, restored behind them); without it such a level is refused after the solve.
    `extrema`: a second pass, over the fine elements (api.cell_extrema with Q = sigma_c; top levels up to 6 in 3D and 8 in 2D,
    with `large_cells` 3D level 7 and 2D levels 9-11 too), adds "peak_energy_density" and
    "min_energy_density" (Ne each: the extrema of grad u . sigma_c grad u in every cell), "concentration" = peak / energy_form and,
    with `thresholds` (up to 8 multiples of energy_form), "exceedance" (Ne, nthr): the volume of every cell on which the energy
    density exceeds each; they are in the returned dict with or without `fields`, and with `save` in the file.
    `locations` (with `extrema`): the same pass also says where (api.cell_extrema_where; every other entry keeps its bits):
    "peak_location" and "min_location" (Ne, dim), the centroids of the fine elements that hold each cell's extrema (NaN for a cell
    whose extrema are NaN), and "hot_spots", the ten cells of highest peak, highest first (fields.hot_spots): a dict of "cell",
    "value", "point" and "sampled" -- the energy density of u sampled at each point on the device (api.sample), which is the
    value again up to rounding; with `save` the peaks also go to `save`_peaks.vtu as a point cloud (vtk.export_points).
    `slices`: a list of rasters (origin, du, dv, nu, nv) -- pixel (a, b) at origin + a du + b dv --; u = xi.x + v is sampled on each
    from the converged corrector on the device (api.sample_raster; any top level) and "slices" in the returned dict is a list of
    dicts with "value", "cell" (nv, nu), "gradient", "flux" (nv, nu, dim) and "energy_density" (nv, nu), NaN / -1 outside the
    domain; with `save` slice i is written to `save`_slice<i>.vts (vtk.export_slice).
    `histogram`: one more pass over the fine elements (api.cell_histogram with Q = sigma_c / energy_form: the bins are in units
    of the mean energy density and need no guessing) says how the energy density is distributed.  A dict of "emin", "emax",
    "sub_bits", or True for emin = -24, emax = 8, sub_bits = 3.  Adds "energy_density_histogram": a dict of "edges"
    (api.histogram_edges), "counts" (Ne, nbins) and "volume" (nbins: the volume of the domain per bin, fields.histogram_volume;
    fields.histogram_quantile reads medians and tails off it).  Top levels up to 6 in 3D and 8 in 2D; with `large_cells` 3D level 7
    and 2D levels 9-11 too ("cell_histogram_windows" = 1 around the pass), without it such a level is refused after the solve.
    Every other entry keeps its bits.  No counterpart in the reference."""
    dim = api._dim_of(eltype)
    own_ctx = ctx is None
    if own_ctx:
        ctx = api.Context(0)
    xi = random_unit_vec(dim) if xi is None else np.asarray(xi, dtype=np.float64)
    if xi.shape != (dim,):
        raise ValueError(f"xi must have {dim} entries")
    hist_rule = _histogram_rule(histogram)
    base = hypercube(eltype, n)
    if cond is None:
        if sigma_grid is None:
            sigma_grid = generate_conductivity(dim, n, seed, values)
        cond = conductivity_per_element(base, sigma_grid, (0.0,) * dim)
    else:
        cond = np.ascontiguousarray(cond, dtype=np.float64)
    total_grids = refinements + 1
    implicit = api.ImplicitFineGrid(ctx, base, total_grids)
    implicit.set_smoother(smoother)
    op = api.L2PlusDivAGrad(implicit, 0.0, cond)
    ops = [op] * total_grids
    base_level = api.BaseLevel(implicit)
    states = [api.LevelState(implicit, i + 1) for i in range(total_grids)]
    top = states[-1]
    xv = api.DeviceMatrix(implicit, total_grids) if accelerate else top.x      # the iterate (zero-filled)
    fcg = api.FlexibleCG(implicit, base_level, ops, states, total_grids, smoothing_steps) if accelerate else None
    cycles, rnorm, r0 = _dirichlet_solve(implicit, op, base_level, states, xv, fcg, xi, smoothing_steps, tolerance, max_cycles,
                                         "dirichlet_homogenization")
    with _large_cells(ctx, large_cells):
        mean, gram = api.cell_moments(xv, implicit, xi)
    vol = cell_fields.cell_volumes(base)
    omega = float(vol.sum())
    en = cell_fields.energy(cond, gram)
    out = {"energy_form": float(en.sum() / omega), "flux_form": cell_fields.flux_row(base, cond, mean), "cycles": cycles,
           "residual": float(rnorm / r0) if r0 > 0.0 else 0.0, "volume": omega}
    peaks = {}
    if extrema:
        thr = np.zeros(0) if thresholds is None else np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        call = api.cell_extrema_where if locations else api.cell_extrema
        with _large_cells(ctx, large_cells):
            qmax, qmin, counts, *where = call(xv, implicit, xi, cell_fields.energy_form(cond), thr * out["energy_form"])
        peaks = {"peak_energy_density": qmax, "min_energy_density": qmin,
                 "concentration": cell_fields.concentration(qmax, out["energy_form"])}
        if thr.size:
            peaks["exceedance"] = cell_fields.exceedance_volume(counts, vol, api.fine_elements(implicit, total_grids))
        if locations:
            cells = np.arange(qmax.shape[0])
            peaks["peak_location"] = cell_fields.element_centroids(implicit, total_grids, cells, where[0])
            peaks["min_location"] = cell_fields.element_centroids(implicit, total_grids, cells, where[1])
            hc, hv, hp = cell_fields.hot_spots(qmax, where[0], implicit, total_grids, k=10)
            here = ~np.isnan(hp).any(axis=1)
            sampled = np.full(hc.shape[0], np.nan)
            if here.any():
                s = api.sample(xv, implicit, hp[here], xi=xi, value=False)
                sampled[here] = cell_fields.sample_energy_density(cond, s["cell"], s["gradient"])
            out["hot_spots"] = {"cell": hc, "value": hv, "point": hp, "sampled": sampled}
            if save is not None:
                vtk.export_points(f"{save}_peaks", peaks["peak_location"], {"peak_energy_density": qmax, "cell": cells})
        out.update(peaks)
    if hist_rule is not None:
        with _large_cells(ctx, large_cells):
            counts = api.cell_histogram(xv, implicit, xi, cell_fields.energy_form(cond) / out["energy_form"], **hist_rule)
        out["energy_density_histogram"] = {
            "edges": api.histogram_edges(**hist_rule), "counts": counts,
            "volume": cell_fields.histogram_volume(counts, vol, api.fine_elements(implicit, total_grids))}
    if slices is not None:
        out["slices"] = []
        for i, (origin, du, dv, nu, nv) in enumerate(slices):
            s = api.sample_raster(xv, implicit, origin, du, dv, nu, nv, xi=xi)
            s["flux"] = cell_fields.sample_flux(cond, s["cell"], s["gradient"])
            s["energy_density"] = cell_fields.sample_energy_density(cond, s["cell"], s["gradient"])
            out["slices"].append(s)
            if save is not None:
                vtk.export_slice(f"{save}_slice{i}", origin, du, dv, s)
    if fields or save is not None:
        flux = cell_fields.mean_flux(cond, mean)
        if save is not None:
            vtk.export_cell_fields(base, {"a": cond, "mean_gradient": mean, "gram": gram, "mean_flux": flux, "energy": en, **peaks},
                                   save)
        if fields:
            out.update(mean=mean, gram=gram, flux=flux, energy=en, volumes=vol, cond=cond, base=base)
    if accelerate:
        fcg.close()
        xv.close()
    for st in states:
        st.close()
    implicit.close()
    if own_ctx:
        ctx.close()
    return out


def dirichlet_homogenization_tensor(n: int, eltype=Tri64, refinements: int = 2, *, ctx=None, sigma_grid=None, seed: int = 0,
                                    values=(1.0, 9.0), tolerance: float = 1e-10, smoother: str = "cg", accelerate: bool = False,
                                    fields: bool = False, save=None, cond=None, smoothing_steps: int = 3, max_cycles: int = 200,
                                    large_cells: bool = False):
    """The full homogenized tensor of the plain Dirichlet cell problem of `dirichlet_homogenization` from ONE grid: d corrector
    solves with xi = e_k on one implicit grid, one operator and one set of level states (the solve loop is
    `dirichlet_homogenization`'s), the correctors v_k kept in d finest-level vectors; then, with u_k = e_k.x + v_k,

        tensor        Sigma_kl = sum_c sigma_c : S_{u_k u_l}(c) / |Omega|      symmetric by construction
        tensor_flux   row k = sum_c |c| sigma_c m_{u_k}(c) / |Omega|           the flux form of corrector k

    S_{u_k u_k} = G_{u_k} comes from api.cell_moments (with the mean gradient the flux form needs), S_{u_k u_l}, k < l, from
    api.cell_pair_moments: d (d + 1) / 2 kernel passes in all, nothing polarised.  xi . tensor . xi is what
    `dirichlet_homogenization(xi=xi)` returns as "energy_form", to the accuracy of the solves.  The keywords are those of
    `dirichlet_homogenization` without `xi` (`large_cells` included: it holds around every moment pass).  Returns a dict: "tensor" (d, d), "tensor_flux" (d, d), "cycles" and "residual"
    (relative), one per solve, "volume"; with `fields` also "pairs" (d, d, Ne, d, d) -- pairs[k, l, c] = S_{u_k u_l}(c), the exact
    sensitivity d(Sigma_kl |Omega|) / d(sigma_c) (fields.tensor_sensitivity) --, "means" (d, Ne, d), "volumes", "cond", "base".
    `save` (a file name) writes the coarse mesh with the cell fields of every pair k <= l, "pair_kl" and "energy_kl" = sigma_c :
    S_{u_k u_l}(c) (vtk.export_cell_fields).  Memory beyond `dirichlet_homogenization`: d finest-level vectors.  No counterpart
    in the reference."""
    base, cond = _hypercube_problem(n, eltype, sigma_grid, seed, values, cond)
    return _tensor_run("dirichlet_homogenization_tensor", None, base, cond, refinements, ctx, tolerance,
                       smoother, accelerate, fields, save, smoothing_steps, max_cycles, large_cells)


def _hypercube_problem(n, eltype, sigma_grid, seed, values, cond):
    """Base mesh and conductivity per cell of the drivers on `hypercube(eltype, n)`: `cond` as given, else `sigma_grid` -- default:
    the seeded checkerboard of `values` -- looked up at the cell centres."""
    dim = api._dim_of(eltype)
    base = hypercube(eltype, n)
    if cond is None:
        if sigma_grid is None:
            sigma_grid = generate_conductivity(dim, n, seed, values)
        cond = conductivity_per_element(base, sigma_grid, (0.0,) * dim)
    else:
        cond = np.ascontiguousarray(cond, dtype=np.float64)
    return base, cond


def _tensor_run(who, faces, base, cond, refinements, ctx, tolerance, smoother, accelerate, fields, save, smoothing_steps,
                max_cycles, large_cells, slices=None):
    """The d corrector solves and moment passes behind `dirichlet_homogenization_tensor` and the drivers that differ from it in
    the base mesh and the constrained set only.  base, cond: the mesh (a torus where `base.period` is set) and the conductivity
    per cell.  faces: None -- the grid's default set, no call --, a function base -> one face array, set once
    before the solves, or base -> a list of d of them, set in front of solve k.  A set of the caller's is taken back behind the
    solves, also when one raises.  slices: rasters (origin, du, dv, nu, nv) every u_k = e_k.x + v_k is sampled on behind the
    solves ("slices": per raster a list over k of what `dirichlet_homogenization(slices=...)` returns per slice); on a torus
    sampling is switched on around these passes only."""
    dim = base.dim
    own_ctx = ctx is None
    if own_ctx:
        ctx = api.Context(0)
    face_sets = None if faces is None else faces(base)
    total_grids = refinements + 1
    implicit = api.ImplicitFineGrid(ctx, base, total_grids)
    implicit.set_smoother(smoother)
    op = api.L2PlusDivAGrad(implicit, 0.0, cond)
    if isinstance(face_sets, np.ndarray):
        implicit.set_dirichlet_faces(face_sets)
    elif face_sets is not None:
        implicit.set_dirichlet_faces(face_sets[0])       # (the level-1 system below is direction 0's)
    base_level = api.BaseLevel(implicit)
    states = [api.LevelState(implicit, i + 1) for i in range(total_grids)]
    top = states[-1]
    xv = api.DeviceMatrix(implicit, total_grids) if accelerate else top.x      # the iterate
    fcg = api.FlexibleCG(implicit, base_level, [op] * total_grids, states, total_grids, smoothing_steps) if accelerate else None
    V = [api.DeviceMatrix(implicit, total_grids) for _ in range(dim)]          # the correctors v_k
    ne = base.elements.shape[0]
    pairs = np.zeros((dim, dim, ne, dim, dim))
    means = np.zeros((dim, ne, dim))
    cycles, residual = [], []
    eye = np.eye(dim)
    try:
        for k in range(dim):
            if k > 0 and face_sets is not None and not isinstance(face_sets, np.ndarray):
                implicit.set_dirichlet_faces(face_sets[k])
                implicit.coarse_setup()
            cyc, rnorm, r0 = _dirichlet_solve(implicit, op, base_level, states, xv, fcg, eye[k], smoothing_steps, tolerance,
                                              max_cycles, f"{who}, direction {k}")
            cycles.append(cyc)
            residual.append(float(rnorm / r0) if r0 > 0.0 else 0.0)
            V[k].copyto(xv)
            with _large_cells(ctx, large_cells):
                means[k], pairs[k, k] = api.cell_moments(V[k], implicit, eye[k])
    finally:
        if face_sets is not None:
            implicit.set_dirichlet_faces(None)
    with _large_cells(ctx, large_cells):
        for k in range(dim):
            for l in range(k + 1, dim):
                pairs[k, l] = pairs[l, k] = api.cell_pair_moments(V[k], V[l], implicit, eye[k], eye[l])
    vol = cell_fields.cell_volumes(base)
    omega = float(vol.sum())
    tensor = np.zeros((dim, dim))
    for k in range(dim):
        for l in range(k, dim):
            tensor[k, l] = tensor[l, k] = float(cell_fields.pair_energy(cond, pairs[k, l]).sum() / omega)
    out = {"tensor": tensor, "tensor_flux": np.stack([cell_fields.flux_row(base, cond, means[k]) for k in range(dim)]),
           "cycles": cycles, "residual": residual, "volume": omega}
    if slices is not None:
        torus = getattr(base, "period", None) is not None
        if torus:
            implicit.set_periodic_sampling(True)
        try:
            out["slices"] = []
            for i, (origin, du, dv, nu, nv) in enumerate(slices):
                per_k = []
                for k in range(dim):
                    s = api.sample_raster(V[k], implicit, origin, du, dv, nu, nv, xi=eye[k])
                    s["flux"] = cell_fields.sample_flux(cond, s["cell"], s["gradient"])
                    s["energy_density"] = cell_fields.sample_energy_density(cond, s["cell"], s["gradient"])
                    per_k.append(s)
                    if save is not None:
                        vtk.export_slice(f"{save}_slice{i}_u{k + 1}", origin, du, dv, s)
                out["slices"].append(per_k)
        finally:
            if torus:
                implicit.set_periodic_sampling(False)
    if save is not None:
        cells = {"a": cond}
        for k in range(dim):
            for l in range(k, dim):
                cells[f"pair_{k + 1}{l + 1}"] = pairs[k, l]
                cells[f"energy_{k + 1}{l + 1}"] = cell_fields.pair_energy(cond, pairs[k, l])
        vtk.export_cell_fields(base, cells, save)
    if fields:
        out.update(pairs=pairs, means=means, volumes=vol, cond=cond, base=base)
    if accelerate:
        fcg.close()
        xv.close()
    for v in V:
        v.close()
    for st in states:
        st.close()
    implicit.close()
    if own_ctx:
        ctx.close()
    return out


def periodic_mesh(eltype, shape) -> Mesh:
    """`shape` unit cubes on a torus (include/hmg.h: hmg_periodic_mesh), the Kuhn split of `checkerboard_mesh`: node ids with the
    last coordinate fastest, taken modulo `shape`; cube q (C order of its multi-index) owns cells 6q .. 6q + 5 (2D: 2q, 2q + 1), so
    a per-cube field maps to cells by `np.repeat` without any coordinate.  An int is a cube.  Every axis needs 3 cubes or more.
    `Mesh.period` = shape; the nodes sit at their multi-index, and a cell that wraps names nodes on opposite sides of the box
    (`Mesh.cell_corners` unwraps it)."""
    import ctypes
    from . import _lib as L
    dim = api._dim_of(eltype)
    shp = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.int64), (dim,)))
    lib = L.load()
    nn, ne = ctypes.c_int64(), ctypes.c_int64()
    L.check(lib.hmg_periodic_mesh_size(dim, shp.ctypes.data_as(L.p_i64), ctypes.byref(nn), ctypes.byref(ne)))
    nodes = np.zeros((nn.value, dim))
    cells = np.zeros((ne.value, dim + 1), dtype=np.int64)
    L.check(lib.hmg_periodic_mesh(dim, shp.ctypes.data_as(L.p_i64), nodes.ctypes.data_as(L.p_f64), cells.ctypes.data_as(L.p_i64)))
    return Mesh(nodes, cells, shp.astype(np.float64))


def periodic_homogenization_tensor(n: int, eltype=Tri64, refinements: int = 2, *, ctx=None, sigma_grid=None, seed: int = 0,
                                   values=(1.0, 9.0), tolerance: float = 1e-10, smoother: str = "cg", accelerate: bool = False,
                                   fields: bool = False, save=None, smoothing_steps: int = 3, max_cycles: int = 200,
                                   large_cells: bool = False, slices=None):
    """The homogenized tensor of the PERIODIC cell problem -- its definition for periodic media, and for random media the boundary
    condition with the smallest boundary-layer error: on the torus of n^d unit cubes (`periodic_mesh`, n >= 3) find v_k periodic
    with a(v_k, w) = -int sigma e_k . grad w for all periodic w (lambda = 0, no constrained node), then "tensor" and "tensor_flux"
    from the per-cell moments of u_k = e_k.x + v_k as in `dirichlet_homogenization_tensor`, whose keywords (without `cond`) and
    returned dict these are.  `sigma_grid`: one tensor per unit cube, (n,) * dim + (dim,) diagonals or + (dim, dim) full symmetric
    tensors; default: the seeded checkerboard of `values`.  The operator has the constants in its kernel: the level-1 solve works on
    their complement (`ImplicitFineGrid.set_mean_free`, the default of a periodic grid), the finer levels need nothing, and a
    corrector is fixed up to a constant -- nothing is normalised, every quantity returned depends on gradients only.  The space of
    `dirichlet_homogenization_tensor` on the same `sigma_grid` is a subspace of the periodic one, so this diagonal is at most
    that one's.  The tensor does not depend on where the period starts (in 3D up to the discretisation: the cells that wrap
    choose their interior diagonals differently).
    `slices`: a list of rasters (origin, du, dv, nu, nv) -- pixel (a, b) at origin + a du + b dv, anywhere: a point is taken
    modulo the period --; behind the solves every u_k = e_k.x + v_k is sampled on each on the device (api.sample_raster with the
    grid's periodic sampling switched on for these passes) and "slices" in the returned dict is, per raster, a list over k of
    dicts "value", "gradient", "cell", "flux" and "energy_density" as `dirichlet_homogenization(slices=...)` returns them.  Over
    several periods e_k.x grows while v_k, the gradient and the flux repeat.  `save` writes `<save>_slice<i>_u<k>.vts`.  The
    tensor does not depend on `slices`.  No counterpart in the reference."""
    dim = api._dim_of(eltype)
    base = periodic_mesh(eltype, n)
    if sigma_grid is None:
        sigma_grid = generate_conductivity(dim, n, seed, values)
    sg = np.asarray(sigma_grid, dtype=np.float64)
    if sg.shape not in ((n,) * dim + (dim,), (n,) * dim + (dim, dim)):
        raise ValueError(f"sigma_grid must have shape {(n,) * dim + (dim,)} or {(n,) * dim + (dim, dim)}, not {sg.shape}")
    per_cube = base.elements.shape[0] // n ** dim
    cond = np.ascontiguousarray(np.repeat(sg.reshape((n ** dim,) + sg.shape[dim:]), per_cube, axis=0))
    return _tensor_run("periodic_homogenization_tensor", None, base, cond, refinements, ctx, tolerance, smoother, accelerate,
                       fields, save, smoothing_steps, max_cycles, large_cells, slices)


def faces_on_plane(base: Mesh, axis: int, value: float):
    """The faces of a base mesh (3D: triangles, 2D: edges) all of whose nodes have coordinate `axis` equal to `value` (to 1e-9 of
    the mesh's extent): an (nfaces, dim) array of 1-based node ids for `ImplicitFineGrid.set_dirichlet_faces`."""
    x = np.asarray(base.nodes, dtype=np.float64)[:, axis]
    on = np.abs(x - value) <= 1e-9 * max(1.0, float(np.ptp(x)))
    faces = np.unique(api.cell_faces(base), axis=0)
    return np.ascontiguousarray(faces[on[faces - 1].all(axis=1)])


def block_faces(base: Mesh, block: int):
    """The faces on the planes x_a = origin_a + j * block, j integer, a = 1 .. dim, of a base mesh of unit cubes whose lowest
    corner is `origin`: the boundaries of its block^dim blocks, the outer boundary included.  (nfaces, dim), 1-based ids."""
    nodes = np.asarray(base.nodes, dtype=np.float64)
    rel = nodes - nodes.min(axis=0)
    on = np.abs(rel / block - np.rint(rel / block)) <= 1e-9              # (Nn, dim): the node lies on a plane of axis a
    faces = np.unique(api.cell_faces(base), axis=0)
    rf = rel[faces - 1]                                                   # (nfaces, dim nodes, dim axes)
    flat = np.abs(rf - rf[:, :1, :]).max(axis=1) <= 1e-9                  # the face is normal to axis a ...
    return np.ascontiguousarray(faces[(flat & on[faces - 1].all(axis=1)).any(axis=1)])    # ... and that plane is a block boundary


def uniaxial_homogenization_tensor(n: int, eltype=Tri64, refinements: int = 2, *, ctx=None, sigma_grid=None, seed: int = 0,
                                   values=(1.0, 9.0), tolerance: float = 1e-10, smoother: str = "cg", accelerate: bool = False,
                                   fields: bool = False, save=None, cond=None, smoothing_steps: int = 3, max_cycles: int = 200,
                                   large_cells: bool = False):
    """The homogenized tensor of the mixed ("uniaxial") cell problems on `hypercube(eltype, n)`: for k = 1 .. d the potential
    u_k = e_k.x + v_k is fixed on the two faces of the cube normal to e_k (v_k = 0 there) and the other faces are insulated --
    the natural condition, which `rhs_axi_grad_v` yields wherever the constraint is absent.  One grid and one operator; in front
    of solve k the two faces become the grid's Dirichlet set (`ImplicitFineGrid.set_dirichlet_faces`, `faces_on_plane`), the
    default set is restored behind the solves.  Row k of "tensor_flux" is the mean flux of u_k, "tensor" the energy form
    sum_c sigma_c : S_{u_k u_l}(c) / |Omega| (its diagonal is the effective conductivity a two-electrode measurement along e_k
    sees; exact for a laminate: the harmonic mean across the layers, the arithmetic mean along them).  The space of v_k contains
    the one of `dirichlet_homogenization_tensor`, so the diagonal is at most that driver's.  Keywords and the returned dict are
    `dirichlet_homogenization_tensor`'s.  No counterpart in the reference."""
    def sides(base):
        x = np.asarray(base.nodes, dtype=np.float64)
        return [np.concatenate([faces_on_plane(base, k, x[:, k].min()), faces_on_plane(base, k, x[:, k].max())])
                for k in range(base.dim)]
    base, cond = _hypercube_problem(n, eltype, sigma_grid, seed, values, cond)
    return _tensor_run("uniaxial_homogenization_tensor", sides, base, cond, refinements, ctx, tolerance,
                       smoother, accelerate, fields, save, smoothing_steps, max_cycles, large_cells)


def block_homogenization_tensor(n: int, block: int, eltype=Tri64, refinements: int = 2, *, ctx=None, sigma_grid=None,
                                seed: int = 0, values=(1.0, 9.0), tolerance: float = 1e-10, smoother: str = "cg",
                                accelerate: bool = False, fields: bool = False, save=None, cond=None, smoothing_steps: int = 3,
                                max_cycles: int = 200, large_cells: bool = False):
    """Block upscaling in one run: the plain Dirichlet cell problem of `dirichlet_homogenization_tensor` on every block^dim block
    of `hypercube(eltype, n)` at once.  With v = 0 on the block boundaries (`block_faces`, set once) the blocks are independent
    cell problems inside one grid: one table build, d solves, and the per-cell moments summed per block give
    "tensor", shape (n / block,) * dim + (dim, dim) -- block [i, j(, k)] is the cube's i-th block along the first axis, as
    `sigma_grid` is indexed --, exactly symmetric and directly usable as the `sigma_grid` of a run at the next scale, and
    "tensor_flux" of the same shape (row k: the flux form of corrector k).  Block b's tensor is what
    `dirichlet_homogenization_tensor` gives on that block's cells as a mesh of their own, to the accuracy of the solves (the
    residual that stops them is the whole grid's).  "cycles", "residual" and "volume" (of one block) as there; `fields` adds that
    driver's fields of the whole grid and "block_of_cell" (Ne, dim).  No counterpart in the reference."""
    dim = api._dim_of(eltype)
    if block < 1 or n % block:
        raise ValueError(f"block must divide n = {n}")
    base, cond = _hypercube_problem(n, eltype, sigma_grid, seed, values, cond)
    run = _tensor_run("block_homogenization_tensor", lambda base: block_faces(base, block), base, cond, refinements, ctx,
                      tolerance, smoother, accelerate, True, save, smoothing_steps, max_cycles, large_cells)
    base, cond, vol, pairs, means = run["base"], run["cond"], run["volumes"], run["pairs"], run["means"]
    nb = n // block
    centers = _centers(base)
    bidx = np.floor((centers - np.asarray(base.nodes).min(axis=0)) / block).astype(np.int64)
    flat = np.ravel_multi_index(tuple(bidx[:, a] for a in range(dim)), (nb,) * dim)
    omega = float(block) ** dim
    tensor = np.zeros((nb ** dim, dim, dim))
    tflux = np.zeros((nb ** dim, dim, dim))
    for k in range(dim):
        flux = cell_fields.mean_flux(cond, means[k]) * vol[:, None]
        for a in range(dim):
            tflux[:, k, a] = np.bincount(flat, weights=flux[:, a], minlength=nb ** dim) / omega
        for l in range(k, dim):
            e = np.bincount(flat, weights=cell_fields.pair_energy(cond, pairs[k, l]), minlength=nb ** dim) / omega
            tensor[:, k, l] = tensor[:, l, k] = e
    out = {"tensor": tensor.reshape((nb,) * dim + (dim, dim)), "tensor_flux": tflux.reshape((nb,) * dim + (dim, dim)),
           "cycles": run["cycles"], "residual": run["residual"], "volume": omega}
    if fields:
        out.update(pairs=pairs, means=means, volumes=vol, cond=cond, base=base, block_of_cell=bidx)
    return out
