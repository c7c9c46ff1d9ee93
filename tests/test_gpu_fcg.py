"""
The V-cycle-preconditioned flexible CG on the device (include/hmg.h: hmg_fcg_*, csrc/hmg_fcg.hip / hmg_fcg.cpp, api.FlexibleCG,
driver.checkerboard_homogenization(accelerate=True)) against its two CPU statements (tests/_fcg_form.py): the global form with
assembled matrices and the oracle's cell-local form.  Coefficient fields and initial guesses are built on the host the way the
CPU statements build them and handed to the device.  Tolerances: x 1e-9 max|x| and R 1e-8 max|R_0| -- what test_gpu_parity.py
allows x and r after one to three V-cycles against the same global form; alpha and beta 1e-8 relative.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

from _fcg_form import fcg_global, fcg_local, local_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Device:
    """Grid, operator, level states, iterate, right-hand side and the FlexibleCG object of one problem."""

    def __init__(self, ctx, mesh, sig, lam, levels, steps, x0, b):
        self.ctx, self.levels = ctx, levels
        self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(mesh.nodes, mesh.elements + 1), levels)
        self.A = hmg.L2PlusDivAGrad(self.g, lam, sig)
        self.sts = [hmg.LevelState(self.g, i + 1) for i in range(levels)]
        self.bl = hmg.BaseLevel(self.g)
        self.x = hmg.DeviceMatrix(self.g, levels).from_host(x0)
        self.b = hmg.DeviceMatrix(self.g, levels).from_host(b)
        self.fcg = hmg.FlexibleCG(self.g, self.bl, [self.A] * levels, self.sts, levels, steps)

    def close(self):
        self.fcg.close()
        for v in (self.x, self.b):
            v.close()
        for s in self.sts:
            s.close()
        self.g.close()


def _consistent(O, implicit, constraint, levels, a):
    a = np.asfortranarray(a)
    O.broadcast_interfaces(a, implicit, levels)
    O.apply_constraint(a, levels, constraint, implicit)
    return a


def _close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("dim,n,grids,steps", [(2, 4, 3, 3), (2, 3, 4, 1), (3, 2, 3, 3), (3, 2, 4, 3)])
def test_device_matches_the_global_form(oracle, ctx, dim, n, grids, steps):
    """The four cases of tests/test_fcg_statement.py (contrast 100, default_rng(11)), after each of 4 steps."""
    from _global_form import GlobalForm
    O, lam = oracle, 1.0
    rng = np.random.default_rng(11)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 100.0)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    x0 = _consistent(O, implicit, constraint, grids, rng.random(states[-1].x.shape))
    b = np.zeros_like(x0, order="F")
    O.local_rhs(b, implicit)
    G = GlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    l = grids - 1
    gx, gb = G.gather(x0, l), G.gather_sum(b, l)
    r0 = np.abs(np.where(G.inner[l], gb - G.A[l] @ gx, 0.0)).max()
    d = Device(ctx, base, cond, lam, grids, steps, x0, b)
    d.fcg.start(d.x, d.b)
    assert np.abs(G.gather_sum(d.fcg.vec("R"), l) - np.where(G.inner[l], gb - G.A[l] @ gx, 0.0)).max() <= 1e-11 * r0
    glob = fcg_global(G, l, gx, gb, steps)
    for it in range(4):
        wx, wR, wp, wa, wb = next(glob)
        d.fcg.step()
        alpha, beta, pq, pr = d.fcg.scalars()
        ex = np.abs(G.gather(d.x.to_host(), l) - wx).max() / np.abs(wx).max()
        eR = np.abs(G.gather_sum(d.fcg.vec("R"), l) - wR).max() / r0
        print(f"step {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.12g} / {wa:.12g}  beta {beta:.12g} / {wb:.12g}")
        assert ex <= 1e-9 and eR <= 1e-8, (it, ex, eR)
        assert _close(alpha, wa, 1e-8) and _close(beta, wb, 1e-8), (it, alpha, wa, beta, wb)
    d.close()


def _against_local(O, ctx, mesh, sig, lam, levels, steps, nsteps, rng, full=None, check_residual_norm=False):
    """full = (mesh, sig) of a larger grid of which `mesh` holds a prefix of the cells and of the nodes: the device objects are
    created on it and shrunk to `mesh` before the start (tests/test_gpu_stream_lengths.py: odd lengths).
    check_residual_norm: after the steps, hmg_fcg_residual_norm against the first-copy norm of the statement's interface-summed
    R, at the 1e-9 test_setup_memory_counters_and_stale_state allows that number."""
    implicit = O.ImplicitFineGrid.create(mesh, levels)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(mesh))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(m), O.mass_matrix(m), constraint, lam, sig)
           for m in implicit.reference.levels]
    states = [O.LevelState.create(mesh.nelements(), implicit.nf(i + 1)) for i in range(levels)]
    shape = states[-1].x.shape
    x0 = _consistent(O, implicit, constraint, levels, rng.random(shape))
    b = np.asfortranarray(rng.standard_normal(shape))
    if full is None:
        d = Device(ctx, mesh, sig, lam, levels, steps, x0, b)
    else:
        fmesh, fsig = full
        pad = lambda a: np.asfortranarray(np.concatenate([a, np.zeros((shape[0], fmesh.nelements() - shape[1]))], axis=1))
        d = Device(ctx, fmesh, fsig, lam, levels, steps, pad(x0), pad(b))
        d.g.shrink(mesh.nelements(), mesh.nnodes())
        d.bl = hmg.BaseLevel(d.g)
        assert d.x.shape == shape
    d.fcg.start(d.x, d.b)
    R0 = d.fcg.vec("R")
    r0 = np.abs(R0).max()
    loc = fcg_local(O, implicit, O.make_base_level(mesh, sig, lam), ops, states, levels, steps, x0, b)
    for it in range(nsteps):
        wx, wR, wp, wa, wb = next(loc)
        d.fcg.step()
        alpha, beta, pq, pr = d.fcg.scalars()
        ex = np.abs(d.x.to_host() - wx).max() / np.abs(wx).max()
        eR = np.abs(d.fcg.vec("R") - wR).max() / r0
        print(f"step {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.12g} / {wa:.12g}  beta {beta:.12g} / {wb:.12g}")
        assert ex <= 1e-9 and eR <= 1e-8, (it, ex, eR)
        assert _close(alpha, wa, 1e-8) and _close(beta, wb, 1e-8), (it, alpha, wa, beta, wb)
    if check_residual_norm:
        summed = np.asfortranarray(wR.copy())
        O.broadcast_interfaces(summed, implicit, levels)
        O.zero_out_all_but_one(summed, implicit, levels)
        want, got = float(np.linalg.norm(summed)), d.fcg.residual_norm()
        print(f"residual norm {got:.12e} / {want:.12e}")
        assert abs(got - want) <= 1e-9 * want, (got, want)
    d.close()


@pytest.mark.parametrize("levels", [4, 5, 6])
def test_device_matches_the_cell_local_statement_3d(oracle, ctx, levels):
    """One mesh per kernel family of the plain apply and of the V-cycle inside: 2 x 2 x 2 cubes, top level 4 (one pipelined wave
    per cell), 5 (one wave per cell), 6 (register-blocked workgroups); two steps."""
    O = oracle
    rng = np.random.default_rng(40 + levels)
    mesh = O.hypercube(3, 2)
    sig = rng.choice([1.0, 9.0], size=(mesh.nelements(), 3))
    _against_local(O, ctx, mesh, sig, 1.0, levels, 3, 2, rng)


def test_device_matches_the_cell_local_statement_level7(oracle, ctx):
    """Cells larger than the LDS (role-split slab kernel): the 48-cell mesh of tests/test_gpu_slab2.py, contrast 100."""
    O = oracle
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, 2, seed=3, values=(1.0, 100.0), lam=0.7)
    g.close()
    mesh = O.Mesh(np.ascontiguousarray(base.nodes), np.ascontiguousarray(base.elements - 1))
    n0 = ctx.counter("slab2_launches")
    _against_local(O, ctx, mesh, cond, 0.7, 7, 3, 2, np.random.default_rng(47))
    assert ctx.counter("slab2_launches") > n0


@pytest.mark.parametrize("levels,n,seed", [(6, 4, 6), (9, 4, 9)])
def test_device_matches_the_cell_local_statement_2d(oracle, ctx, levels, n, seed):
    """Triangles: top level 6 (workgroup per cell) and 9 (cells larger than the LDS, row-band kernel; the smallest mesh of
    tests/test_gpu_tri_deep.py: 4 x 4 squares, perturbed nodes)."""
    O = oracle
    mesh = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, n, origin=(-n / 2.0,) * 2))
    rng = np.random.default_rng(seed)
    mesh.nodes = mesh.nodes + 0.2 * (rng.random(mesh.nodes.shape) - 0.5)
    sig = rng.choice([1.0, 9.0], size=(mesh.nelements(), 2))
    n0 = ctx.counter("rows_launches")
    _against_local(O, ctx, mesh, sig, 0.7, levels, 3, 2, rng)
    assert (ctx.counter("rows_launches") > n0) == (levels >= 9)


def _three_steps(ctx, dim, n, levels, steps, zero_entry):
    O_rng = np.random.default_rng(5)
    base = driver.hypercube(hmg.Tet64 if dim == 3 else hmg.Tri64, n)
    sig = O_rng.choice([1.0, 9.0], size=(base.elements.shape[0], dim))
    ctx.set_option("zero_entry", zero_entry)
    try:
        g = hmg.ImplicitFineGrid(ctx, base, levels)
        A = hmg.L2PlusDivAGrad(g, 1.0, sig)
        sts = [hmg.LevelState(g, i + 1) for i in range(levels)]
        bl = hmg.BaseLevel(g)
        x, b = hmg.DeviceMatrix(g, levels), hmg.DeviceMatrix(g, levels)
        x.rand(3)
        hmg.broadcast_interfaces(x, g, levels)
        hmg.apply_constraint(x, levels, g)
        hmg.local_rhs(b, g)
        f = hmg.FlexibleCG(g, bl, [A] * levels, sts, levels, steps)
        f.start(x, b)
        for _ in range(3):
            f.step()
        out = x.to_host(), f.vec("R"), f.vec("p"), f.scalars()
        f.close()
        for v in [x, b] + sts:
            v.close()
        g.close()
        return out
    finally:
        ctx.set_option("zero_entry", 1)


@pytest.mark.parametrize("dim,n,levels,steps", [(3, 3, 4, 2), (3, 2, 5, 2), (3, 2, 6, 2), (3, 3, 4, 3), (2, 4, 5, 2)])
def test_zero_entry_and_reruns_give_the_same_bits(ctx, dim, n, levels, steps):
    """With two smoothing steps the top level is entered with a zero that is never written; option "zero_entry" = 0 writes it
    (three steps: always written).  x, R, p after three steps are equal to the last bit, and so is a second run in a fresh
    context (fixed-order reductions)."""
    on = _three_steps(ctx, dim, n, levels, steps, 1)
    off = _three_steps(ctx, dim, n, levels, steps, 0)
    fresh_ctx = hmg.Context(0)
    again = _three_steps(fresh_ctx, dim, n, levels, steps, 1)
    fresh_ctx.close()
    for name, a, b_, c in zip(("x", "R", "p"), on, off, again):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b_), name
        assert np.array_equal(a, c), name
    assert on[3] == off[3] == again[3]


def test_setup_memory_counters_and_stale_state(oracle, ctx):
    """p, q, R are setup memory ("device_allocs" does not move across start / step, "fcg_bytes" = 3 vectors of the top level);
    after a shrink or a new lambda a step without a start is an error."""
    O, levels = oracle, 3
    mesh = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 6, origin=(-3.0,) * 3))
    rng = np.random.default_rng(5)
    sig = rng.choice([1.0, 9.0], size=(mesh.nelements(), 3))
    shape = (35, mesh.nelements())
    bytes0 = ctx.counter("fcg_bytes")
    d = Device(ctx, mesh, sig, 0.5, levels, 3, np.zeros(shape, order="F"), rng.standard_normal(shape))
    assert ctx.counter("fcg_bytes") - bytes0 == 3 * 8 * d.g.ld(levels) * d.g.ncells()
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        d.fcg.x = d.x
        d.fcg.step()
    d.fcg.start(d.x, d.b)
    ctx.sync()
    allocs = ctx.counter("device_allocs")
    for _ in range(5):
        d.fcg.step()
    ctx.sync()
    assert ctx.counter("device_allocs") == allocs
    r5 = d.fcg.residual_norm()
    d.fcg.start(d.x, d.b)
    assert ctx.counter("device_allocs") == allocs
    assert abs(d.fcg.residual_norm() - r5) <= 1e-9 * r5          # the recurred residual is the true one
    with pytest.raises(HmgError, match="state vectors"):
        d.fcg.start(d.sts[-1].x, d.b)
    d.fcg.start(d.x, d.b)
    d.A.lam = 0.25
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        d.fcg.step()
    d.fcg.start(d.x, d.b)
    d.fcg.step()
    d.g.shrink(O.find_elements_in_radius(mesh, 2), O.find_nodes_in_radius(mesh, 2))
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        d.fcg.step()
    with pytest.raises(HmgError, match="hmg_fcg_start"):
        d.fcg.residual_norm()
    d.close()
    assert ctx.counter("fcg_bytes") == bytes0


def test_shrunk_grid_matches_the_oracle_on_the_shrunk_mesh(oracle, ctx):
    """The set-up of test_driver_with_domain_shrink_matches_cpu (2D, n = 5, two refinements: 112 x 112 squares shrunk to
    110 x 110 with lambda = 1/2): object and vectors created on the full grid, start + 3 steps after hmg_grid_shrink against
    the cell-local statement on the shrunk mesh."""
    O, n, levels, steps = oracle, 5, 3, 3
    radius = driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n)
    width = 2 * radius
    mesh = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, width, origin=(-float(radius),) * 2))
    sgrid = driver.generate_conductivity(2, width, 31)
    cond = O.conductivity_per_element(mesh, sgrid, (radius + 1.0,) * 2)
    x_full = hmg.host_random((15, mesh.nelements()), 131)
    d = Device(ctx, mesh, cond, 1.0, levels, steps, x_full, np.zeros_like(x_full))
    hmg.broadcast_interfaces(d.x, d.g, levels)
    lam = 0.5
    small = driver.compute_box_radius(1, n) + driver.compute_boundary_layer(lam, n)
    assert small < radius
    ne, nn = O.find_elements_in_radius(mesh, small), O.find_nodes_in_radius(mesh, small)
    d.g.shrink(ne, nn)
    hmg.apply_constraint(d.x, levels, d.g)
    d.A.lam = lam
    hmg.next_rhs(d.b, d.x, d.g)
    d.bl = hmg.BaseLevel(d.g)
    sub = O.Mesh(mesh.nodes[:nn], np.ascontiguousarray(mesh.elements[:ne]))
    sig = np.ascontiguousarray(cond[:ne])
    implicit = O.ImplicitFineGrid.create(sub, levels)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(sub))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(m), O.mass_matrix(m), constraint, lam, sig)
           for m in implicit.reference.levels]
    states = [O.LevelState.create(ne, implicit.nf(i + 1)) for i in range(levels)]
    x0, b = d.x.to_host(), d.b.to_host()
    assert x0.shape == (15, ne)
    d.fcg.start(d.x, d.b)
    r0 = np.abs(d.fcg.vec("R")).max()
    loc = fcg_local(O, implicit, O.make_base_level(sub, sig, lam), ops, states, levels, steps, x0, b)
    for it in range(3):
        wx, wR, wp, wa, wb = next(loc)
        d.fcg.step()
        alpha, beta, pq, pr = d.fcg.scalars()
        ex = np.abs(d.x.to_host() - wx).max() / np.abs(wx).max()
        eR = np.abs(d.fcg.vec("R") - wR).max() / r0
        print(f"step {it + 1}: x {ex:.2e}  R {eR:.2e}  alpha {alpha:.12g} / {wa:.12g}  beta {beta:.12g} / {wb:.12g}")
        assert ex <= 1e-9 and eR <= 1e-8, (it, ex, eR)
        assert _close(alpha, wa, 1e-8) and _close(beta, wb, 1e-8)
    d.close()


_NF = {2: [3, 6, 15, 45, 153], 3: [4, 10, 35, 165, 969]}


@pytest.mark.parametrize("dim,refinements", [(2, 3), (3, 1), (3, 2)])
def test_accelerated_driver_converges_to_the_direct_fem_answer_in_fewer_cycles(oracle, ctx, dim, refinements):
    """The cases of test_driver_converges_to_the_direct_fem_answer (n = 0, tolerance 1e-12, field and xi from default_rng(8)) with
    x0 = default_rng(0).random: accelerate=True reaches the sparse direct solve's number to 1e-8 and takes strictly fewer cycles
    than the plain driver (CPU statement: 18 / 15 / 18 against 26 / 18 / 27)."""
    from _textbook_fem import converged_first_term
    rng = np.random.default_rng(8)
    sgrid = np.where(rng.random((10,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    xi = rng.standard_normal(dim)
    xi /= np.linalg.norm(xi)
    x0 = np.random.default_rng(0).random((_NF[dim][refinements], (2 if dim == 2 else 6) * 10 ** dim))
    el = hmg.Tet64 if dim == 3 else hmg.Tri64
    kw = dict(refinements=refinements, tolerance=1e-12, xi=xi, sigma_grid=sgrid, x0=x0, ctx=ctx, max_cycles=60)
    t_acc, t_plain = {}, {}
    sigma, hist = driver.checkerboard_homogenization(0, el, accelerate=True, timings=t_acc, **kw)
    plain, hist_p = driver.checkerboard_homogenization(0, el, accelerate=False, timings=t_plain, **kw)
    want = converged_first_term(oracle, dim, sgrid, xi, refinements)
    print(f"accelerated {len(hist)} cycles, sigma - want = {sigma - want:.3e};  plain {len(hist_p)} cycles, {plain - want:.3e}")
    assert abs(sigma - want) <= 1e-8 * abs(want), (sigma, want, len(hist))
    assert len(hist) < len(hist_p), (len(hist), len(hist_p))
    assert t_acc["vcycles"] == len(hist) and t_acc["inexact_vcycles"] == 0
    r = [h[2] for h in hist]
    assert r[-1] < 1e-6 * r[0]                                # entry 2 is the norm of the true residual


def test_accelerated_driver_at_contrast_100(ctx):
    """Where it matters: 3D, sigma in {1, 100}, n = 1, two refinements, tolerance 1e-5, field then x0 from default_rng(7) in the
    oracle driver's order.  CPU statement: 24 iterations against 45 V-cycles (a ratio of 1.9); 1.5 leaves room for the device's
    different rounding path through a non-linear iteration."""
    rng = np.random.default_rng(7)
    n, refinements = 1, 2
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sgrid = np.where(rng.random((width,) * 3 + (3,)) < 0.5, 1.0, 100.0)
    x0 = rng.random((_NF[3][refinements], 6 * width ** 3))
    kw = dict(refinements=refinements, tolerance=1e-5, sigma_grid=sgrid, x0=x0, ctx=ctx)
    sigma, hist = driver.checkerboard_homogenization(n, hmg.Tet64, accelerate=True, **kw)
    plain, hist_p = driver.checkerboard_homogenization(n, hmg.Tet64, accelerate=False, **kw)
    print(f"accelerated {len(hist)} cycles (sigma {sigma:.8f}), plain {len(hist_p)} cycles (sigma {plain:.8f})")
    assert len(hist) <= len(hist_p) / 1.5, (len(hist), len(hist_p))
    assert abs(sigma - plain) <= 1e-3 * abs(plain)            # (they stop at iterates about the tolerance apart)
