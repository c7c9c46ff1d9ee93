"""
The flat-pair streaming kernels (one double2 per thread and vector over the ld x ncells storage, 256-thread blocks, no grid-stride
loop, thread 0 of block 0 finishes an odd length: csrc/hmg_kernels.hip k_fill ... k_cg_pupdate, csrc/hmg_fcg.hip) at the lengths
where that shape can go wrong -- tests/_stream_twin.py names the classes, tests/test_stream_twin_host.py holds the ladder to them.

  1. BLAS-1 at every length class, to the last bit against the one-rounding twins, reductions exactly on integer data, with the
     storage behind the prefix of a shrunk grid and 64 guard doubles behind the vector compared as bit patterns after every call.
  2. The two reduction routes at their switch (2048 | 2049 blocks) and a fold whose 256 blocks all hold partials (2304), exactly.
  3. The default CG smoother and the V-cycle against the CPU oracle on grids with an odd number of entries (47 of 48 tetrahedra,
     31 of 32 triangles), fused and unfused.
  4. The flexible CG at odd lengths against its cell-local statement, and its two branches for a vanishing p.q.
  5. hmg_vec_wrap refuses memory that is not 16-byte aligned.

Tolerances: bit equality and integer sums, or those the neighbouring files apply to the same quantity against the same oracle
(x, r, p of a smoother 1e-10: test_gpu_parity.py test_smoothing_steps; x 1e-9 and r 1e-8 after V-cycles:
test_unstructured_delaunay_mesh; flexible CG: test_gpu_fcg.py).  The one bound on a rounded sum is n 2^-53 sum |x_i y_i|, which
holds for any summation order.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd._lib import HmgError

import _stream_twin as T
from test_gpu_fcg import _against_local

pytestmark = pytest.mark.gpu

GUARD = 64                                   # doubles behind every wrapped vector
SENTINELS = (1.5e300, -2.5e300, 3.5e300)     # one per vector: a copy from one vector's guard into another's shows


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def _cube(O, dim, n):
    return O.order_nodes_and_elements_by_magnitude(O.hypercube(dim, n, origin=(-n / 2.0,) * dim))


class Wrapped:
    """A level vector in a torch tensor of ld * ncells_full + GUARD doubles, written and read raw (BLAS-1 does not care about the
    storage order).  `write` puts the sentinel everywhere behind the first n entries, `read` returns those n entries and checks
    that everything behind them still holds the sentinel's bits."""

    def __init__(self, ctx, g, level, sentinel):
        import torch
        self.torch, self.ctx, self.g, self.level, self.sentinel = torch, ctx, g, level, sentinel
        self.total = g.ld(level) * g.ncells()
        self.t = torch.full((self.total + GUARD,), sentinel, dtype=torch.float64, device="cuda")
        self.v = hmg.DeviceMatrix(g, level, device_ptr=self.t.data_ptr())

    def n(self):
        return self.g.ld(self.level) * self.g.ncells()

    def write(self, a):
        host = np.full(self.total + GUARD, self.sentinel)
        host[: a.size] = np.asarray(a, dtype=np.float64).reshape(-1)
        self.t.copy_(self.torch.from_numpy(host))
        self.torch.cuda.synchronize()
        return self

    def reset_guard(self):
        n = self.n()
        self.t[n:] = self.sentinel
        self.torch.cuda.synchronize()

    def read(self, what=""):
        self.ctx.sync()
        host = self.t.cpu().numpy()
        n = self.n()
        behind = T.bits(host[n:])
        touched = np.flatnonzero(behind != T.bits(np.array([self.sentinel]))[0])
        assert touched.size == 0, f"{what}: entries {n + touched[:8]} behind the {n} of the prefix were written"
        return host[:n].copy()

    def close(self):
        self.v.close()


class LadderGrid:
    """One grid per dimension, created at full size; every level's three wrapped vectors are made at full size, on demand."""

    def __init__(self, O, ctx, dim):
        width, levels = T.LADDER_MESH[dim]
        self.O, self.ctx, self.dim, self.levels = O, ctx, dim, levels
        self.mesh = _cube(O, dim, width)
        self.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.mesh.nodes, self.mesh.elements + 1), levels)
        self.vecs, self.impls = {}, {}

    def shrink(self, cells):
        self.g.shrink(cells, self.mesh.nnodes())
        assert self.g.ncells() == cells

    def vectors(self, level):
        if level not in self.vecs:
            self.shrink(self.mesh.nelements())
            self.vecs[level] = [Wrapped(self.ctx, self.g, level, s) for s in SENTINELS]
        return self.vecs[level]

    def impl(self, cells):
        if cells not in self.impls:
            O = self.O
            sub = O.Mesh(self.mesh.nodes.copy(), np.ascontiguousarray(self.mesh.elements[:cells]))
            self.impls[cells] = O.ImplicitFineGrid.create(sub, self.levels)
        return self.impls[cells]

    def close(self):
        for vs in self.vecs.values():
            for w in vs:
                w.close()
        self.g.close()


@pytest.fixture(scope="module")
def ladder_grids(oracle, ctx):
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = LadderGrid(oracle, ctx, dim)
        return made[dim]
    yield get
    for s in made.values():
        s.close()


# ---- 1. BLAS-1 at every length class ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,level,cells", T.LADDER, ids=[f"{d}d-level{l}-{k}cells" for d, l, k in T.LADDER])
def test_blas1_at_length(ladder_grids, dim, level, cells):
    """fill, copy, axpy, xpby bit-equal to the twins on random normal data; dot and norm exact on integer data; dot on random
    data within the any-order bound; norm_unique exact on integer data; copy() and similar() take the prefix shape; after every
    call the dropped columns and the guards of all three vectors keep their bits."""
    S = ladder_grids(dim)
    X, Y, Z = S.vectors(level)
    S.shrink(cells)
    c = T.length_class(S.g.ld(level), cells)
    n = c["n"]
    assert S.g.ld(level) == T.NF[dim][level - 1] and X.n() == n
    print(f"n = {n}, odd {c['odd']}, pairs {c['h']} (mod 256: {c['hmod']}), blocks {c['nb']}: {sorted(T.classes_of(c['ld'], cells))}")
    rng = np.random.default_rng(1000 * dim + 100 * level + cells)

    def check(what, *pairs):
        for w, want in pairs:
            got = w.read(what)
            np.testing.assert_array_equal(T.bits(got), T.bits(want), err_msg=what)

    x, y, z = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    X.write(x), Y.write(y), Z.write(z)
    check("upload", (X, x), (Y, y), (Z, z))
    hmg.axpy(0.37, X.v, Y.v)
    y = T.axpy(0.37, x, y)
    check("axpy", (X, x), (Y, y), (Z, z))
    hmg.xpby(X.v, -1.7, Y.v)                                             # y = x - 1.7 y
    y = T.xpby(x, -1.7, y)
    check("xpby", (X, x), (Y, y), (Z, z))
    Z.v.copyto(Y.v)
    check("copy", (X, x), (Y, y), (Z, y))
    Y.v.fill(-0.3125)
    check("fill", (X, x), (Y, np.full(n, -0.3125)), (Z, y))
    Y.v.fill(0.0)
    check("fill with zero", (X, x), (Y, np.zeros(n)), (Z, y))

    # a rounded dot product: any order of summation stays within n u sum |x_i y_i|
    got = hmg.dot(X.v, Z.v)
    exact, sum_abs = T.exact_dot(x, y)
    err, bound = abs(Fraction(got) - exact), T.dot_bound(n, sum_abs)
    print(f"dot of random data: error {float(err):.3e}, bound {float(bound):.3e}")
    assert err <= bound, (got, float(exact), float(err), float(bound))
    check("dot", (X, x), (Y, np.zeros(n)), (Z, y))

    # exact reductions
    xi, yi = T.integers(rng, n), T.integers(rng, n)
    X.write(xi), Y.write(yi)
    assert T.integer_sums_are_exact(n)
    assert hmg.dot(X.v, Y.v) == T.int_dot(xi, yi)
    assert hmg.dot(Y.v, X.v) == T.int_dot(xi, yi)
    assert hmg.dot(X.v, X.v) == T.int_dot(xi, xi)
    assert hmg.norm(X.v) == math.sqrt(T.int_dot(xi, xi)) and hmg.norm(Y.v) == math.sqrt(T.int_dot(yi, yi))
    check("integer dot and norm", (X, xi), (Y, yi), (Z, y))

    # norm_unique: first copies only, in the hierarchical order an upload takes
    nf = S.g.nf(level)
    a = np.asfortranarray(T.integers(rng, (nf, cells)))
    X.reset_guard()
    X.v.from_host(a)
    X.read("from_host")
    first = a.copy(order="F")
    S.O.zero_out_all_but_one(first, S.impl(cells), level)
    want = T.int_dot(first, first)
    got = hmg.norm_unique(X.v)
    assert got == math.sqrt(want) and round(got * got) == want, (got, want)
    np.testing.assert_array_equal(X.v.to_host(), a)
    X.read("norm_unique")

    # copy() and similar() are vectors of the prefix
    cp, sim = X.v.copy(), X.v.similar()
    assert cp.shape == sim.shape == (nf, cells)
    np.testing.assert_array_equal(cp.to_host(), a)
    assert hmg.dot(cp, X.v) == T.int_dot(a, a)
    assert not sim.to_host().any()
    cp.close(), sim.close()
    check("copy() and similar()", (Y, yi), (Z, y))
    X.read("copy() and similar()")


def test_norm_unique_at_full_size(ladder_grids):
    """... and on the grids nobody shrank (the full lattice: shared edges and nodes of every multiplicity)."""
    for dim in (2, 3):
        S = ladder_grids(dim)
        level = S.levels
        X = S.vectors(level)[0]
        cells = S.mesh.nelements()
        S.shrink(cells)
        a = np.asfortranarray(T.integers(np.random.default_rng(dim), (S.g.nf(level), cells)))
        X.v.from_host(a)
        first = a.copy(order="F")
        S.O.zero_out_all_but_one(first, S.impl(cells), level)
        want = T.int_dot(first, first)
        assert 0 < want < T.int_dot(a, a)
        assert hmg.norm_unique(X.v) == math.sqrt(want)
        X.read("norm_unique")


# ---- 2. the two reduction routes at their switch -----------------------------------------------------------------------------------
class SwitchProblem:
    """3D level 4 on 11 x 11 x 11 cubes: 7986 cells of 165 entries.  The oracle's smoothing step on each prefix mesh is computed
    once and shared by the fused and the unfused device run."""
    LAM = 0.7

    def __init__(self, O, ctx):
        dim, width, self.level = T.SWITCH_MESH
        self.O, self.ctx = O, ctx
        self.mesh = _cube(O, dim, width)
        self.sig = np.random.default_rng(61).choice([1.0, 9.0], size=(self.mesh.nelements(), dim))
        self.grids, self.want = {}, {}

    def grid(self, fused=1):
        if fused not in self.grids:
            self.ctx.set_option("fuse_cg", fused)                        # (read when a grid is created)
            try:
                g = hmg.ImplicitFineGrid(self.ctx, hmg.Mesh(self.mesh.nodes, self.mesh.elements + 1), self.level)
            finally:
                self.ctx.set_option("fuse_cg", 1)
            self.grids[fused] = (g, hmg.L2PlusDivAGrad(g, self.LAM, self.sig))
        return self.grids[fused]

    def smoothed(self, cells):
        """x0, b and the oracle's (x, r, p) after one smoothing step on the first `cells` cells, all nodes kept"""
        if cells not in self.want:
            O, lev = self.O, self.level
            sub = O.Mesh(self.mesh.nodes.copy(), np.ascontiguousarray(self.mesh.elements[:cells]))
            impl = O.ImplicitFineGrid.create(sub, lev)
            cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(sub))
            ref = impl.reference.levels[lev - 1]
            op = O.L2PlusDivAGrad(O.build_local_diffusion_operators(ref), O.mass_matrix(ref), cons, self.LAM,
                                  np.ascontiguousarray(self.sig[:cells]))
            rng = np.random.default_rng(cells)
            st = O.LevelState.create(cells, impl.nf(lev))
            st.x[...] = rng.standard_normal(st.x.shape)
            O.broadcast_interfaces(st.x, impl, lev)
            O.apply_constraint(st.x, lev, cons, impl)
            st.b[...] = rng.standard_normal(st.x.shape)
            x0, b = st.x.copy(order="F"), st.b.copy(order="F")
            O.smoothing_steps(1, impl, op, st, lev)
            self.want[cells] = (x0, b, st.x, st.r, st.p)
        return self.want[cells]

    def close(self):
        for g, A in self.grids.values():
            g.close()


@pytest.fixture(scope="module")
def switch(oracle, ctx):
    s = SwitchProblem(oracle, ctx)
    yield s
    s.close()


@pytest.fixture(scope="module")
def switch_vectors(ctx, switch):
    g, A = switch.grid(1)
    g.shrink(switch.mesh.nelements(), switch.mesh.nnodes())              # (wrapped at full size, whatever ran before)
    vs = [Wrapped(ctx, g, switch.level, s) for s in SENTINELS[:2]]
    yield vs
    for w in vs:
        w.close()


@pytest.mark.parametrize("dim,level,cells", T.SWITCH, ids=["2048-blocks-direct", "2049-blocks-folded", "2304-blocks-folded"])
def test_reductions_on_both_sides_of_the_route_switch(ctx, switch, switch_vectors, dim, level, cells):
    """dot and norm exact on integer data at the last length finalized directly (n = 1 048 575: odd, 255 pairs in the last block)
    and at the first one folded to 256 partials first (2049 blocks: no multiple of 256), and at 2304 blocks, where every one of the
    256 fold blocks holds partials and the last holds the vector's end; axpy with a = 3, where the fma is exact, against numpy; no
    call allocates -- the fold buffer was sized when the vectors were created on the full grid."""
    g, A = switch.grid(1)
    X, Y = switch_vectors
    g.shrink(cells, switch.mesh.nnodes())
    c = T.length_class(g.ld(level), cells)
    n = c["n"]
    assert c["nb"] == {6355: T.DIRECT_BLOCKS, 6356: T.DIRECT_BLOCKS + 1, 7149: 2304}[cells] and X.n() == n
    assert T.integer_sums_are_exact(9 * n)
    rng = np.random.default_rng(cells)
    x, y = T.integers(rng, n), T.integers(rng, n)
    x[0], y[0], x[-1], y[-1] = 8.0, 8.0, -7.0, 7.0                      # the first and the last product: 64 and -49, in no other sum
    X.write(x), Y.write(y)
    ctx.sync()
    allocs = ctx.counter("device_allocs")
    xy, xx, yy = int(np.dot(x, y)), int(np.dot(x, x)), int(np.dot(y, y))   # (integers below 2^53: numpy's sum is exact in any order)
    assert xy == T.int_dot(x, y)
    assert hmg.dot(X.v, Y.v) == xy and hmg.dot(X.v, X.v) == xx
    assert hmg.norm(Y.v) == math.sqrt(yy)
    x[0] = 0.0                                                           # ... and each of them alone
    X.write(x)
    assert hmg.dot(X.v, Y.v) == xy - 64
    x[0], x[-1] = 8.0, 0.0
    X.write(x)
    assert hmg.dot(X.v, Y.v) == xy + 49
    x[-1] = -7.0
    X.write(x)
    hmg.axpy(3.0, X.v, Y.v)
    y = 3.0 * x + y
    np.testing.assert_array_equal(Y.read("axpy"), y)
    assert hmg.dot(Y.v, Y.v) == int(np.dot(y, y))
    hmg.xpby(X.v, -2.0, Y.v)
    y = x - 2.0 * y
    np.testing.assert_array_equal(Y.read("xpby"), y)
    np.testing.assert_array_equal(X.read("xpby"), x)
    Y.v.copyto(X.v)
    X.v.fill(2.0)
    assert hmg.dot(X.v, Y.v) == 2 * int(x.sum())
    np.testing.assert_array_equal(Y.read("copy"), x)
    np.testing.assert_array_equal(X.read("fill"), np.full(n, 2.0))
    ctx.sync()
    assert ctx.counter("device_allocs") == allocs


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("cells", [k for _, _, k in T.SWITCH[:2]])
def test_smoothing_step_on_both_sides_of_the_route_switch(ctx, switch, cells, fused):
    """One step of the default CG smoother against the oracle at the two lengths: its reductions (r.r, p.Ap of the unfused form,
    the r-update's r.r of both) take the direct route at 6355 cells and the folded one at 6356."""
    g, A = switch.grid(fused)
    lev = switch.level
    g.shrink(cells, switch.mesh.nnodes())
    x0, b, wx, wr, wp = switch.smoothed(cells)
    dst = hmg.LevelState(g, lev)
    dst.x.from_host(x0)
    dst.b.from_host(b)
    hmg.smoothing_steps(1, g, A, dst, lev)
    ex, er, ep = relerr(dst.x.to_host(), wx), relerr(dst.r.to_host(), wr), relerr(dst.p.to_host(), wp)
    print(f"{cells} cells ({g.ld(lev) * cells} entries), fuse_cg {fused}: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
    dst.close()
    assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (ex, er, ep)


# ---- 3. the default CG smoother and the V-cycle at odd lengths ---------------------------------------------------------------------
class Shrunk:
    """A cube mesh less its last cell: the oracle's objects on the prefix mesh, device grids created on the full mesh and shrunk
    (the set-up of test_smoother_on_a_shrunk_grid_with_an_odd_number_of_entries in test_gpu_pcg_smoother.py, default smoother).
    The node prefix holds the nodes the kept cells use: all 27 in 3D; in 2D the dropped corner triangle is the only one at its
    corner, the last node."""

    def __init__(self, O, dim, width, levels, lam, seed):
        self.O, self.dim, self.levels, self.lam = O, dim, levels, lam
        self.full = _cube(O, dim, width)
        self.keep = self.full.nelements() - 1
        self.nn = int(self.full.elements[: self.keep].max()) + 1
        assert len(np.unique(self.full.elements[: self.keep])) == self.nn
        self.rng = np.random.default_rng(seed)
        self.sig_full = self.rng.choice([1.0, 9.0], size=(self.full.nelements(), dim))
        self.sig = np.ascontiguousarray(self.sig_full[: self.keep])
        self.mesh = O.Mesh(self.full.nodes[: self.nn].copy(), np.ascontiguousarray(self.full.elements[: self.keep]))
        self.impl = O.ImplicitFineGrid.create(self.mesh, levels)
        self.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(self.mesh))
        self._ops = {}

    def op(self, lev):
        if lev not in self._ops:
            O, ref = self.O, self.impl.reference.levels[lev - 1]
            self._ops[lev] = O.L2PlusDivAGrad(O.build_local_diffusion_operators(ref), O.mass_matrix(ref), self.cons, self.lam, self.sig)
        return self._ops[lev]

    def device(self, ctx, levels=None, fused=1):
        ctx.set_option("fuse_cg", fused)                                  # (read when a grid is created)
        try:
            g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.full.nodes, self.full.elements + 1), levels or self.levels)
        finally:
            ctx.set_option("fuse_cg", 1)
        A = hmg.L2PlusDivAGrad(g, self.lam, self.sig_full)
        g.shrink(self.keep, self.nn)
        assert g.ncells() == self.keep and g.smoother() == "cg"
        return g, A

    def state(self, lev):
        O = self.O
        st = O.LevelState.create(self.keep, self.impl.nf(lev))
        st.x[...] = self.rng.standard_normal(st.x.shape)
        O.broadcast_interfaces(st.x, self.impl, lev)
        O.apply_constraint(st.x, lev, self.cons, self.impl)
        st.b[...] = self.rng.standard_normal(st.x.shape)
        return st


@pytest.fixture(scope="module")
def tets47(oracle):
    """47 of the 48 tetrahedra of 2 x 2 x 2 cubes, six levels"""
    return Shrunk(oracle, 3, 2, 6, 1.0, 47)


@pytest.fixture(scope="module")
def tris31(oracle):
    """31 of the 32 triangles of 4 x 4 squares, five levels"""
    return Shrunk(oracle, 2, 4, 5, 1.0, 31)


def _check_smoother(P, ctx, fused, levels_checked):
    O = P.O
    g, A = P.device(ctx, levels=max(levels_checked), fused=fused)
    for lev in levels_checked:
        n = g.ld(lev) * g.ncells()
        assert n & 1, (lev, n)
        for steps in (1, 2, 3):
            st = P.state(lev)
            dst = hmg.LevelState(g, lev)
            dst.x.from_host(st.x)
            dst.b.from_host(st.b)
            O.smoothing_steps(steps, P.impl, P.op(lev), st, lev)
            hmg.smoothing_steps(steps, g, A, dst, lev)
            ex, er, ep = relerr(dst.x.to_host(), st.x), relerr(dst.r.to_host(), st.r), relerr(dst.p.to_host(), st.p)
            print(f"level {lev} ({n} entries), {steps} steps, fuse_cg {fused}: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
            dst.close()
            assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (lev, steps, ex, er, ep)
    g.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_cg_smoother_3d_odd_lengths(ctx, tets47, fused):
    """hmg_smooth, default smoother, 1 to 3 steps on levels 3, 4, 5 of the 47-cell grid (35, 165, 969 entries per cell: every
    length odd, flat pairs straddle columns, k_cg_rupdate_faces finds the cell of both halves of such a pair) against the
    oracle's smoothing_steps on the 47-cell mesh."""
    _check_smoother(tets47, ctx, fused, [3, 4, 5])


@pytest.mark.parametrize("fused", [1, 0])
def test_cg_smoother_2d_odd_lengths(ctx, tris31, fused):
    """The same on 31 triangles, levels 4 and 5 (45 and 153 entries per cell)."""
    _check_smoother(tris31, ctx, fused, [4, 5])


@pytest.mark.parametrize("top,steps", [(4, 3), (5, 3), (6, 3), (5, 2)])
def test_vcycle_odd_lengths(ctx, tets47, top, steps):
    """Two hmg_vcycle with default options on the 47-cell grid against the oracle's on the 47-cell mesh.  Top level 6 takes the
    forms that leave x-updates and the last r-update pending (the counter says so); the downloads are the reads that settle them."""
    P, O = tets47, tets47.O
    g, A = P.device(ctx, levels=top)
    ops = [P.op(l) for l in range(1, top + 1)]
    sts = [O.LevelState.create(P.keep, P.impl.nf(i + 1)) for i in range(top)]
    sts[-1] = P.state(top)
    dsts = [hmg.LevelState(g, i + 1) for i in range(top)]
    dsts[-1].x.from_host(sts[-1].x)
    dsts[-1].b.from_host(sts[-1].b)
    assert (g.ld(top) * g.ncells()) & 1
    base, dbase = O.make_base_level(P.mesh, P.sig, P.lam), hmg.BaseLevel(g)
    for _ in range(2):
        O.vcycle(P.impl, base, ops, sts, top, steps)
        hmg.vcycle(g, dbase, [A] * top, dsts, top, steps)
    form = ctx.counter("lazy_x_form")
    assert form == ((3 if steps == 3 else 2) if top == 6 else 0), form
    ex = relerr(dsts[-1].x.to_host(), sts[-1].x)
    er = relerr(dsts[-1].r.to_host(), sts[-1].r)
    print(f"top level {top}, {steps} steps, lazy_x_form {form}: x {ex:.2e}  r {er:.2e}")
    for s in dsts:
        s.close()
    g.close()
    assert ex <= 1e-9 and er <= 1e-8, (ex, er)


# ---- 4. the flexible CG at odd lengths and on arrival ------------------------------------------------------------------------------
@pytest.mark.parametrize("which,top", [("tets47", 4), ("tets47", 6), ("tris31", 5)])
def test_fcg_odd_lengths(request, ctx, which, top):
    """Three steps of hmg_fcg_* on the shrunk grids against fcg_local on the prefix mesh, then the residual norm: every k_fcg_*
    kernel runs its tail entry."""
    P = request.getfixturevalue(which)
    assert (T.NF[P.dim][top - 1] * P.keep) & 1
    _against_local(P.O, ctx, P.mesh, P.sig, P.lam, top, 3, 3, np.random.default_rng(50 + top), full=(P.full, P.sig_full),
                   check_residual_norm=True)


def test_fcg_that_has_arrived_adds_nothing(ctx, tets47):
    """b = 0 and x0 = 0 on the 47-cell grid, top level 4 (7755 entries), Chebyshev smoother: that smoother forms no reduction and
    the level-1 solve returns at once for a right-hand side with b.b = 0, so z = V(0, 0) is exactly zero.  The first step takes
    k_fcg_update's branch p.q = 0 -> alpha = 0, the second k_fcg_direction's (p.q)_prev = 0 -> beta = 0: x, R and p stay exactly
    zero and every scalar is finite.  (With the default CG smoother the same input is 0 / 0 inside the smoother, as it is in the
    reference; that is neither asserted nor changed here.)"""
    P, top = tets47, 4
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(P.full.nodes, P.full.elements + 1), top)
    g.set_smoother("chebyshev")
    A = hmg.L2PlusDivAGrad(g, P.lam, P.sig_full)
    g.shrink(P.keep, P.nn)
    n = g.ld(top) * g.ncells()
    assert n & 1
    sts = [hmg.LevelState(g, i + 1) for i in range(top)]
    x, b = hmg.DeviceMatrix(g, top), hmg.DeviceMatrix(g, top)
    x.fill(0.0), b.fill(0.0)
    f = hmg.FlexibleCG(g, hmg.BaseLevel(g), [A] * top, sts, top, 3)
    f.start(x, b)
    for step in (1, 2):
        f.step()
        alpha, beta, pq, pr = f.scalars()
        assert all(math.isfinite(v) for v in (alpha, beta, pq, pr)), (step, alpha, beta, pq, pr)
        assert alpha == 0.0 and beta == 0.0 and pq == 0.0, (step, alpha, beta, pq)
        for name, a in (("x", x.to_host()), ("R", f.vec("R")), ("p", f.vec("p")), ("z", sts[-1].x.to_host())):
            assert a.shape == (g.nf(top), P.keep) and not a.any(), (step, name)
    assert f.residual_norm() == 0.0
    f.close()
    for v in [x, b] + sts:
        v.close()
    g.close()


# ---- 5. alignment of wrapped memory ------------------------------------------------------------------------------------------------
def test_wrap_refuses_memory_that_is_not_16_byte_aligned(ctx, ladder_grids):
    """The flat-pair kernels read the storage as double2.  hmg_vec_wrap says so before anything is allocated or launched: no
    kernel ever sees the odd pointer."""
    import torch
    S = ladder_grids(3)
    S.shrink(S.mesh.nelements())
    level = S.levels
    t = torch.zeros(S.g.ld(level) * S.g.ncells() + 2, dtype=torch.float64, device="cuda")
    assert t.data_ptr() % 16 == 0 and t[1:].data_ptr() % 16 == 8
    ctx.sync()
    allocs = ctx.counter("device_allocs")
    with pytest.raises(HmgError, match="16-byte aligned"):
        hmg.DeviceMatrix(S.g, level, device_ptr=t[1:].data_ptr())
    assert ctx.counter("device_allocs") == allocs
    for ptr in (t.data_ptr(), t[2:].data_ptr()):
        v = hmg.DeviceMatrix(S.g, level, device_ptr=ptr)
        v.fill(1.0)
        assert hmg.dot(v, v) == S.g.ld(level) * S.g.ncells()
        v.close()
