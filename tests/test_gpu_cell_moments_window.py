"""GPU tests of the per-cell moments of cells larger than the LDS (context option "cell_moments_windows",
csrc/hmg_fields_window.hip: k_cell_pair_moments_slab for 3D level 7, k_cell_pair_moments_rows for 2D levels 9-11) against the CPU
statements of tests/_cell_moments_form.py and tests/_cell_pair_moments_form.py (`reference_form`), on consistent random vectors.
Shapes: 3D level 7 on hypercube(3, 1) with perturbed nodes (6 cells, 9 slabs; J neither diagonal nor a permutation); 2D level 9 on
n = 2, perturbed (8 cells, several bands); 2D levels 10 and 11 on n = 1 (level 11: rows of 1 025 nodes, wider than the workgroup, the
two-row move near its limit, short bands).  The same grids carry the levels of the kernel-against-kernel check of option value 2:
3D level 6 (one slab), 2D levels 2 (m = 2: no interior), 3, 4 and 8 (a single band).
Bound: TOL = 1e-11 of the largest magnitude over the cells, the project's bound of tests/test_gpu_cell_moments.py (pairs: of the
Cauchy-Schwarz scale of tests/test_gpu_cell_pair_moments.py); on the CPU the two independent statements agree at these shapes to
1.5e-12 (mean) / 4e-14 (gram) in 3D and 6e-14 / 1.1e-13 in 2D.  The context is this module's own: the option is set on it and
restored at teardown."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
import _cell_moments_form as F
import _cell_pair_moments_form as P
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
OPT, COUNTER = "cell_moments_windows", "cell_moments_window_launches"
# name: dim, n, finest level
GRIDS = {"cube7": (3, 1, 7), "square9": (2, 2, 9), "square10": (2, 1, 10), "square11": (2, 1, 11)}
LARGE = [("cube7", 7), ("square9", 9), ("square10", 10), ("square11", 11)]
FITTING = [("cube7", 6), ("square9", 2), ("square9", 3), ("square9", 4), ("square9", 8)]
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    prev = c.counter(OPT)
    c.set_option(OPT, 1)
    yield c
    c.set_option(OPT, prev)
    c.close()


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per grid: perturbed oracle mesh, implicit grid, device grid; per (grid, level): two consistent random vectors and their
    reference forms (computed once, read only)"""
    def get(name, level):
        O = oracle
        if name not in _cache:
            dim, n, grids = GRIDS[name]
            base = O.hypercube(dim, n)
            base.nodes = base.nodes + 0.2 * (np.random.default_rng(5).random(base.nodes.shape) - 0.5)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            v = F.consistent_random(O, implicit, level, np.random.default_rng(100 + level))
            w = F.consistent_random(O, implicit, level, np.random.default_rng(200 + level))
            K = O.build_local_diffusion_operators(implicit.reference.levels[level - 1])
            mean_v, gram_v = F.reference_form(O, implicit, level, v, K)
            gram_w = F.reference_form(O, implicit, level, w, K)[1]
            _cache[(name, level)] = (v, w, mean_v, gram_v, gram_w, P.reference_form(O, implicit, level, v, w, K))
        return (base, implicit, g) + _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("name,level", LARGE)
def test_device_against_the_statement(oracle, ctx, shapes, name, level):
    O = oracle
    base, implicit, g, v, w, mean_v, gram_v, gram_w, (mv, mw, pair) = shapes(name, level)
    vol = F.cell_volumes(O, base)
    dv, dw = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(w)
    n0 = ctx.counter(COUNTER)
    mean, gram = hmg.cell_moments(dv, g)
    assert ctx.counter(COUNTER) == n0 + 1
    assert ctx.counter("cell_moments_kernel_ns") > 0 and ctx.counter("cell_moments_download_ns") > 0
    e1, e2 = rel(mean, mean_v), rel(gram, gram_v)
    print(f"{name} level {level}: mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    np.testing.assert_array_equal(gram, np.swapaxes(gram, 1, 2))
    xi = np.array([0.6, -0.3, 0.5])[:base.dim]
    mu, gu = hmg.cell_moments(dv, g, xi)
    wm, wg = F.with_xi(mean_v, gram_v, vol, xi)
    e1, e2 = rel(mu, wm), rel(gu, wg)
    print(f"{name} level {level}: with xi mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    # the pair form on two different vectors
    sc = P.scale(gram_v, gram_w)
    S = hmg.cell_pair_moments(dv, dw, g)
    assert ctx.counter(COUNTER) == n0 + 3
    assert ctx.counter("cell_pair_moments_kernel_ns") > 0 and ctx.counter("cell_pair_moments_download_ns") > 0
    e = np.abs(S - pair).max() / sc
    print(f"{name} level {level}: pair against the reference form {e:.2e}")
    assert e <= TOL
    np.testing.assert_array_equal(S, np.swapaxes(S, 1, 2))
    xv, xw = np.array([0.6, -0.3, 0.5])[:base.dim], np.array([-0.2, 0.9, 0.4])[:base.dim]
    for a, b in ((xv, xw), (xv, None), (None, xw)):
        Su = hmg.cell_pair_moments(dv, dw, g, a, b)
        gu_ = gram_v if a is None else F.with_xi(mv, gram_v, vol, a)[1]
        gz_ = gram_w if b is None else F.with_xi(mw, gram_w, vol, b)[1]
        e = np.abs(Su - P.with_xi(mv, mw, pair, vol, a, b)).max() / min(sc, P.scale(gu_, gz_))
        print(f"{name} level {level}: pair with xi_v {a is not None} xi_w {b is not None} {e:.2e}")
        assert e <= TOL
        np.testing.assert_array_equal(Su, np.swapaxes(Su, 1, 2))
    # the operands exchanged
    e = np.abs(hmg.cell_pair_moments(dw, dv, g) - S).max() / sc
    print(f"{name} level {level}: pair(w, v) against pair(v, w) {e:.2e}")
    assert e <= TOL
    # one handle twice: the same kernel and the same host arithmetic as cell_moments -- the same bits
    np.testing.assert_array_equal(hmg.cell_pair_moments(dv, dv, g), gram)
    # the same bits in a second call
    mean2, gram2 = hmg.cell_moments(dv, g)
    np.testing.assert_array_equal(mean2, mean)
    np.testing.assert_array_equal(gram2, gram)
    np.testing.assert_array_equal(hmg.cell_pair_moments(dv, dw, g), S)
    dv.close()
    dw.close()


@pytest.mark.parametrize("name,level", LARGE)
def test_linear_field_on_the_device(oracle, shapes, name, level):
    O = oracle
    base, implicit, g = shapes(name, level)[:3]
    gvec, hvec = np.array([0.7, -1.3, 0.45])[:base.dim], np.array([-0.4, 0.8, 1.1])[:base.dim]
    dv = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(O, implicit, level, gvec))
    dw = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(O, implicit, level, hvec))
    vol = F.cell_volumes(O, base)
    mean, gram = hmg.cell_moments(dv, g)
    want = vol[:, None, None] * np.outer(gvec, gvec)[None]
    e1 = np.abs(mean - gvec[None, :]).max() / np.abs(gvec).max()
    e2 = rel(gram, want)
    print(f"{name} level {level}: m_v = g {e1:.2e}, G_v = |c| g g^T {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    wantp = vol[:, None, None] * P.sym(np.outer(gvec, hvec))[None]
    sc = P.scale(want, vol[:, None, None] * np.outer(hvec, hvec)[None])
    e3 = np.abs(hmg.cell_pair_moments(dv, dw, g) - wantp).max() / sc
    print(f"{name} level {level}: S = |c| sym(g h^T) {e3:.2e}")
    assert e3 <= TOL
    dv.close()
    dw.close()


@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_energy_identity_with_a_tensor_operator(oracle, shapes, name, level):
    """sigma_c : G_v(c) = v_c . (K_c v_c): the library's own apply (lambda = 0, no constraint), both downloaded"""
    base, implicit, g, v = shapes(name, level)[:4]
    sig = T.random_spd(np.random.default_rng(7), base.nelements(), base.dim)
    A = hmg.L2PlusDivAGrad(g, 0.0, sig)
    A._bind()
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    out = hmg.DeviceMatrix(g, level)
    hmg.apply_ex(1.0, g, dv, None, out, constrain=False)
    want = np.einsum("ie,ie->e", v, out.to_host())
    got = np.einsum("ekl,ekl->e", sig, hmg.cell_moments(dv, g)[1])
    err = rel(got, want)
    print(f"{name} level {level}: sigma:G vs v.(A v) {err:.2e}")
    assert err <= TOL
    dv.close()
    out.close()


def moments_at(ctx, value, dv, dw, g, xi, xw):
    """cell_moments and cell_pair_moments with the option at `value`, and how many window launches that took"""
    prev = ctx.counter(OPT)
    ctx.set_option(OPT, value)
    try:
        n0 = ctx.counter(COUNTER)
        mean, gram = hmg.cell_moments(dv, g, xi)
        S = hmg.cell_pair_moments(dv, dw, g, xi, xw)
        return mean, gram, S, ctx.counter(COUNTER) - n0
    finally:
        ctx.set_option(OPT, prev)


@pytest.mark.parametrize("name,level", FITTING)
def test_window_kernels_against_the_lds_kernels(ctx, shapes, name, level):
    """option value 2 sends a level that fits the LDS through the window kernels: kernel against kernel, 1e-12 (the summation
    orders differ: no bits); value 1 leaves such a level to the LDS kernels -- the bits of value 0, no window launch"""
    base, implicit, g, v, w, _, gram_v, gram_w = shapes(name, level)[:8]
    dv, dw = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(w)
    xi, xw = np.array([0.6, -0.3, 0.5])[:base.dim], np.array([-0.2, 0.9, 0.4])[:base.dim]
    for a, b in ((None, None), (xi, xw)):
        m0, g0, s0, k0 = moments_at(ctx, 0, dv, dw, g, a, b)
        m1, g1, s1, k1 = moments_at(ctx, 1, dv, dw, g, a, b)
        m2, g2, s2, k2 = moments_at(ctx, 2, dv, dw, g, a, b)
        assert (k0, k1, k2) == (0, 0, 2)
        for x, y in ((m0, m1), (g0, g1), (s0, s1)):
            np.testing.assert_array_equal(x, y)
        gz = hmg.cell_moments(dw, g, b)[1]                              # (the module's option value 1: the LDS kernel)
        e = (rel(m2, m0), rel(g2, g0), np.abs(s2 - s0).max() / P.scale(g0, gz))
        print(f"{name} level {level} xi {a is not None}: window against LDS kernels mean {e[0]:.2e} gram {e[1]:.2e} pair {e[2]:.2e}")
        assert max(e) <= 1e-12
    dv.close()
    dw.close()


@pytest.mark.parametrize("name,level", [("cube7", 3), ("cube7", 5), ("cube7", 6), ("square9", 2), ("square9", 8), ("cube7", 7),
                                        ("square9", 9)])
def test_equal_values_in_two_handles_give_the_bits_of_one_handle(oracle, shapes, name, level):
    """two handles take the two-column instantiation of a kernel, one handle given twice the one-column instantiation: on equal
    values the same bits.  One level per thread count of the LDS kernel (3D levels 3, 5, 6: 64, 256, 512 threads; 2D level 2,
    m = 2 without interior, and level 8) and one per window kernel (3D level 7, 2D level 9; the module's option value 1)."""
    base, implicit, g = shapes(name, GRIDS[name][2])[:3]
    v = F.consistent_random(oracle, implicit, level, np.random.default_rng(100 + level))
    dv, dc = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(v)
    xv, xw = np.array([0.6, -0.3, 0.5])[:base.dim], np.array([-0.2, 0.9, 0.4])[:base.dim]
    for a, b in ((None, None), (xv, xw)):
        np.testing.assert_array_equal(hmg.cell_pair_moments(dv, dc, g, a, b), hmg.cell_pair_moments(dv, dv, g, a, b))
    dv.close()
    dc.close()


def test_shrink_gives_the_prefix_bit_for_bit(oracle, ctx):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, 4, origin=(-2.0, -2.0)))
    level = 9
    implicit = O.ImplicitFineGrid.create(m, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), level)
    hmg.L2PlusDivAGrad(g, 0.0, np.ones((m.nelements(), 2)))            # (a shrink re-forms the operator's tables)
    dv = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(9)))
    dw = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(10)))
    xv, xw = np.array([0.3, -0.7]), np.array([-0.5, 0.4])
    mean, gram = hmg.cell_moments(dv, g, xv)
    S = hmg.cell_pair_moments(dv, dw, g, xv, xw)
    ne, nn = O.find_elements_in_radius(m, 1.0), O.find_nodes_in_radius(m, 1.0)
    assert 0 < ne < m.nelements()
    g.shrink(ne, nn)
    mean2, gram2 = hmg.cell_moments(dv, g, xv)
    S2 = hmg.cell_pair_moments(dv, dw, g, xv, xw)
    assert mean2.shape == (ne, 2) and gram2.shape == (ne, 2, 2) and S2.shape == (ne, 2, 2)
    np.testing.assert_array_equal(mean2, mean[:ne])                    # the moments do not see the boundary
    np.testing.assert_array_equal(gram2, gram[:ne])
    np.testing.assert_array_equal(S2, S[:ne])
    for o in (dv, dw, g):
        o.close()


def test_no_allocation_appears_inside_a_vcycle(ctx):
    """the moments of 3D level 7 may allocate; a V-cycle after them still makes none"""
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, 7, seed=0)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(7)]
    states[-1].b.rand(3)
    hmg.vcycle(g, bl, [op] * 7, states, 7, 3)
    n0 = ctx.counter(COUNTER)
    hmg.cell_moments(states[-1].x, g)
    hmg.cell_pair_moments(states[-1].x, states[-1].r, g)
    ctx.sync()
    assert ctx.counter(COUNTER) == n0 + 2
    a0 = ctx.counter("device_allocs")
    hmg.vcycle(g, bl, [op] * 7, states, 7, 3)
    ctx.sync()
    assert ctx.counter("device_allocs") == a0
    for st in states:
        st.close()
    g.close()


@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_the_refusal_returns_with_the_option_and_the_context_goes_on(ctx, shapes, name, level):
    base, implicit, g, v, w, mean_v = shapes(name, level)[:6]
    dv, dw = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(w)
    n0 = ctx.counter(COUNTER)
    ctx.set_option(OPT, 0)
    try:
        with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS.*{OPT}"):
            hmg.cell_moments(dv, g)
        with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS.*{OPT}"):
            hmg.cell_pair_moments(dv, dw, g)
    finally:
        ctx.set_option(OPT, 1)
    assert ctx.counter(COUNTER) == n0
    assert rel(hmg.cell_moments(dv, g)[0], mean_v) <= TOL
    assert ctx.counter(COUNTER) == n0 + 1
    with pytest.raises(hmg._lib.HmgError, match="0, 1 or 2"):
        ctx.set_option(OPT, 3)
    assert ctx.counter(OPT) == 1
    dv.close()
    dw.close()
