"""GPU tests of the per-cell gradient moments (hmg_cell_moments, csrc/hmg_fields.hip) against the CPU statement of
tests/_cell_moments_form.py (pinned by tests/test_cell_moments_statement.py).  Smallest shapes that reach every path: 3D 48 cells on
levels 2-4 (one wave per workgroup), 5 (256 threads) and six cells on level 6 (512 threads, the 52 KB image and its guard); 2D 18
cells on levels 2, 5 (one wave), 8 (512 threads, 67 KB); Delaunay meshes in 2D and 3D, whose J is neither diagonal nor a
permutation and whose cells have both orientations.  Bound: 1e-11 of the largest magnitude of the quantity over the cells, the
project's bound for the apply (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
import _cell_moments_form as F
import _meshes
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def build(O, name):
    if name == "cube":
        return O.hypercube(3, 2), 5
    if name == "cube6":
        return O.hypercube(3, 1), 6
    if name == "square":
        return O.hypercube(2, 3), 8
    if name == "delaunay2":
        return _meshes.delaunay_mesh(O, 2, 14, 3), 4
    return _meshes.delaunay_mesh(O, 3, 12, 4), 3


CASES = [("cube", 2), ("cube", 3), ("cube", 4), ("cube", 5), ("cube6", 6), ("square", 2), ("square", 5), ("square", 8),
         ("delaunay2", 4), ("delaunay3", 3)]
_cache = {}


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per mesh: oracle mesh and implicit grid, device grid; per (mesh, level): a consistent random vector and its moments"""
    def get(name, level):
        O = oracle
        if name not in _cache:
            base, grids = build(O, name)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            v = F.consistent_random(O, implicit, level, np.random.default_rng(100 + level))
            _cache[(name, level)] = (v,) + F.reference_form(O, implicit, level, v)
        return (base, implicit, g) + _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def errs(mean, gram, want_mean, want_gram):
    return (np.abs(mean - want_mean).max() / np.abs(want_mean).max(), np.abs(gram - want_gram).max() / np.abs(want_gram).max())


@pytest.mark.parametrize("name,level", CASES)
def test_device_against_the_statement(oracle, shapes, name, level):
    base, implicit, g, v, want_mean, want_gram = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    mean, gram = hmg.cell_moments(dv, g)
    e1, e2 = errs(mean, gram, want_mean, want_gram)
    print(f"{name} level {level}: mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    np.testing.assert_array_equal(gram, np.swapaxes(gram, 1, 2))
    # with xi: the moments of u = xi.x + v
    xi = np.array([0.6, -0.3, 0.5])[:base.dim]
    mu, gu = hmg.cell_moments(dv, g, xi)
    wm, wg = F.with_xi(want_mean, want_gram, F.cell_volumes(oracle, base), xi)
    e1, e2 = errs(mu, gu, wm, wg)
    print(f"{name} level {level}: with xi mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    # the same bits in a second call
    mean2, gram2 = hmg.cell_moments(dv, g)
    np.testing.assert_array_equal(mean2, mean)
    np.testing.assert_array_equal(gram2, gram)
    dv.close()


@pytest.mark.parametrize("name,level", CASES)
def test_linear_field_on_the_device(oracle, shapes, name, level):
    O = oracle
    base, implicit, g = shapes(name, level)[:3]
    gvec = np.array([0.7, -1.3, 0.45])[:base.dim]
    dv = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(O, implicit, level, gvec))
    vol = F.cell_volumes(O, base)
    mean, gram = hmg.cell_moments(dv, g)
    want = vol[:, None, None] * np.outer(gvec, gvec)[None]
    e1 = np.abs(mean - gvec[None, :]).max() / np.abs(gvec).max()
    e2 = np.abs(gram - want).max() / np.abs(want).max()
    print(f"{name} level {level}: m_v = g {e1:.2e}, G_v = |c| g g^T {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    xi = np.array([0.25, 0.5, -1.0])[:base.dim]
    mu, _ = hmg.cell_moments(dv, g, xi)
    e3 = np.abs(mu - (xi + gvec)[None, :]).max() / np.abs(xi + gvec).max()
    print(f"{name} level {level}: m_u = xi + g {e3:.2e}")
    assert e3 <= TOL
    dv.close()


@pytest.mark.parametrize("name,level", [c for c in CASES if c[0] in ("cube", "square")])
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
    _, gram = hmg.cell_moments(dv, g)
    got = np.einsum("ekl,ekl->e", sig, gram)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{name} level {level}: sigma:G vs v.(A v) {err:.2e}")
    assert err <= TOL
    dv.close()
    out.close()


def test_shrink_gives_the_prefix_bit_for_bit(oracle, ctx):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 4, origin=(-2.0, -2.0, -2.0)))
    level = 3
    implicit = O.ImplicitFineGrid.create(m, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), level)
    hmg.L2PlusDivAGrad(g, 0.0, np.ones((m.nelements(), 3)))            # (a shrink re-forms the operator's tables)
    v = F.consistent_random(O, implicit, level, np.random.default_rng(9))
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    xi = np.array([0.3, 0.2, -0.7])
    mean, gram = hmg.cell_moments(dv, g, xi)
    ne, nn = O.find_elements_in_radius(m, 1.0), O.find_nodes_in_radius(m, 1.0)
    assert 0 < ne < m.nelements()
    g.shrink(ne, nn)
    mean2, gram2 = hmg.cell_moments(dv, g, xi)
    assert mean2.shape == (ne, 3) and gram2.shape == (ne, 3, 3)
    np.testing.assert_array_equal(mean2, mean[:ne])                    # the moments do not see the boundary
    np.testing.assert_array_equal(gram2, gram[:ne])
    dv.close()
    g.close()


@pytest.mark.parametrize("dim,level", [(3, 7), (2, 9)])
def test_large_cells_are_refused_and_the_context_goes_on(oracle, ctx, dim, level):
    O = oracle
    base = O.hypercube(dim, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    dv = hmg.DeviceMatrix(g, level)
    with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS"):
        hmg.cell_moments(dv, g)
    # another grid's vector is refused too
    g2 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(hmg._lib.HmgError, match="another grid"):
        hmg.cell_moments(dv, g2)
    # ... and the next call on the same context succeeds
    d2 = hmg.DeviceMatrix(g, 2).from_host(F.linear_interpolant(O, O.ImplicitFineGrid.create(base, 2), 2, np.ones(dim)))
    mean, _ = hmg.cell_moments(d2, g)
    assert np.abs(mean - 1.0).max() <= TOL
    for o in (dv, d2, g2, g):
        o.close()


def fd_check(ctx, n, eltype, refinements, xi, seed, cell):
    r = driver.dirichlet_homogenization(n, eltype, refinements, xi, ctx=ctx, seed=seed, fields=True)
    e, f = r["energy_form"], r["flux_form"]
    err = abs(e - np.dot(xi, f)) / abs(e)
    print(f"n {n} {eltype}: energy form {e:.15g} xi.flux form {np.dot(xi, f):.15g} ({err:.2e}), {r['cycles']} cycles, "
          f"residual {r['residual']:.2e}")
    assert r["residual"] <= 1e-10
    assert err <= 1e-8
    eps, es = 1e-4, []
    for s in (+1.0, -1.0):
        cond = r["cond"].copy()
        cond[cell, 0] += s * eps
        q = driver.dirichlet_homogenization(n, eltype, refinements, xi, ctx=ctx, cond=cond)
        es.append(q["energy_form"] * q["volume"])
    fd = (es[0] - es[1]) / (2 * eps)
    G = r["gram"][cell, 0, 0]
    err = abs(fd - G) / abs(G)
    print(f"n {n} {eltype}: central difference {fd:.12g}, gram[{cell}, 0, 0] {G:.12g} ({err:.2e})")
    assert err <= 1e-6


def test_dirichlet_homogenization_2d(ctx):
    fd_check(ctx, 3, hmg.Tri64, 3, np.array([0.6, 0.8]), 2, 7)


def test_dirichlet_homogenization_3d(ctx):
    fd_check(ctx, 2, hmg.Tet64, 2, np.array([0.6, 0.0, 0.8]), 2, 20)


@pytest.mark.parametrize("accelerate", [False, True])
def test_dirichlet_homogenization_uniform_medium(ctx, accelerate):
    xi = np.array([0.6, 0.8])
    r = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, ctx=ctx, sigma_grid=np.full((3, 3, 2), 3.0), accelerate=accelerate)
    print("uniform medium:", r["flux_form"], r["energy_form"], r["cycles"])
    assert r["cycles"] in (0, 1)
    np.testing.assert_allclose(r["flux_form"], 3.0 * xi, rtol=1e-12)
    np.testing.assert_allclose(r["energy_form"], 3.0, rtol=1e-12)


def test_dirichlet_homogenization_accelerated_agrees(ctx):
    xi = np.array([0.6, 0.8])
    a = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, ctx=ctx, seed=2)
    b = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, ctx=ctx, seed=2, accelerate=True, smoother="jacobi")
    print("V-cycles", a["cycles"], a["energy_form"], "FCG + jacobi", b["cycles"], b["energy_form"])
    assert abs(a["energy_form"] - b["energy_form"]) <= 1e-8 * abs(a["energy_form"])
    np.testing.assert_allclose(a["flux_form"], b["flux_form"], rtol=1e-8)


def test_no_allocation_appears_inside_a_vcycle(ctx, oracle):
    """hmg_cell_moments may allocate; a V-cycle after it still makes none"""
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, 3, seed=0)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(3)]
    states[-1].b.rand(3)
    hmg.vcycle(g, bl, [op] * 3, states, 3, 3)
    hmg.cell_moments(states[-1].x, g)
    ctx.sync()
    n0 = ctx.counter("device_allocs")
    hmg.vcycle(g, bl, [op] * 3, states, 3, 3)
    ctx.sync()
    assert ctx.counter("device_allocs") == n0
    for st in states:
        st.close()
    g.close()
