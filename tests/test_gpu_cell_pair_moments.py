"""GPU tests of the per-cell pair moments (hmg_cell_pair_moments, csrc/hmg_fields.hip) against the CPU statement of
tests/_cell_pair_moments_form.py (pinned by tests/test_cell_pair_moments_statement.py), and of what is built on them
(driver.dirichlet_homogenization_tensor, fields.tensor_sensitivity).  The shapes are those of tests/test_gpu_cell_moments.py, the
smallest that reach every path: 3D 48 cells on levels 2-4 (one wave per workgroup), 5 (256 threads) and six cells on level 6 (512
threads, the 52 KB image and its guard); 2D 18 cells on levels 2, 5 (one wave), 8 (512 threads, 67 KB); Delaunay meshes in 2D and
3D.  Bound: 1e-11, the project's bound for the apply (tests/test_gpu_parity.py), on max |got - want| / sqrt(max |G_v| max |G_w|)
over cells and entries: the Cauchy-Schwarz scale of a cross moment, which a small cross term does not inflate.
Measured on the MI355X: at most 6e-16 against the statement, the exchanged operands and the polarised single-vector kernel,
5.2e-13 on linear fields (level 6), 3e-16 in the energy identity; the sensitivities 2e-12 / 8e-10 / 6e-12 of their bound 1e-6."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver, fields
import _cell_moments_form as F
import _cell_pair_moments_form as P
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
    """per mesh: oracle mesh and implicit grid, device grid; per (mesh, level): two different consistent random vectors, their
    Gram tensors and the reference form of the pair (computed once, read only)"""
    def get(name, level):
        O = oracle
        if name not in _cache:
            base, grids = build(O, name)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            v = F.consistent_random(O, implicit, level, np.random.default_rng(100 + level))
            w = F.consistent_random(O, implicit, level, np.random.default_rng(200 + level))
            gv, gw = F.reference_form(O, implicit, level, v)[1], F.reference_form(O, implicit, level, w)[1]
            _cache[(name, level)] = (v, w, gv, gw, P.reference_form(O, implicit, level, v, w))
        return (base, implicit, g) + _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


@pytest.mark.parametrize("name,level", CASES)
def test_device_against_the_statement(oracle, shapes, name, level):
    O = oracle
    base, implicit, g, v, w, gv, gw, (mv, mw, want) = shapes(name, level)
    sc = P.scale(gv, gw)
    dv, dw = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(w)
    S = hmg.cell_pair_moments(dv, dw, g)
    assert S.shape == (base.nelements(), base.dim, base.dim)
    e = np.abs(S - want).max() / sc
    print(f"{name} level {level}: pair against the reference form {e:.2e}")
    assert e <= TOL
    np.testing.assert_array_equal(S, np.swapaxes(S, 1, 2))
    # with two different xi: the pair moment of u = xi_v.x + v and z = xi_w.x + w; the scale is the smaller of (v, w)'s and (u, z)'s
    vol = F.cell_volumes(O, base)
    xv, xw = np.array([0.6, -0.3, 0.5])[:base.dim], np.array([-0.2, 0.9, 0.4])[:base.dim]
    for a, b in ((xv, xw), (xv, None), (None, xw)):
        Su = hmg.cell_pair_moments(dv, dw, g, a, b)
        gu = gv if a is None else F.with_xi(mv, gv, vol, a)[1]
        gz = gw if b is None else F.with_xi(mw, gw, vol, b)[1]
        e = np.abs(Su - P.with_xi(mv, mw, want, vol, a, b)).max() / min(sc, P.scale(gu, gz))
        print(f"{name} level {level}: with xi_v {a is not None} xi_w {b is not None} {e:.2e}")
        assert e <= TOL
        np.testing.assert_array_equal(Su, np.swapaxes(Su, 1, 2))
    # the operands exchanged
    e = np.abs(hmg.cell_pair_moments(dw, dv, g) - S).max() / sc
    print(f"{name} level {level}: pair(w, v) against pair(v, w) {e:.2e}")
    assert e <= TOL
    # the same handle twice: the Gram tensor of the single-vector kernel
    gram_v = hmg.cell_moments(dv, g)[1]
    e = np.abs(hmg.cell_pair_moments(dv, dv, g) - gram_v).max() / np.abs(gv).max()
    print(f"{name} level {level}: pair(v, v) against cell_moments(v) {e:.2e}")
    assert e <= TOL
    # polarisation through the existing kernel alone: no new code on this route
    ds = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v + w))
    pol = 0.5 * (hmg.cell_moments(ds, g)[1] - gram_v - hmg.cell_moments(dw, g)[1])
    e = np.abs(S - pol).max() / sc
    print(f"{name} level {level}: pair(v, w) against (G_(v+w) - G_v - G_w) / 2 {e:.2e}")
    assert e <= TOL
    # the same bits in a second call
    np.testing.assert_array_equal(hmg.cell_pair_moments(dv, dw, g), S)
    for d in (dv, dw, ds):
        d.close()


@pytest.mark.parametrize("name,level", CASES)
def test_linear_fields_on_the_device(oracle, shapes, name, level):
    O = oracle
    base, implicit, g = shapes(name, level)[:3]
    gvec, hvec = np.array([0.7, -1.3, 0.45])[:base.dim], np.array([-0.4, 0.8, 1.1])[:base.dim]
    dv = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(O, implicit, level, gvec))
    dw = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(O, implicit, level, hvec))
    vol = F.cell_volumes(O, base)
    want = vol[:, None, None] * P.sym(np.outer(gvec, hvec))[None]
    sc = P.scale(vol[:, None, None] * np.outer(gvec, gvec)[None], vol[:, None, None] * np.outer(hvec, hvec)[None])
    e = np.abs(hmg.cell_pair_moments(dv, dw, g) - want).max() / sc
    print(f"{name} level {level}: S = |c| sym(g h^T) {e:.2e}")
    assert e <= TOL
    dv.close()
    dw.close()


@pytest.mark.parametrize("name,level", [c for c in CASES if c[0] in ("cube", "square")])
def test_energy_identity_with_a_tensor_operator(oracle, shapes, name, level):
    """sigma_c : S_vw(c) = w_c . (K_c v_c): the library's own apply (lambda = 0, no constraint), both downloaded.  Scale: the
    Cauchy-Schwarz bound of the bilinear form, sqrt(max sigma : G_v  max sigma : G_w)."""
    base, implicit, g, v, w, gv, gw = shapes(name, level)[:7]
    sig = T.random_spd(np.random.default_rng(7), base.nelements(), base.dim)
    A = hmg.L2PlusDivAGrad(g, 0.0, sig)
    A._bind()
    dv, dw = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(g, level).from_host(w)
    out = hmg.DeviceMatrix(g, level)
    hmg.apply_ex(1.0, g, dv, None, out, constrain=False)
    want = np.einsum("ie,ie->e", w, out.to_host())
    got = fields.pair_energy(sig, hmg.cell_pair_moments(dv, dw, g))
    sc = np.sqrt(np.einsum("ekl,ekl->e", sig, gv).max() * np.einsum("ekl,ekl->e", sig, gw).max())
    err = np.abs(got - want).max() / sc
    print(f"{name} level {level}: sigma:S vs w.(A v) {err:.2e}")
    assert err <= TOL
    for d in (dv, dw, out):
        d.close()


def test_shrink_gives_the_prefix_bit_for_bit(oracle, ctx):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 4, origin=(-2.0, -2.0, -2.0)))
    level = 3
    implicit = O.ImplicitFineGrid.create(m, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), level)
    hmg.L2PlusDivAGrad(g, 0.0, np.ones((m.nelements(), 3)))            # (a shrink re-forms the operator's tables)
    dv = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(9)))
    dw = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(10)))
    xv, xw = np.array([0.3, 0.2, -0.7]), np.array([-0.5, 0.1, 0.4])
    S = hmg.cell_pair_moments(dv, dw, g, xv, xw)
    ne, nn = O.find_elements_in_radius(m, 1.0), O.find_nodes_in_radius(m, 1.0)
    assert 0 < ne < m.nelements()
    g.shrink(ne, nn)
    S2 = hmg.cell_pair_moments(dv, dw, g, xv, xw)
    assert S2.shape == (ne, 3, 3)
    np.testing.assert_array_equal(S2, S[:ne])                          # the moments do not see the boundary
    dv.close()
    dw.close()
    g.close()


def level2_call_succeeds(O, base, g):
    dim = base.dim
    implicit = O.ImplicitFineGrid.create(base, 2)
    gvec, hvec = np.ones(dim), np.arange(1.0, dim + 1.0)
    d1 = hmg.DeviceMatrix(g, 2).from_host(F.linear_interpolant(O, implicit, 2, gvec))
    d2 = hmg.DeviceMatrix(g, 2).from_host(F.linear_interpolant(O, implicit, 2, hvec))
    S = hmg.cell_pair_moments(d1, d2, g)
    want = F.cell_volumes(O, base)[:, None, None] * P.sym(np.outer(gvec, hvec))[None]
    assert np.abs(S - want).max() <= TOL * np.abs(want).max()
    d1.close()
    d2.close()


@pytest.mark.parametrize("dim,level", [(3, 7), (2, 9)])
def test_large_cells_are_refused_and_the_context_goes_on(oracle, ctx, dim, level):
    O = oracle
    base = O.hypercube(dim, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    dv, dw = hmg.DeviceMatrix(g, level), hmg.DeviceMatrix(g, level)
    with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS"):
        hmg.cell_pair_moments(dv, dw, g)
    level2_call_succeeds(O, base, g)
    for o in (dv, dw, g):
        o.close()


def test_mismatched_vectors_are_refused_and_the_context_goes_on(oracle, ctx):
    O = oracle
    base = O.hypercube(2, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 3)
    g2 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 3)
    d2, d3, other = hmg.DeviceMatrix(g, 2), hmg.DeviceMatrix(g, 3), hmg.DeviceMatrix(g2, 3)
    for a, b in ((d2, d3), (d3, d2)):
        with pytest.raises(hmg._lib.HmgError, match="different levels"):
            hmg.cell_pair_moments(a, b, g)
    for a, b in ((d3, other), (other, d3)):
        with pytest.raises(hmg._lib.HmgError, match="another grid"):
            hmg.cell_pair_moments(a, b, g)
    with pytest.raises(ValueError):
        hmg.cell_pair_moments(d3, d3, g, np.ones(3))
    level2_call_succeeds(O, base, g)
    for o in (d2, d3, other, g2, g):
        o.close()


def test_no_allocation_appears_inside_a_vcycle(ctx, oracle):
    """hmg_cell_pair_moments may allocate; a V-cycle after it still makes none"""
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, 2, 3, seed=0)
    bl = hmg.BaseLevel(g)
    states = [hmg.LevelState(g, i + 1) for i in range(3)]
    states[-1].b.rand(3)
    hmg.vcycle(g, bl, [op] * 3, states, 3, 3)
    hmg.cell_pair_moments(states[-1].x, states[-1].r, g)
    ctx.sync()
    assert ctx.counter("cell_pair_moments_kernel_ns") > 0 and ctx.counter("cell_pair_moments_download_ns") > 0
    n0 = ctx.counter("device_allocs")
    hmg.vcycle(g, bl, [op] * 3, states, 3, 3)
    ctx.sync()
    assert ctx.counter("device_allocs") == n0
    for st in states:
        st.close()
    g.close()


# ---- the Dirichlet tensor driver ----

DRIVER_CASES = {"2d": (3, hmg.Tri64, 3, np.array([0.6, 0.8])), "3d": (2, hmg.Tet64, 2, np.array([0.6, 0.0, 0.8]))}
_runs = {}


@pytest.fixture(scope="module")
def tensor_run(ctx):
    """the tensor driver's result per case, with fields: computed once, read only"""
    def get(key):
        if key not in _runs:
            n, eltype, refinements, _ = DRIVER_CASES[key]
            _runs[key] = driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, seed=2, tolerance=1e-10, fields=True)
        return _runs[key]
    yield get
    _runs.clear()


@pytest.mark.parametrize("key", ["2d", "3d"])
def test_tensor_driver_against_the_single_direction_driver(ctx, tensor_run, key):
    n, eltype, refinements, xi = DRIVER_CASES[key]
    r = tensor_run(key)
    dim = xi.size
    Sg = r["tensor"]
    print(f"{key}: tensor\n{Sg}\nflux\n{r['tensor_flux']}\ncycles {r['cycles']} residual {r['residual']}")
    assert Sg.shape == (dim, dim) and r["tensor_flux"].shape == (dim, dim)
    assert len(r["cycles"]) == dim and len(r["residual"]) == dim and max(r["residual"]) <= 1e-10
    assert r["pairs"].shape == (dim, dim, r["volumes"].size, dim, dim) and r["means"].shape == (dim, r["volumes"].size, dim)
    np.testing.assert_array_equal(Sg, Sg.T)
    for k in range(dim):
        e = driver.dirichlet_homogenization(n, eltype, refinements, np.eye(dim)[k], ctx=ctx, seed=2, tolerance=1e-10)["energy_form"]
        err = abs(Sg[k, k] - e) / abs(e)
        print(f"{key}: tensor[{k}, {k}] {Sg[k, k]:.15g} energy_form(e_{k}) {e:.15g} ({err:.2e})")
        assert err <= 1e-8
    e = driver.dirichlet_homogenization(n, eltype, refinements, xi, ctx=ctx, seed=2, tolerance=1e-10)["energy_form"]
    err = abs(xi @ Sg @ xi - e) / abs(e)
    print(f"{key}: xi.tensor.xi {xi @ Sg @ xi:.15g} energy_form(xi) {e:.15g} ({err:.2e})")
    assert err <= 1e-8
    err = np.abs(r["tensor_flux"] - Sg).max() / np.abs(Sg).max()
    print(f"{key}: flux form against energy form {err:.2e}")
    assert err <= 1e-8


def test_tensor_driver_uniform_medium(ctx):
    r = driver.dirichlet_homogenization_tensor(3, hmg.Tri64, 2, ctx=ctx, sigma_grid=np.full((3, 3, 2), 3.0))
    print("uniform medium:", r["tensor"], r["tensor_flux"], r["cycles"])
    assert all(c in (0, 1) for c in r["cycles"])
    # (off the diagonal the entries are compared with 0: the absolute bound is the relative one at the tensor's scale, 3)
    np.testing.assert_allclose(r["tensor"], 3.0 * np.eye(2), rtol=1e-12, atol=3e-12)
    np.testing.assert_allclose(r["tensor_flux"], 3.0 * np.eye(2), rtol=1e-12, atol=3e-12)


def test_tensor_driver_accelerated_agrees(ctx, tensor_run):
    n, eltype, refinements, _ = DRIVER_CASES["2d"]
    a = tensor_run("2d")
    b = driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, seed=2, tolerance=1e-10, accelerate=True,
                                               smoother="jacobi")
    err = np.abs(a["tensor"] - b["tensor"]).max() / np.abs(a["tensor"]).max()
    print("V-cycles", a["cycles"], "FCG + jacobi", b["cycles"], f"{err:.2e}")
    assert err <= 1e-8
    np.testing.assert_array_equal(b["tensor"], b["tensor"].T)


def test_tensor_driver_saves_the_cell_fields_of_every_pair(ctx, tmp_path):
    from homogenization_jl_amd import vtk
    path = str(tmp_path / "pairs")
    r = driver.dirichlet_homogenization_tensor(3, hmg.Tri64, 1, ctx=ctx, seed=2, save=path, fields=True)
    back = vtk.read_vtu(path + ".vtu")["cell_data"]
    for k, l in ((0, 0), (0, 1), (1, 1)):
        np.testing.assert_array_equal(back[f"pair_{k + 1}{l + 1}"], r["pairs"][k, l][:, [0, 0, 1], [0, 1, 1]])
        np.testing.assert_array_equal(back[f"energy_{k + 1}{l + 1}"], fields.pair_energy(r["cond"], r["pairs"][k, l]))


def fd_check(ctx, key, r, cond, entry, cell, move, analytic):
    """central difference of tensor[entry] |Omega| under `move` (a function that shifts a copy of cond by s) against `analytic`;
    eps and the bound are those of tests/test_gpu_cell_moments.py: the first-order error terms vanish here too, because both
    correctors are stationary.  Normalised by the largest entry of pairs[:, :, cell]."""
    n, eltype, refinements, _ = DRIVER_CASES[key]
    eps, vals = 1e-4, []
    for s in (+1.0, -1.0):
        q = driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, cond=move(cond.copy(), s * eps), tolerance=1e-10)
        vals.append(q["tensor"][entry] * q["volume"])
    fd = (vals[0] - vals[1]) / (2 * eps)
    err = abs(fd - analytic) / np.abs(r["pairs"][:, :, cell]).max()
    print(f"{key}: entry {entry} cell {cell}: central difference {fd:.12g}, analytic {analytic:.12g} ({err:.2e})")
    assert err <= 1e-6


def test_sensitivity_2d_diagonal_cond(ctx, tensor_run):
    r, cell = tensor_run("2d"), 7
    sens = fields.tensor_sensitivity(r["pairs"], diagonal=True)

    def move(cond, s):
        cond[cell, 0] += s
        return cond
    fd_check(ctx, "2d", r, r["cond"], (0, 1), cell, move, sens[0, 1, cell, 0])


def test_sensitivity_2d_full_tensor_cond(ctx):
    n, eltype, refinements, _ = DRIVER_CASES["2d"]
    r = driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, sigma_grid=driver.generate_polycrystal(2, n, 2),
                                               tolerance=1e-10, fields=True)
    assert r["cond"].shape[1:] == (2, 2)
    np.testing.assert_array_equal(r["tensor"], r["tensor"].T)
    cell = 7

    def move(cond, s):                       # the symmetric off-diagonal pair moves together: 2 S_01
        cond[cell, 0, 1] += s
        cond[cell, 1, 0] += s
        return cond
    fd_check(ctx, "2d", r, r["cond"], (0, 1), cell, move, 2.0 * fields.tensor_sensitivity(r["pairs"])[0, 1, cell, 0, 1])


def test_sensitivity_3d_diagonal_cond(ctx, tensor_run):
    r, cell = tensor_run("3d"), 20
    sens = fields.tensor_sensitivity(r["pairs"], diagonal=True)

    def move(cond, s):
        cond[cell, 0] += s
        return cond
    fd_check(ctx, "3d", r, r["cond"], (0, 2), cell, move, sens[0, 2, cell, 0])
