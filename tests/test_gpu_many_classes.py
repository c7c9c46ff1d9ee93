"""GPU tests of the class-weight cache at class counts past the old limit of 1 024: 6^3 cubes, 1 296 cells, one tensor -- and so
one coefficient row, one class -- per cell.  Context option "weight_cache_classes" (0, the default: no limit by count; 1024: the
library's behaviour before the option), counters "weight_cache_classes" / "weight_cache_bytes", and the agreement of the two
settings.  Which levels keep the cached-weight kernels above 1 024 classes is for the measurement of
profiles/tensor_many_classes.txt to decide; FAST_ABOVE_1024 below states what the launchers do and is asserted.  (That file holds
no figure yet: every level keeps its cached-weight kernel.)"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
NCELLS = 1296
# level -> the counter that advances when the level's cached-weight kernel runs at more than 1 024 classes (None: the level keeps
# the generic kernel there); level 6: the instantiations k_apply<.., WC> of the register-blocked kernel
FAST_ABOVE_1024 = {2: "small_launches", 3: "small_launches", 4: "small_launches", 5: "wave_launches", 6: "weight_cache_launches"}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def field(oracle):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 6, origin=(-3.0, -3.0, -3.0)))
    assert m.nelements() == NCELLS
    return hmg.Mesh(m.nodes, m.elements + 1), T.random_spd(np.random.default_rng(41), NCELLS, 3)


def make(ctx, field, levels, limit):
    base, sig = field
    ctx.set_option("weight_cache_classes", limit)
    try:
        g = hmg.ImplicitFineGrid(ctx, base, levels)
        A = hmg.L2PlusDivAGrad(g, 1.0, sig)                       # (the option is read where the operator is set)
    finally:
        ctx.set_option("weight_cache_classes", 0)
    return g, A


def counters(ctx):
    return {n: ctx.counter(n) for n in ("small_launches", "wave_launches", "weight_cache_launches", "weight_cache_classes",
                                        "weight_cache_bytes")}


@pytest.mark.parametrize("levels", [5, 6])
def test_a_row_per_cell_stays_on_the_cached_weight_kernels(ctx, field, levels):
    c0 = counters(ctx)
    gb, Ab = make(ctx, field, levels, 1024)                       # the library before the option: no cache above 1 024 rows
    assert gb.table_i32("cell_class").size == 0
    c1 = counters(ctx)
    assert c1["weight_cache_classes"] == c0["weight_cache_classes"] and c1["weight_cache_bytes"] == c0["weight_cache_bytes"]
    gc, Ac = make(ctx, field, levels, 0)
    cls = gc.table_i32("cell_class")
    assert cls.shape == (NCELLS,) and np.unique(cls).size == NCELLS
    c2 = counters(ctx)
    assert c2["weight_cache_classes"] - c1["weight_cache_classes"] == NCELLS
    assert c2["weight_cache_bytes"] - c1["weight_cache_bytes"] == NCELLS * 2 * 240 * 8 * (levels - 1)

    rng = np.random.default_rng(levels)
    for lev in range(2, levels + 1):
        nf = gc.nf(lev)
        x = np.asfortranarray(rng.standard_normal((nf, NCELLS)))
        y = np.asfortranarray(rng.standard_normal((nf, NCELLS)))
        got = {}
        for name, g, A in (("limit", gb, Ab), ("default", gc, Ac)):
            n0 = counters(ctx)
            dx, dy = hmg.DeviceMatrix(g, lev).from_host(x), hmg.DeviceMatrix(g, lev).from_host(y)
            hmg.mul(-1.0, g, A, dx, dy)                             # apply, alpha = -1, with a source
            st = hmg.LevelState(g, lev)
            st.x.from_host(x); st.b.from_host(y)
            hmg.local_residual(g, A, st, lev)                       # residual
            got[name] = (dy.to_host(), st.r.to_host())
            n1 = counters(ctx)
            which = FAST_ABOVE_1024.get(lev)
            for cnt in ("small_launches", "wave_launches", "weight_cache_launches"):
                advanced = n1[cnt] - n0[cnt]
                assert advanced == (2 if name == "default" and cnt == which else 0), (lev, name, cnt, advanced)
            st.close(); dx.close(); dy.close()
        slot = gc.table_i32("hier2slot", lev)
        for a, b in zip(got["default"], got["limit"]):
            if lev == 5 and FAST_ABOVE_1024.get(5):
                # as tests/test_gpu_wave.py holds the one-wave kernel to the 256-thread kernel: bit for bit, except the 45 nodes
                # of the three edges of the slanted face (one fused multiply-add contracted the other way round)
                slanted = (slot >= 49) & (slot < 94)
                np.testing.assert_array_equal(a[~slanted], b[~slanted])
                assert np.abs(a[slanted] - b[slanted]).max() <= 8 * np.finfo(float).eps * np.abs(b).max()
            else:
                assert relerr(a, b) <= 1e-13, lev                   # (tests/test_gpu_small.py: the workgroup kernel to rounding)

    # one V-cycle: 1e-12 relative; three more allocate nothing
    out = {}
    for name, g, A in (("limit", gb, Ab), ("default", gc, Ac)):
        sts = [hmg.LevelState(g, i + 1) for i in range(levels)]
        sts[-1].x.rand(5); sts[-1].b.rand(6)
        hmg.broadcast_interfaces(sts[-1].x, g, levels)
        hmg.apply_constraint(sts[-1].x, levels, g)
        bl = hmg.BaseLevel(g)
        n0 = counters(ctx)
        hmg.vcycle(g, bl, [A] * levels, sts, levels, 3)
        out[name] = (sts[-1].x.to_host(), sts[-1].r.to_host())
        n1 = counters(ctx)
        for cnt in ("small_launches", "wave_launches"):
            expected = name == "default" and cnt in [FAST_ABOVE_1024.get(l) for l in range(2, levels + 1)]
            assert (n1[cnt] > n0[cnt]) == expected, (name, cnt)
        a0 = ctx.counter("device_allocs")
        for _ in range(3):
            hmg.vcycle(g, bl, [A] * levels, sts, levels, 3)
        ctx.sync()
        assert ctx.counter("device_allocs") == a0
        for s in sts:
            s.close()
    ex, er = relerr(out["default"][0], out["limit"][0]), relerr(out["default"][1], out["limit"][1])
    print(f"{levels} levels, V-cycle: default against limit 1024: x {ex:.2e} r {er:.2e}")
    assert ex <= 1e-12 and er <= 1e-12

    # lambda changes in place; a new operator of few rows shrinks the cache; closing the grid hands it back
    Ac.lam = 0.25
    assert counters(ctx)["weight_cache_bytes"] == c2["weight_cache_bytes"]
    gc.set_operator(np.random.default_rng(1).choice([1.0, 9.0], size=(NCELLS, 3)), 1.0)
    few = np.unique(gc.table_i32("cell_class")).size
    c3 = counters(ctx)
    assert few < 200 and c3["weight_cache_classes"] - c1["weight_cache_classes"] == few
    assert c3["weight_cache_bytes"] - c1["weight_cache_bytes"] == few * 2 * 240 * 8 * (levels - 1)
    gc.close(); gb.close()
    c4 = counters(ctx)
    assert c4["weight_cache_classes"] == c0["weight_cache_classes"] and c4["weight_cache_bytes"] == c0["weight_cache_bytes"]


def test_a_shrink_keeps_the_limit_its_operator_was_set_under(ctx, field):
    """Option "weight_cache_classes" is read where the operator is set; hmg_grid_shrink classes the remaining cells under the limit
    stored then, whatever the option says by now.  1 296 rows shrink to the 384 of the inner 4^3 cubes: a grid set under limit 200
    stays without a cache after the option is back at 0, one set under no limit keeps its cache after the option becomes 200."""
    from homogenization_jl_amd import driver
    base, sig = field
    nc, nn = driver.find_elements_in_radius(base, 2.0), driver.find_nodes_in_radius(base, 2.0)
    assert nc == 384
    c0 = counters(ctx)
    ga, Aa = make(ctx, field, 3, 200)                             # (make() puts the option back to 0)
    assert ga.table_i32("cell_class").size == 0
    ga.shrink(nc, nn)
    assert ga.table_i32("cell_class").size == 0
    assert counters(ctx)["weight_cache_classes"] == c0["weight_cache_classes"]
    gb, Ab = make(ctx, field, 3, 0)
    ctx.set_option("weight_cache_classes", 200)
    try:
        gb.shrink(nc, nn)
    finally:
        ctx.set_option("weight_cache_classes", 0)
    assert np.unique(gb.table_i32("cell_class")).size == nc
    assert counters(ctx)["weight_cache_classes"] - c0["weight_cache_classes"] == nc
    ga.close(); gb.close()
    assert counters(ctx)["weight_cache_classes"] == c0["weight_cache_classes"]
