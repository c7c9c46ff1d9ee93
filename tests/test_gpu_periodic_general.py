"""
Grids on a GENERAL torus on the device: nodes off the integer lattice, a stretched box, representatives stored whole periods
away (tests/_periodic_form.py: general_torus), and a full conductivity tensor per cell.  Every apply family, the residual, the
interface sum and the unique norm are held to the statements of tests/_periodic_device.py -- the oracle's (diagonal) or
tests/_tensor_sigma_form.py's (full tensors) cell-local operator on the cells as disjoint simplices, the sum over copies from a
grouping of the fine nodes by position modulo the period -- at the project's 1e-11.  The cases are the smallest that reach each
kernel family; each asserts the launch counter of its family (tests/test_gpu_periodic.py::test_3d_levels_2_to_6).  Level 7 is
not repeated here.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

import _tensor_sigma_form as TS
from _periodic_device import Torus, check_primitives, per_cube
from _periodic_form import DEN, general_torus

pytestmark = pytest.mark.gpu

FAMILIES = ("small_launches", "wave_launches", "weight_cache_launches")


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def test_3d_diagonal_levels_3_5_6(oracle, ctx):
    """k_apply_small / _pack (3), k_apply_wave (5), k_apply with the class-weight cache (6): one class per cell here"""
    c = Torus(oracle, ctx, 3, 6, seed=1, mesh=general_torus((3, 3, 3), 1), den=DEN)
    n0 = {n: ctx.counter(n) for n in FAMILIES}
    worst = check_primitives(c, [3, 5, 6])
    print(f"worst {worst:.2e}")
    assert all(ctx.counter(n) > v for n, v in n0.items()), n0
    c.close()


def test_3d_full_tensors_levels_2_4_5_6(oracle, ctx):
    c = Torus(oracle, ctx, 3, 6, seed=2, mesh=general_torus((3, 3, 3), 2), tensor=True, den=DEN)
    assert np.abs(c.sig[:, 0, 1]).min() > 0.0 and c.g.table_i32("cell_class").size == 162
    n0 = {n: ctx.counter(n) for n in FAMILIES}
    worst = check_primitives(c, [2, 4, 5, 6])
    print(f"worst {worst:.2e}")
    assert all(ctx.counter(n) > v for n, v in n0.items()), n0
    c.close()


def test_3d_full_tensors_level_6_without_the_weight_cache(oracle, ctx):
    c = Torus(oracle, ctx, 3, 6, seed=2, classes=1, mesh=general_torus((3, 3, 3), 2), tensor=True, den=DEN)
    assert c.g.table_i32("cell_class").size == 0
    n0 = ctx.counter("weight_cache_launches")
    worst = check_primitives(c, [6])
    print(f"worst {worst:.2e}")
    assert ctx.counter("weight_cache_launches") == n0
    c.close()


def test_3d_one_tensor_per_cube_level_6_with_the_weight_cache(oracle, ctx):
    """27 tensors on the unit cubes of driver.periodic_mesh: rows repeat (27 tensors x 6 orientations at most), the classes of
    the weight cache are fewer than the cells, and the cached weights are those of full tensors"""
    mesh = driver.periodic_mesh(hmg.Tet64, 3)
    sig = per_cube(mesh, TS.random_spd(np.random.default_rng(8), 27, 3).reshape(3, 3, 3, 3, 3))
    c = Torus(oracle, ctx, 3, 6, seed=3, mesh=mesh, sig=sig, tensor=True)
    cls = c.g.table_i32("cell_class")
    assert cls.size == 162 and 27 <= np.unique(cls).size <= 162
    n0 = ctx.counter("weight_cache_launches")
    worst = check_primitives(c, [6])
    print(f"worst {worst:.2e}, {np.unique(cls).size} classes")
    assert ctx.counter("weight_cache_launches") > n0
    c.close()


@pytest.mark.parametrize("levels,counter", [(5, None), (9, "rows_launches")])
def test_2d_full_tensors_levels_5_and_9(oracle, ctx, levels, counter):
    c = Torus(oracle, ctx, 2, levels, seed=4, mesh=general_torus((4, 3), 3), tensor=True, den=DEN)
    n0 = ctx.counter(counter) if counter else 0
    worst = check_primitives(c, [levels])
    print(f"worst {worst:.2e}")
    assert counter is None or ctx.counter(counter) > n0
    c.close()


def test_3d_representatives_do_not_matter_on_the_device(oracle, ctx):
    """the same torus with every node stored up to two periods away: level 4 against the statement, and apply, residual and
    interface sum of the same vectors against the unshifted grid's, bit for bit (tests/test_periodic_host.py holds the tables)"""
    a = Torus(oracle, ctx, 3, 4, seed=5, mesh=general_torus((3, 3, 3), 4), den=DEN)
    b = Torus(oracle, ctx, 3, 4, seed=5, mesh=general_torus((3, 3, 3), 4, shift=True), den=DEN)
    assert not np.array_equal(a.mesh.nodes, b.mesh.nodes) and np.array_equal(a.sig, b.sig)
    worst = check_primitives(b, [4])
    print(f"worst {worst:.2e}")
    x, src = a.rand(4), a.rand(4)
    outs = []
    for c in (a, b):
        for lam in (0.7, 0.0):
            c.A.lam = lam
            out, dx, dsrc = hmg.DeviceMatrix(c.g, 4), c.dev(4, x), c.dev(4, src)
            c.A._bind()
            hmg.apply_ex(-1.3, c.g, dx, dsrc, out, constrain=True)
            st = hmg.LevelState(c.g, 4)
            st.x.from_host(x)
            st.b.from_host(src)
            hmg.local_residual(c.g, c.A, st, 4)
            outs.append((c is a, lam, out.to_host(), st.r.to_host()))
            hmg.broadcast_interfaces(out, c.g, 4)
            outs[-1] += (out.to_host(),)
            for v in (out, dx, dsrc):
                v.close()
            st.close()
    for (_, lam, *pa), (_, lam_b, *pb) in zip(outs[:2], outs[2:]):
        assert lam == lam_b
        for u, v in zip(pa, pb):
            assert np.abs(u).max() > 0 and np.array_equal(u.view(np.int64), v.view(np.int64))
    a.close()
    b.close()
