"""GPU tests of the Dirichlet drivers on a top level whose cell exceeds the LDS (keyword `large_cells`, context option
"cell_moments_windows", csrc/hmg_fields_window.hip).
  * driver.dirichlet_homogenization(1, Tri64, refinements=8) -- top level 9, two cells of 33 153 nodes -- and
    driver.dirichlet_homogenization_tensor at the same shape.  hypercube(1) is one unit square: the seeded field has one value, the
    medium is uniform, the corrector is zero and no cycle runs (its base mesh has no interior node either, so no level-1 system
    exists).  The case shows the keyword, the routing, the restored option and the refusal without the keyword.
  * the same two drivers at n = 2 (2D: refinements=8, 8 cells; 3D: Tet64, refinements=6, top level 7, 48 cells of 47 905 nodes)
    on the seeded 1 / 9 checkerboard: real solves, a dozen or more cycles.
  * 3D at n = 1 (Tet64, refinements=6) is NOT a driver test here: the uniform medium's loads cancel to rounding in 3D, not to
    zero, the driver returns at once as documented and reports the residual relative to that noise -- 1.0 at 0 cycles (measured),
    which no residual bound can meet.  3D level 7 is covered by tests/test_gpu_cell_moments_window.py and by the n = 2 run above.
Bounds: those of fd_check in tests/test_gpu_cell_moments.py (residual 1e-10, energy form = xi . flux form to 1e-8) and of the tensor
driver's tests in tests/test_gpu_cell_pair_moments.py (exactly symmetric, flux form to 1e-8)."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

pytestmark = pytest.mark.gpu
OPT, COUNTER = "cell_moments_windows", "cell_moments_window_launches"
# key: n, element type, refinements, top level, xi, cycles at least
CASES = {"2d-n1": (1, hmg.Tri64, 8, 9, np.array([0.6, 0.8]), 0), "2d-n2": (2, hmg.Tri64, 8, 9, np.array([0.6, 0.8]), 2),
         "3d-n2": (2, hmg.Tet64, 6, 7, np.array([0.6, 0.0, 0.8]), 2)}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("key", list(CASES))
def test_dirichlet_homogenization_on_large_cells(ctx, key):
    n, eltype, refinements, level, xi, min_cycles = CASES[key]
    assert ctx.counter(OPT) == 0
    n0 = ctx.counter(COUNTER)
    r = driver.dirichlet_homogenization(n, eltype, refinements, xi, ctx=ctx, seed=2, tolerance=1e-10, large_cells=True, fields=True)
    assert ctx.counter(OPT) == 0                                       # restored
    assert ctx.counter(COUNTER) == n0 + 1
    e, f = r["energy_form"], r["flux_form"]
    err = abs(e - np.dot(xi, f)) / abs(e)
    print(f"{key}: energy form {e:.15g} xi.flux form {np.dot(xi, f):.15g} ({err:.2e}), {r['cycles']} cycles, "
          f"residual {r['residual']:.2e}")
    assert r["cycles"] >= min_cycles and r["residual"] <= 1e-10
    assert err <= 1e-8
    assert r["mean"].shape == (r["volumes"].size, xi.size) and r["gram"].shape == (r["volumes"].size, xi.size, xi.size)


def test_without_the_keyword_the_refusal_stands(ctx):
    n, eltype, refinements, level, xi, _ = CASES["2d-n1"]
    with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS"):
        driver.dirichlet_homogenization(n, eltype, refinements, xi, ctx=ctx, seed=2, tolerance=1e-10)
    assert ctx.counter(OPT) == 0


def test_the_option_is_restored_to_the_callers_value(ctx):
    n, eltype, refinements, level, xi, _ = CASES["2d-n1"]
    ctx.set_option(OPT, 2)
    try:
        driver.dirichlet_homogenization(1, eltype, 2, xi, ctx=ctx, seed=2, large_cells=True)
        assert ctx.counter(OPT) == 2
    finally:
        ctx.set_option(OPT, 0)


@pytest.mark.parametrize("key", ["2d-n1", "2d-n2"])
def test_dirichlet_tensor_on_large_cells(ctx, key):
    n, eltype, refinements, level, xi, min_cycles = CASES[key]
    n0 = ctx.counter(COUNTER)
    r = driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, seed=2, tolerance=1e-10, large_cells=True)
    assert ctx.counter(OPT) == 0
    assert ctx.counter(COUNTER) == n0 + 3                              # two single-vector passes and one pair
    Sg = r["tensor"]
    print(f"tensor\n{Sg}\nflux\n{r['tensor_flux']}\ncycles {r['cycles']} residual {r['residual']}")
    assert min(r["cycles"]) >= min_cycles and max(r["residual"]) <= 1e-10
    np.testing.assert_array_equal(Sg, Sg.T)
    err = np.abs(r["tensor_flux"] - Sg).max() / np.abs(Sg).max()
    print(f"flux form against energy form {err:.2e}")
    assert err <= 1e-8
    with pytest.raises(hmg._lib.HmgError, match=f"level {level} .*does not fit the LDS"):
        driver.dirichlet_homogenization_tensor(n, eltype, refinements, ctx=ctx, seed=2, tolerance=1e-10)
