"""GPU tests of tensor fields through the partitioned drivers and the driver benchmark tool: a polycrystal `sigma_grid` (one rotated
tensor per unit cube) through dist.partitioned_checkerboard_homogenization and its tensor variant on a one-rank communicator,
against the single-GPU drivers on the same field, as tests/test_gpu_dist.py holds the diagonal field; and
tools/driver_bench.py --polycrystal end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver, dist as hdist

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim,n", [(2, 1), (3, 0)])
def test_partitioned_drivers_take_a_polycrystal(dim, n):
    tag = hmg.Tri64 if dim == 2 else hmg.Tet64
    width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
    sg = driver.generate_polycrystal(dim, width, 31)
    ctx = hmg.Context(0)
    try:
        kw = dict(refinements=2, tolerance=1e-3, sigma_grid=sg, seed=4)
        want, hist_s = driver.checkerboard_homogenization(n, tag, ctx=ctx, **kw)
        got, hist_p = hdist.partitioned_checkerboard_homogenization(ctx, n, tag, 1, 0, backend="rccl", **kw)
        assert len(hist_s) == len(hist_p) and abs(got - want) <= 1e-10 * max(1.0, abs(want)), (got, want)
        Sw, hist_s = driver.checkerboard_homogenization_tensor(n, tag, ctx=ctx, **kw)
        Sg, hist_p = hdist.partitioned_checkerboard_homogenization_tensor(ctx, n, tag, 1, 0, backend="rccl", **kw)
        assert len(hist_s) == len(hist_p) and np.abs(Sg - Sw).max() <= 1e-10 * max(1.0, np.abs(Sw).max()), (Sg, Sw)
    finally:
        ctx.close()


def test_driver_bench_polycrystal():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "driver_bench.py"), "--dim", "2", "--n", "1", "--refinements", "2",
                          "--tolerance", "1e-3", "--polycrystal", "--field-seed", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["polycrystal"] is True and res["field_seed"] == 3 and "sigma_cpu" not in res
    assert res["vcycles"] > 0 and np.isfinite(res["sigma_gpu"])
    # every tensor of the field has the eigenvalues 1 and 9: a homogenized conductivity, and its distance to the mean, lie in (0, 9)
    assert 0.0 < res["sigma_gpu"] < 9.0
