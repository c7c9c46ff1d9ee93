"""Per-level apply times and V-cycle times at one coefficient row per cell: the measurement behind profiles/tensor_many_classes.txt.
One library / field / class limit per process, one JSON line each (appended to measure_classes.jsonl in the current directory):

  python tools/dev/measure_classes.py TAG FIELD LIMIT [option=value ...]
      FIELD  polycrystal (driver.generate_polycrystal, one tensor per cube) | perturbed (two-valued diagonal field on a mesh
             with perturbed nodes: as many distinct rows, for a build without the tensor entry) | checkerboard (48 rows)
      LIMIT  context option "weight_cache_classes" (0: no limit, 1024: the library before the option), or `none`: not set
             (an older build loaded through HMG_LIB_PATH / HMG_LIB_AB=1)
      option=value  further context options, e.g. apply_small=0, apply_wave=0, weight_cache=0: one kernel family at a time

3D, width 16 (24 576 cells), 6 grids, three smoothing steps; five repeats of ten V-cycles (wall clock around a device synchronise)
after four warm-up cycles; then five V-cycles under option "time_apply" = 1 for the per-level apply times.  Alternate the
settings and run the list twice: the spread of one setting's repeats is what a difference has to beat."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

tag, field, limit = sys.argv[1], sys.argv[2], sys.argv[3]
extra = dict(kv.split("=") for kv in sys.argv[4:])
W, LEVELS, STEPS, REPEATS, PER = 16, 6, 3, 5, 10
base = driver.checkerboard_mesh(hmg.Tet64, W, origin=(-W / 2.0,) * 3, transposed_lookup=True)
if field == "polycrystal":
    cond = driver.conductivity_per_element(base, driver.generate_polycrystal(3, W, 5, (1.0, 9.0, 100.0)), (W / 2.0 + 1.0,) * 3)
else:
    cond = driver.conductivity_per_element(base, driver.generate_conductivity(3, W, 5), (W / 2.0 + 1.0,) * 3)
    if field == "perturbed":
        base = hmg.Mesh(base.nodes + 0.2 * (np.random.default_rng(1).random(base.nodes.shape) - 0.5), base.elements)
ctx = hmg.Context(0)
if limit != "none":
    ctx.set_option("weight_cache_classes", int(limit))
for k, v in extra.items():
    ctx.set_option(k, int(v))
g = hmg.ImplicitFineGrid(ctx, base, LEVELS)
A = hmg.L2PlusDivAGrad(g, 1.0, cond)
rows = np.unique(g.table_f64("coef").reshape(-1, 8).view(np.uint64), axis=0).shape[0]
sts = [hmg.LevelState(g, i + 1) for i in range(LEVELS)]
sts[-1].x.rand(5); sts[-1].b.rand(6)
hmg.broadcast_interfaces(sts[-1].x, g, LEVELS)
hmg.apply_constraint(sts[-1].x, LEVELS, g)
bl = hmg.BaseLevel(g)
ops = [A] * LEVELS
for _ in range(4):
    hmg.vcycle(g, bl, ops, sts, LEVELS, STEPS)
ctx.sync()
c0 = {n: ctx.counter(n) for n in ("wave_launches", "small_launches", "device_allocs")}
ms = []
for _ in range(REPEATS):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(PER):
        hmg.vcycle(g, bl, ops, sts, LEVELS, STEPS)
    ctx.sync()
    ms.append((time.perf_counter() - t0) * 1e3 / PER)
c1 = {n: ctx.counter(n) for n in c0}
lev = {}
for rep in range(REPEATS):
    ctx.set_option("time_apply", 1)
    hmg.vcycle(g, bl, ops, sts, LEVELS, STEPS)
    for l in range(2, LEVELS + 1):
        n, t, by = ctx.apply_timing_level(l)
        lev.setdefault(l, []).append((n, t))
ctx.set_option("time_apply", 0)
out = {"tag": tag, "field": field, "limit": limit, "extra": extra, "cells": g.ncells(), "distinct_rows": rows,
       "vcycle_ms": [round(v, 4) for v in ms], "vcycle_ms_median": round(float(np.median(ms)), 4),
       "launches_per_vcycle": {n: (c1[n] - c0[n]) / (REPEATS * PER) for n in c0},
       "apply_ms_per_vcycle_by_level": {l: {"launches": v[0][0], "ms": [round(t, 4) for _, t in v]} for l, v in lev.items()},
       "weight_cache_classes": ctx.counter("weight_cache_classes"), "weight_cache_bytes": ctx.counter("weight_cache_bytes"),
       "rnorm": hmg.norm_unique(sts[-1].r), "xnorm": hmg.norm(sts[-1].x)}
print(json.dumps(out))
with open("measure_classes.jsonl", "a") as f:
    f.write(json.dumps(out) + "\n")
