#!/usr/bin/env python3
"""Price of one flexible-CG iteration against one V-cycle on the driver's problem (default: BASELINE config 3, n = 2, five
refinements): `--blocks` alternating blocks of `--per-block` hmg_fcg_step / hmg_vcycle calls after `--warmup` of each, wall clock
around a synchronise.  Prints one JSON line.  Per-kernel times of the four streaming kernels come from a kernel trace of the
same program:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/fcg_bench.py --blocks 1 --per-block 5
  python tools/fcg_bench.py [--n 2] [--dim 3] [--refinements 5] [--steps 3]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2)
ap.add_argument("--dim", type=int, default=3)
ap.add_argument("--refinements", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--blocks", type=int, default=2)
ap.add_argument("--per-block", type=int, default=10)
a = ap.parse_args()

tag = hmg.Tet64 if a.dim == 3 else hmg.Tri64
radius = driver.compute_box_radius(0, a.n) + driver.compute_boundary_layer(1.0, a.n)
L = a.refinements + 1
ctx = hmg.Context(0)
base, cond, g, op = driver.checkerboard_problem(ctx, tag, 2 * radius, L, seed=5, lam=1.0)
sts = [hmg.LevelState(g, i + 1) for i in range(L)]
x = hmg.DeviceMatrix(g, L)
x.rand(8)
hmg.broadcast_interfaces(x, g, L)
hmg.apply_constraint(x, L, g)
hmg.rhs_axi_grad_v(sts[-1].b, g, driver.random_unit_vec(a.dim))
bl = hmg.BaseLevel(g)
ops = [op] * L
f = hmg.FlexibleCG(g, bl, ops, sts, L, a.steps)
f.start(x, sts[-1].b)
sts[-1].x.copyto(x)


def timed(fn, count):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / count * 1e3


vc = lambda: hmg.vcycle(g, bl, ops, sts, L, a.steps)
timed(f.step, a.warmup)
timed(vc, a.warmup)
ms_step, ms_vc = [], []
for _ in range(a.blocks):
    ms_step.append(timed(f.step, a.per_block))
    ms_vc.append(timed(vc, a.per_block))
dofs = g.ld(L) * g.ncells()
print(json.dumps({"config": f"n={a.n} dim={a.dim} refinements={a.refinements} steps={a.steps}", "cells": g.ncells(),
                  "top_level_doubles": dofs, "vector_GB": 8e-9 * dofs, "fcg_bytes": ctx.counter("fcg_bytes"),
                  "ms_per_fcg_step": ms_step, "ms_per_vcycle": ms_vc,
                  "ratio_step_to_vcycle": min(ms_step) / min(ms_vc), "residual_norm": f.residual_norm()}))
