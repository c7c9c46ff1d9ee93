#!/usr/bin/env python3
"""Price of the Jacobi-preconditioned CG smoother (hmg_grid_set_smoother) on the driver's checkerboard (default: BASELINE config 3,
32^3 cubes, six levels).  One process, one set of level vectors:

  --mode vcycle   `--rounds` rounds of: smoother "cg", one untimed V-cycle, a burst of `--burst` timed ones; then the same with
                  "jacobi" (every switch re-forms the inverse diagonals, outside the timed part).  Wall clock around a synchronise.
                  Prints the medians and their ratio -- the byte count puts it near 1.5.
  --mode smooth   `--burst` hmg_smooth calls of `--steps` steps on the finest level with each smoother, for a kernel trace:
                      rocprofv3 --kernel-trace --stats -d DIR -- python tools/dev/pcg_smoother_timing.py --mode smooth
                  gives the time per launch of k_pcg_start (24 B/DOF), k_pcg_rupdate (32), k_pcg_xp (48), k_operator_diag and
                  k_dinv_finish (8 and 16) next to k_cg_rupdate_faces (24 + faces) of the "cg" calls; the DOFs per launch are printed.
  --mode cg       V-cycles with the default smoother only (A/B of two builds: HMG_LIB_PATH=<other build> HMG_LIB_AB=1).
  python tools/dev/pcg_smoother_timing.py [--width 32] [--levels 6] [--contrast 9] [--steps 3]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("vcycle", "smooth", "cg"), default="vcycle")
ap.add_argument("--width", type=int, default=32)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--contrast", type=float, default=9.0)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=3)
a = ap.parse_args()

ctx = hmg.Context(0)
L = a.levels
base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, a.width, L, seed=0, values=(1.0, a.contrast))
st = [hmg.LevelState(g, i + 1) for i in range(L)]
st[-1].x.rand(1234)
hmg.broadcast_interfaces(st[-1].x, g, L)
hmg.apply_constraint(st[-1].x, L, g)
hmg.rhs_axi_grad_v(st[-1].b, g, driver.random_unit_vec(3))
bl = hmg.BaseLevel(g)
ops = [op] * L
dofs = g.ld(L) * g.ncells()
out = {"mode": a.mode, "cells": g.ncells(), "levels": L, "top_level_doubles": dofs, "vector_GB": 8e-9 * dofs, "steps": a.steps,
       "contrast": a.contrast, "lib": os.environ.get("HMG_LIB_PATH", "this build")}


def burst(fn, count):
    fn()                                                   # (first call after a switch not timed)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / count * 1e3


vc = lambda: hmg.vcycle(g, bl, ops, st, L, a.steps)
if a.mode == "cg":
    vc()
    out["ms_per_vcycle"] = [burst(vc, a.burst) for _ in range(a.rounds)]
    out["median_ms"] = float(np.median(out["ms_per_vcycle"]))
elif a.mode == "vcycle":
    t = {"cg": [], "jacobi": []}
    for r in range(a.rounds):
        for kind in (("cg", "jacobi") if r % 2 == 0 else ("jacobi", "cg")):
            g.set_smoother(kind)
            t[kind].append(burst(vc, a.burst))
    out.update(ms_per_vcycle_cg=t["cg"], ms_per_vcycle_jacobi=t["jacobi"], median_ms_cg=float(np.median(t["cg"])),
               median_ms_jacobi=float(np.median(t["jacobi"])), ratio=float(np.median(t["jacobi"]) / np.median(t["cg"])),
               smoother_diag_bytes=ctx.counter("smoother_diag_bytes"))
else:
    sm = lambda: hmg.smoothing_steps(a.steps, g, op, st[-1], L)
    for kind in ("cg", "jacobi"):
        g.set_smoother(kind)
        out[f"ms_per_smooth_{kind}"] = burst(sm, a.burst)
    # inside hmg_vcycle the "cg" smoother takes its r-update with the face sums (k_cg_rupdate_faces); two cycles for the trace
    g.set_smoother("cg")
    out["ms_per_vcycle_cg"] = burst(vc, 2)
print(json.dumps(out))
