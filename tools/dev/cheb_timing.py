#!/usr/bin/env python3
"""Price of the Chebyshev-Jacobi smoother (hmg_grid_set_smoother_chebyshev) next to the other two on the driver's checkerboard
(default: BASELINE config 3, 32^3 cubes, six levels).  One process, one set of level vectors:

  --mode vcycle   `--rounds` rounds over "cg", "jacobi", "chebyshev" in rotating order: set the smoother, one untimed V-cycle (it
                  forms the inverse diagonals and the bounds), a burst of `--burst` timed ones.  Wall clock around a synchronise.
                  Prints every burst, the medians and their ratios to "cg".
  --mode smooth   `--burst` hmg_smooth calls of `--steps` steps on the finest level with "jacobi" and "chebyshev" on the same
                  vectors, for a kernel trace:
                      rocprofv3 --kernel-trace --stats -d DIR -- python tools/dev/cheb_timing.py --mode smooth
                  gives the time per launch of k_cheb_step (64 B/DOF), k_cheb_start (24), k_cheb_tail (24 / 48) next to k_pcg_xp
                  (48), k_pcg_rupdate (32), k_pcg_start (24); the doubles per launch are printed, GB/s = B/DOF * doubles / time.
  python tools/dev/cheb_timing.py [--width 32] [--levels 6] [--contrast 9] [--steps 3]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

KINDS = ("cg", "jacobi", "chebyshev")
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("vcycle", "smooth"), default="vcycle")
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
g.set_smoother("chebyshev")                                # (reserves the inverse diagonals before the level vectors)
st = [hmg.LevelState(g, i + 1) for i in range(L)]
st[-1].x.rand(1234)
hmg.broadcast_interfaces(st[-1].x, g, L)
hmg.apply_constraint(st[-1].x, L, g)
hmg.rhs_axi_grad_v(st[-1].b, g, driver.random_unit_vec(3))
g.reserve_spare(True)                                   # (the "cg" forms take their spare direction vector as on a grid of their own)
bl = hmg.BaseLevel(g)
ops = [op] * L
dofs = g.ld(L) * g.ncells()
out = {"mode": a.mode, "cells": g.ncells(), "levels": L, "top_level_doubles": dofs, "vector_GB": 8e-9 * dofs, "steps": a.steps,
       "contrast": a.contrast}


def burst(fn, count):
    fn()                                                   # (first call after a switch not timed)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / count * 1e3


vc = lambda: hmg.vcycle(g, bl, ops, st, L, a.steps)
if a.mode == "vcycle":
    t = {k: [] for k in KINDS}
    for r in range(a.rounds):
        for i in range(3):
            kind = KINDS[(r + i) % 3]
            g.set_smoother(kind)
            t[kind].append(burst(vc, a.burst))
    med = {k: float(np.median(v)) for k, v in t.items()}
    g.set_smoother("chebyshev")
    vc()                                                   # (forms the bounds: the query below then needs no scratch vector)
    out.update(ms_per_vcycle=t, median_ms=med, ratio_to_cg={k: med[k] / med["cg"] for k in KINDS},
               bounds={lev: hmg.smoother_bounds(g, lev) for lev in range(2, L + 1)},
               smoother_diag_bytes=ctx.counter("smoother_diag_bytes"))
else:
    sm = lambda: hmg.smoothing_steps(a.steps, g, op, st[-1], L)
    for kind in ("jacobi", "chebyshev"):
        g.set_smoother(kind)
        out[f"ms_per_smooth_{kind}"] = burst(sm, a.burst)
print(json.dumps(out))
