#!/usr/bin/env python3
"""Per-call time and TB/s of the driver integrals on one level: hmg_integrate modes 1 (integrate_terms), 3 (mass pairing) and
4 (load pairing), each 16 B per DOF of algorithmic traffic.
  python tools/dev/pair_integral_timing.py --width 32 --levels 6 [--dim 3] [--calls 20] [--rounds 3]
A call is the pass, its two small reduction kernels and the read-back of the scalar; the host clock runs around `calls` calls,
each of which ends in a device synchronise.  One untimed call per mode first, then `rounds` rounds that alternate the modes.
With HMG_LIB_PATH / HMG_LIB_AB=1 (an older build, homogenization.jl_amd/_lib.py) the modes it lacks are reported as absent:
mode 1 of two builds is compared by running this twice in one job."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=32)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--dim", type=int, default=3)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
ctx = hmg.Context(0)
tag = hmg.Tet64 if a.dim == 3 else hmg.Tri64
base, cond, g, op = driver.checkerboard_problem(ctx, tag, a.width, a.levels, seed=3)
v, w, s = (hmg.DeviceMatrix(g, a.levels) for _ in range(3))
v.rand(1)
w.rand(2)
hmg.broadcast_interfaces(v, g, a.levels)
hmg.broadcast_interfaces(w, g, a.levels)
hmg.rhs_axi_grad_v(s, g, np.ones(a.dim))
ne = g.ncells()
dofs = float(g.nf(a.levels)) * ne
modes = {"mode 1 (v + w).Mv": lambda: hmg.integrate_terms(v, w, g, ne),
         "mode 3 w.Mv": lambda: hmg.integrate_pair_mass(v, w, g, ne),
         "mode 4 v.s": lambda: hmg.integrate_pair_load(v, s, g, ne)}
absent = []
for name, fn in list(modes.items()):
    try:
        fn()
    except hmg._lib.HmgError as e:
        absent.append(name)
        del modes[name]
ms = {name: [] for name in modes}
for _ in range(a.rounds):
    for name, fn in modes.items():
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        ms[name].append((time.perf_counter() - t0) / a.calls * 1e3)
out = {"lib": os.environ.get("HMG_LIB_PATH", "this build"), "dim": a.dim, "width": a.width, "levels": a.levels, "cells": ne,
       "dofs": dofs, "calls": a.calls, "absent": absent,
       "ms_per_call": {k: [round(x, 4) for x in t] for k, t in ms.items()},
       "best_TB_per_s": {k: round(16.0 * dofs / (min(t) * 1e-3) / 1e12, 3) for k, t in ms.items()}}
print(json.dumps(out))
