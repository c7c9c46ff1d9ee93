#!/usr/bin/env python3
"""Timing of the per-cell gradient moments (hmg_cell_moments) at the finest level of BASELINE config 3 (32^3 cubes x 6 tetrahedra,
level 6) next to the plain operator apply y += A x (24 B/DOF) on the same vectors in the same process.
  python tools/dev/cell_moments_timing.py [--width 32] [--levels 6] [--reps 5] [--out profiles/cell_moments.txt]
The kernel's time comes from device events inside the call (hmg_ctx_counter "cell_moments_kernel_ns"), the download of the
per-cell sums from the host clock ("cell_moments_download_ns"); best of `reps` synchronised calls each."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=32)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_moments.txt"))
a = ap.parse_args()

ctx = hmg.Context(0)
L = a.levels
base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, a.width, L, seed=0, lam=0.0)
x = hmg.DeviceMatrix(g, L).rand(1)
hmg.broadcast_interfaces(x, g, L)
y = hmg.DeviceMatrix(g, L).rand(2)
ndof = g.nf(L) * g.ncells()

kern, down, wall = [], [], []
hmg.cell_moments(x, g)                                            # warm-up: code object, pool block
for _ in range(a.reps):
    ctx.sync()
    t0 = time.perf_counter()
    hmg.cell_moments(x, g)
    wall.append((time.perf_counter() - t0) * 1e3)
    kern.append(ctx.counter("cell_moments_kernel_ns") * 1e-6)
    down.append(ctx.counter("cell_moments_download_ns") * 1e-6)
apply_ms = []
hmg.mul(1.0, g, op, x, y)
for _ in range(a.reps):
    ctx.sync()
    t0 = time.perf_counter()
    hmg.mul(1.0, g, op, x, y)
    ctx.sync()
    apply_ms.append((time.perf_counter() - t0) * 1e3)

k, d, w, p = min(kern), min(down), min(wall), min(apply_ms)
lines = [
    f"per-cell gradient moments, {a.width}^3 cubes x 6 tetrahedra = {g.ncells()} cells, level {L} ({g.nf(L)} nodes per cell, {ndof} DOFs)",
    f"best of {a.reps} synchronised calls, one process, the same vectors",
    f"k_cell_pair_moments, one column       {k:9.3f} ms   {8 * ndof / (k * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF",
    f"download of {g.ncells()} x 9 sums      {d:9.3f} ms",
    f"hmg_cell_moments, whole call (host)   {w:9.3f} ms   (kernel + download + the host's transform per cell)",
    f"plain apply y += A x (host clock)     {p:9.3f} ms   {24 * ndof / (p * 1e-3) / 1e12:6.3f} TB/s on 24 B/DOF",
    f"kernel / plain apply                  {k / p:9.3f}      (bar: no slower than the plain apply, i.e. <= 1)",
]
print("\n".join(lines))
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
