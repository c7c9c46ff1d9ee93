#!/usr/bin/env python3
"""Timing of the per-cell pair moments (hmg_cell_pair_moments, 16 B/DOF) next to the single-vector kernel (hmg_cell_moments,
8 B/DOF), which is the yardstick: the same grid, the same vectors, one process.
  python tools/dev/cell_pair_moments_timing.py [--width 8 16] [--levels 6] [--reps 5] [--out profiles/cell_pair_moments.txt]
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_moments_kernel_ns",
"cell_pair_moments_kernel_ns"), after a warm-up call of each; best of `reps` synchronised calls.  The expectation is about twice
the single-vector kernel's time (twice the bytes); the file records what was measured."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, nargs="+", default=[8])
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_pair_moments.txt"))
a = ap.parse_args()

ctx = hmg.Context(0)
L = a.levels
lines = []
for width in a.width:
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, width, L, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, L).rand(1)
    y = hmg.DeviceMatrix(g, L).rand(2)
    for d in (x, y):
        hmg.broadcast_interfaces(d, g, L)
    ndof = g.nf(L) * g.ncells()
    hmg.cell_moments(x, g)                                        # warm-up: code objects, pool block
    hmg.cell_pair_moments(x, y, g)
    single, pair, same = [], [], []
    for _ in range(a.reps):
        hmg.cell_moments(x, g)
        single.append(ctx.counter("cell_moments_kernel_ns") * 1e-6)
        hmg.cell_pair_moments(x, y, g)
        pair.append(ctx.counter("cell_pair_moments_kernel_ns") * 1e-6)
        hmg.cell_pair_moments(x, x, g)
        same.append(ctx.counter("cell_pair_moments_kernel_ns") * 1e-6)
    s, p, q = min(single), min(pair), min(same)
    lines += [
        f"{width}^3 cubes x 6 tetrahedra = {g.ncells()} cells, level {L} ({g.nf(L)} nodes per cell, {ndof} DOFs, "
        f"{8 * ndof / 1e9:.3f} GB per vector); best of {a.reps} calls after a warm-up, device events",
        f"  hmg_cell_moments (v)            {s:9.3f} ms   {8 * ndof / 1e9:7.3f} GB read   {8 * ndof / (s * 1e-3) / 1e12:6.3f} TB/s on  8 B/DOF",
        f"  k_cell_pair_moments (v, w)      {p:9.3f} ms   {16 * ndof / 1e9:7.3f} GB read   {16 * ndof / (p * 1e-3) / 1e12:6.3f} TB/s on 16 B/DOF",
        f"  k_cell_pair_moments (v, v)      {q:9.3f} ms   (one handle twice: the column is read once, as by hmg_cell_moments)",
        f"  pair / single                   {p / s:9.3f}      (expectation from the bytes: about 2)",
    ]
    x.close()
    y.close()
    g.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
