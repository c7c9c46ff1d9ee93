#!/usr/bin/env python3
"""Timing of the per-cell moments of cells larger than the LDS (context option "cell_moments_windows", csrc/hmg_fields_window.hip)
next to the LDS-resident kernels, which are the yardstick: kernel time per DOF, one process.
  python tools/dev/cell_moments_window_timing.py [--reps 5] [--out profiles/cell_moments_window_timing.txt]
Rows:
  3D level 7, 16^3 cubes x 6 (window kernel) against 3D level 6, 32^3 cubes x 6 (LDS kernel), about the same DOF count;
  3D level 6, 32^3 cubes x 6: option value 2 (window kernel) against value 0 (LDS kernel) on the same vectors;
  2D level 10, n = 4 (window kernel) against 2D level 8, n = 16 (LDS kernel), about the same DOF count.
Each in the single-vector form, the pair form on two vectors and the pair form on one vector given twice.  The kernels' times come
from device events inside the calls (hmg_ctx_counter "cell_moments_kernel_ns", "cell_pair_moments_kernel_ns"), after a warm-up call
of each; best of `reps` synchronised calls.  The pass is bound by FP64 work per node, not by HBM: the window form adds the plane /
row move, the list words and one barrier pair per slab / band, and in 3D has half the resident workgroups -- a ratio up to about
1.5 is the expectation; the file records what was measured."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--small", action="store_true", help="an eighth of the cells (a quick look, not the recorded shapes)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_moments_window_timing.txt"))
a = ap.parse_args()

ctx = hmg.Context(0)
OPT = "cell_moments_windows"


def measure(eltype, width, level, value):
    """ns per DOF of the three forms with the option at `value`, and the window launches they took"""
    base, cond, g, op = driver.checkerboard_problem(ctx, eltype, width, level, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, level).rand(1)
    y = hmg.DeviceMatrix(g, level).rand(2)
    for d in (x, y):
        hmg.broadcast_interfaces(d, g, level)
    ndof = g.nf(level) * g.ncells()
    ctx.set_option(OPT, value)
    try:
        n0 = ctx.counter("cell_moments_window_launches")
        hmg.cell_moments(x, g)                                    # warm-up: code objects, pool block
        hmg.cell_pair_moments(x, y, g)
        single, pair, same = [], [], []
        for _ in range(a.reps):
            hmg.cell_moments(x, g)
            single.append(ctx.counter("cell_moments_kernel_ns"))
            hmg.cell_pair_moments(x, y, g)
            pair.append(ctx.counter("cell_pair_moments_kernel_ns"))
            hmg.cell_pair_moments(x, x, g)
            same.append(ctx.counter("cell_pair_moments_kernel_ns"))
        launches = ctx.counter("cell_moments_window_launches") - n0
    finally:
        ctx.set_option(OPT, 0)
    out = {"cells": g.ncells(), "nf": g.nf(level), "ndof": ndof, "launches": launches,
           "single": min(single), "pair": min(pair), "same": min(same)}
    for d in (x, y, g):
        d.close()
    return out


def row(tag, r):
    kind = "window" if r["launches"] else "LDS   "
    return (f"  {tag:<34} {kind}  {r['cells']:>7} cells x {r['nf']:>6} nodes = {r['ndof']:>11} DOFs   single {r['single'] * 1e-6:8.3f} ms "
            f"({r['single'] / r['ndof']:.4f} ns/DOF)   pair {r['pair'] * 1e-6:8.3f} ms ({r['pair'] / r['ndof']:.4f})   "
            f"pair (v, v) {r['same'] * 1e-6:8.3f} ms ({r['same'] / r['ndof']:.4f})")


def ratio(tag, num, den):
    return (f"  {tag:<34} per-DOF ratio window / LDS: single {num['single'] / num['ndof'] / (den['single'] / den['ndof']):.2f}   "
            f"pair {num['pair'] / num['ndof'] / (den['pair'] / den['ndof']):.2f}   pair (v, v) "
            f"{num['same'] / num['ndof'] / (den['same'] / den['ndof']):.2f}")


k = 2 if a.small else 1
l7 = measure(hmg.Tet64, 16 // k, 7, 1)
l6 = measure(hmg.Tet64, 32 // k, 6, 0)
l6w = measure(hmg.Tet64, 32 // k, 6, 2)
d10 = measure(hmg.Tri64, 4 // k, 10, 1)
d8 = measure(hmg.Tri64, 16 // k, 8, 0)
lines = [f"kernel time of the per-cell moments, best of {a.reps} calls after a warm-up, device events; one process, one device",
         row("3D level 7, option 1", l7), row("3D level 6, option 0", l6), ratio("3D level 7 against level 6", l7, l6),
         row("3D level 6, option 2", l6w), ratio("3D level 6, same vectors", l6w, l6),
         row("2D level 10, option 1", d10), row("2D level 8, option 0", d8), ratio("2D level 10 against level 8", d10, d8)]
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
