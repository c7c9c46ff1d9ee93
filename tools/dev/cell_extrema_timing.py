#!/usr/bin/env python3
"""Timing of the per-cell extrema over the fine elements (hmg_cell_extrema, k_cell_extrema: 8 B/DOF, 8 LDS reads and 6 quadratic
forms per node) next to k_cell_pair_moments in its one-vector form (hmg_cell_moments: 8 B/DOF, 15 LDS reads, 90 + 6 fused
operations per node), which is the yardstick: the same grid, the same vector, one process.
  python tools/dev/cell_extrema_timing.py [--width 16 8] [--levels 6] [--reps 7] [--out profiles/cell_extrema.txt]
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_moments_kernel_ns",
"cell_extrema_kernel_ns"), after a warm-up call of each; medians of `reps` synchronised calls that alternate the two.  The
expectation from the counts of LDS reads and of arithmetic is about the same time per cell; the file records what was measured."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver, fields     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, nargs="+", default=[16, 8])
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_extrema.txt"))
a = ap.parse_args()

ctx = hmg.Context(0)
L = a.levels
lines = []
for width in a.width:
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, width, L, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, L).rand(1)
    hmg.broadcast_interfaces(x, g, L)
    ndof = g.nf(L) * g.ncells()
    form = fields.energy_form(cond)
    xi = np.array([0.6, 0.0, 0.8])
    thr4 = [1.0, 10.0, 100.0, 1000.0]
    thr8 = thr4 + [2.0, 20.0, 200.0, 2000.0]
    hmg.cell_moments(x, g, xi)                                    # warm-up: code objects, pool blocks, the element mask
    for thr in (None, thr4, thr8):
        hmg.cell_extrema(x, g, xi, form, thr)
    single, ext = [], {0: [], 4: [], 8: []}
    for _ in range(a.reps):
        hmg.cell_moments(x, g, xi)
        single.append(ctx.counter("cell_moments_kernel_ns") * 1e-6)
        for n, thr in ((0, None), (4, thr4), (8, thr8)):
            hmg.cell_extrema(x, g, xi, form, thr)
            ext[n].append(ctx.counter("cell_extrema_kernel_ns") * 1e-6)
    s = statistics.median(single)
    e = {n: statistics.median(t) for n, t in ext.items()}
    lines += [
        f"{width}^3 cubes x 6 tetrahedra = {g.ncells()} cells, level {L} ({g.nf(L)} nodes and {hmg.fine_elements(g, L)} fine elements "
        f"per cell, {ndof} DOFs, {8 * ndof / 1e9:.3f} GB per vector); medians of {a.reps} calls after a warm-up, device events",
        f"  k_cell_pair_moments (v, v)      {s:9.3f} ms   {8 * ndof / (s * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF   (hmg_cell_moments: the yardstick)",
    ]
    for n in (0, 4, 8):
        lines.append(f"  k_cell_extrema, {n} thresholds    {e[n]:9.3f} ms   {8 * ndof / (e[n] * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF   "
                     f"extrema / moments {e[n] / s:6.3f}")
    lines.append("  (expectation from the counts of LDS reads, 8 against 15 per node, and of arithmetic: about 1)")
    x.close()
    g.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
