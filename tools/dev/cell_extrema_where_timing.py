#!/usr/bin/env python3
"""What the locations cost: hmg_cell_extrema_where (the located instantiations of the per-cell extrema kernels: two codes ride
next to the running extrema, the folds carry pairs) against hmg_cell_extrema, the yardstick -- a kernel the located call does not
touch --, on the same vector in one process:
  1. 3D level 6, widths 16 and 8 (24 576 and 3 072 cells): k_cell_extrema_where<3, 512> against k_cell_extrema<3, 512>;
  2. 3D level 7, width 16, through the window (option "cell_extrema_windows" = 1): k_extrema_where_slab against k_cell_extrema_slab;
  3. 2D level 10 on 32 cells: k_extrema_where_rows against k_cell_extrema_rows (one cell's walk, not a bandwidth);
each with 0, 4 and 8 thresholds.
  python tools/dev/cell_extrema_where_timing.py [--width 16 8] [--width7 16] [--width2d 4] [--reps 11]
                                                 [--out profiles/cell_extrema_where.txt]
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_extrema_kernel_ns",
"cell_extrema_where_kernel_ns"), after a warm-up call of each shape; medians, and the spread (min .. max), of `reps` synchronised
calls that alternate the two.  The two calls' maxima, minima and counts are compared bit for bit on the way.  No time is a
threshold of anything: the file records what was measured."""
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
ap.add_argument("--width", type=int, nargs="*", default=[16, 8])
ap.add_argument("--width7", type=int, default=16, help="0: leave the level-7 part out")
ap.add_argument("--width2d", type=int, default=4, help="0: leave the 2D part out")
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_extrema_where.txt"))
a = ap.parse_args()

THR = {0: None, 4: [1.0, 10.0, 100.0, 1000.0], 8: [1.0, 10.0, 100.0, 1000.0, 2.0, 20.0, 200.0, 2000.0]}
ctx = hmg.Context(0)
lines = ["hmg_cell_extrema_where against hmg_cell_extrema (the yardstick: its kernels are not touched), one MI355X; medians "
         f"(min .. max) of {a.reps} calls after a warm-up, alternating the two calls; kernel times from device events"]


def part(what, tag, width, level, option, old_name, new_name, note=None):
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, width, level, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, level).rand(1)
    hmg.broadcast_interfaces(x, g, level)
    form = fields.energy_form(cond)
    xi = np.array([0.6, 0.0, 0.8]) if tag is hmg.Tet64 else np.array([0.6, 0.8])
    ndof = g.nf(level) * g.ncells()
    lines.append(f"{what} = {g.ncells()} cells, level {level} ({g.nf(level)} nodes and {hmg.fine_elements(g, level)} fine elements per "
                 f"cell, {ndof} DOFs, {8 * ndof / 1e9:.3f} GB per vector)")
    ctx.set_option("cell_extrema_windows", option)
    try:
        for n, thr in THR.items():                                    # warm-up: code objects, pool blocks, the element mask
            old = hmg.cell_extrema(x, g, xi, form, thr)
            new = hmg.cell_extrema_where(x, g, xi, form, thr)
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(old, new[:3])), "the two calls' results differ"
        t_old, t_new = {n: [] for n in THR}, {n: [] for n in THR}
        for _ in range(a.reps):
            for n, thr in THR.items():
                hmg.cell_extrema(x, g, xi, form, thr)
                t_old[n].append(ctx.counter("cell_extrema_kernel_ns") * 1e-6)
                hmg.cell_extrema_where(x, g, xi, form, thr)
                t_new[n].append(ctx.counter("cell_extrema_where_kernel_ns") * 1e-6)
    finally:
        ctx.set_option("cell_extrema_windows", 0)
    for n in THR:
        o, w = statistics.median(t_old[n]), statistics.median(t_new[n])
        lines.append(f"  {old_name + ', ' + str(n) + ' thresholds':<44}{o:9.3f} ms ({min(t_old[n]):.3f} .. {max(t_old[n]):.3f})   "
                     f"{8 * ndof / (o * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF")
        lines.append(f"  {new_name + ', ' + str(n) + ' thresholds':<44}{w:9.3f} ms ({min(t_new[n]):.3f} .. {max(t_new[n]):.3f})   "
                     f"{8 * ndof / (w * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF   where / extrema {w / o:6.3f}")
    if note:
        lines.append("  " + note)
    x.close()
    g.close()


try:
    for k, width in enumerate(a.width):
        part(f"1{'abcdef'[k]}. {width}^3 cubes x 6 tetrahedra", hmg.Tet64, width, 6, 0, "k_cell_extrema<3, 512>", "k_cell_extrema_where<3, 512>")
    if a.width7:
        part(f"2. {a.width7}^3 cubes x 6 tetrahedra", hmg.Tet64, a.width7, 7, 1, "k_cell_extrema_slab", "k_extrema_where_slab")
    if a.width2d:
        part(f"3. {a.width2d}^2 squares x 2 triangles", hmg.Tri64, a.width2d, 10, 1, "k_cell_extrema_rows", "k_extrema_where_rows",
             "(32 workgroups on 256 CUs: the time of one cell's walk, not a bandwidth)")
except Exception as err:                                  # the file says what could not be produced
    lines.append(f"NOT PRODUCED from here on: {type(err).__name__}: {err}")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
