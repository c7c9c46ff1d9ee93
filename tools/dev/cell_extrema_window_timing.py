#!/usr/bin/env python3
"""Timing of the per-cell extrema of cells larger than the LDS (context option "cell_extrema_windows",
csrc/hmg_extrema_window.hip) on one GPU, three comparisons in one process:
  1. 3D level 7, 16^3 cubes x 6 tetrahedra: k_cell_extrema_slab with 0, 4 and 8 thresholds against hmg_cell_moments through ITS
     window kernel (k_cell_pair_moments_slab, one vector) on the same vector -- the same 8 B/DOF and the same walk;
  2. 3D level 6, the same width: the window kernel (option 2) against k_cell_extrema (option 0);
  3. 2D level 10 on 32 cells (4^2 squares x 2 triangles): k_cell_extrema_rows against the rows moment kernel.
  python tools/dev/cell_extrema_window_timing.py [--width 16] [--width2d 4] [--reps 7] [--out profiles/cell_extrema_window.txt]
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_moments_kernel_ns",
"cell_extrema_kernel_ns"), after a warm-up call of each; medians of `reps` synchronised calls that alternate the kernels.  No time
is a threshold of anything: the file records what was measured."""
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
ap.add_argument("--width", type=int, default=16)
ap.add_argument("--width2d", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_extrema_window.txt"))
a = ap.parse_args()

THR4 = [1.0, 10.0, 100.0, 1000.0]
THR8 = THR4 + [2.0, 20.0, 200.0, 2000.0]
ctx = hmg.Context(0)
lines = ["Per-cell extrema of cells larger than the LDS (context option \"cell_extrema_windows\", csrc/hmg_extrema_window.hip), one "
         "MI355X; medians of %d calls after a warm-up, kernel times from device events" % a.reps]


def problem(tag, width, level):
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, width, level, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, level).rand(1)
    hmg.broadcast_interfaces(x, g, level)
    return g, x, fields.energy_form(cond), np.array([0.6, 0.0, 0.8]) if tag is hmg.Tet64 else np.array([0.6, 0.8])


def medians(g, x, xi, form, moments_opt, extrema_opts):
    """medians (ms) of hmg_cell_moments with "cell_moments_windows" = moments_opt and, per value of "cell_extrema_windows" in
    extrema_opts, of hmg_cell_extrema with 0, 4 and 8 thresholds; and the window launches of the extrema the timed calls made"""
    ctx.set_option("cell_moments_windows", moments_opt)
    hmg.cell_moments(x, g, xi)                                        # warm-up: code objects, pool blocks, the element mask
    for opt in extrema_opts:
        ctx.set_option("cell_extrema_windows", opt)
        for thr in (None, THR4, THR8):
            hmg.cell_extrema(x, g, xi, form, thr)
    single, ext = [], {(opt, n): [] for opt in extrema_opts for n in (0, 4, 8)}
    launches = {opt: 0 for opt in extrema_opts}
    for _ in range(a.reps):
        hmg.cell_moments(x, g, xi)
        single.append(ctx.counter("cell_moments_kernel_ns") * 1e-6)
        for opt in extrema_opts:
            ctx.set_option("cell_extrema_windows", opt)
            n0 = ctx.counter("cell_extrema_window_launches")
            for n, thr in ((0, None), (4, THR4), (8, THR8)):
                hmg.cell_extrema(x, g, xi, form, thr)
                ext[(opt, n)].append(ctx.counter("cell_extrema_kernel_ns") * 1e-6)
            launches[opt] += ctx.counter("cell_extrema_window_launches") - n0
    ctx.set_option("cell_moments_windows", 0)
    ctx.set_option("cell_extrema_windows", 0)
    return statistics.median(single), {k: statistics.median(t) for k, t in ext.items()}, launches


def head(what, g, level):
    ndof = g.nf(level) * g.ncells()
    lines.append(f"{what} = {g.ncells()} cells, level {level} ({g.nf(level)} nodes and {hmg.fine_elements(g, level)} fine elements per "
                 f"cell, {ndof} DOFs, {8 * ndof / 1e9:.3f} GB per vector)")
    return ndof


def row(name, ms, ndof, ref=None, ref_name=""):
    tail = f"   / {ref_name} {ms / ref:6.3f}" if ref else ""
    lines.append(f"  {name:<52}{ms:9.3f} ms   {8 * ndof / (ms * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF{tail}")


try:
    # 1. 3D level 7: window extrema against window moments
    g, x, form, xi = problem(hmg.Tet64, a.width, 7)
    ndof = head(f"1. {a.width}^3 cubes x 6 tetrahedra", g, 7)
    s, e, n = medians(g, x, xi, form, 1, (1,))
    assert n[1] == 3 * a.reps
    row("k_cell_pair_moments_slab (v, v) (hmg_cell_moments)", s, ndof)
    for k in (0, 4, 8):
        row(f"k_cell_extrema_slab, {k} thresholds", e[(1, k)], ndof, s, "moments")
    x.close()
    g.close()
    # 2. 3D level 6: the window kernel against the LDS-resident one
    g, x, form, xi = problem(hmg.Tet64, a.width, 6)
    ndof = head(f"2. {a.width}^3 cubes x 6 tetrahedra", g, 6)
    s, e, n = medians(g, x, xi, form, 0, (0, 2))
    assert n[0] == 0 and n[2] == 3 * a.reps
    row("k_cell_pair_moments (v, v) (hmg_cell_moments)", s, ndof)
    for k in (0, 4, 8):
        row(f"k_cell_extrema (option 0), {k} thresholds", e[(0, k)], ndof, s, "moments")
        row(f"k_cell_extrema_slab (option 2), {k} thresholds", e[(2, k)], ndof, e[(0, k)], "option 0")
    x.close()
    g.close()
    # 3. 2D level 10 on 32 cells
    g, x, form, xi = problem(hmg.Tri64, a.width2d, 10)
    ndof = head(f"3. {a.width2d}^2 squares x 2 triangles", g, 10)
    s, e, n = medians(g, x, xi, form, 1, (1,))
    assert n[1] == 3 * a.reps
    row("k_cell_pair_moments_rows (v, v) (hmg_cell_moments)", s, ndof)
    for k in (0, 4, 8):
        row(f"k_cell_extrema_rows, {k} thresholds", e[(1, k)], ndof, s, "moments")
    lines.append("  (32 workgroups on 256 CUs: the time of one cell's walk, not a bandwidth)")
    x.close()
    g.close()
except Exception as err:                                  # the file says what could not be produced
    lines.append(f"NOT PRODUCED from here on: {type(err).__name__}: {err}")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
