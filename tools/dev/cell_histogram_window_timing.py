#!/usr/bin/env python3
"""Timing of the per-cell histograms of cells larger than the LDS (context option "cell_histogram_windows",
csrc/hmg_histogram_window.hip) and of the group sums on the device (hmg_cell_histogram_groups) on one GPU, four comparisons in
one process:
  1. 3D level 7, 16^3 cubes x 6 tetrahedra (24 576 cells): k_cell_histogram_slab with 67 and with 1 027 bins against
     k_cell_extrema_slab with eight thresholds on the same vector -- the kernel that answers the same question in 13 passes;
  2. 3D level 6, the same width: the window kernel (option 2) against k_cell_histogram (option 0), both rules;
  3. 2D level 10 on 32 cells (4^2 squares x 2 triangles): k_cell_histogram_rows against k_cell_extrema_rows with eight thresholds
     -- 32 workgroups on 256 CUs: the time of one cell's walk;
  4. the grid of 1.: api.cell_histogram_groups with 2 and with 64 groups against api.cell_histogram plus the host's sums
     (fields.histogram_volume with labels and the integer sums) -- the WHOLE call by the host clock: kernel, download, widening.
  python tools/dev/cell_histogram_window_timing.py [--width 16] [--width2d 4] [--reps 11] [--out profiles/cell_histogram_window.txt]
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_histogram_kernel_ns",
"cell_extrema_kernel_ns", "cell_histogram_groups_kernel_ns"), after a warm-up call of each; medians of `reps` synchronised calls
that alternate the candidates.  No time is a threshold of anything: the file records what was measured.  `--append FILE` copies
the lines of FILE (say, bench.py's result lines of this tree and of its parent from the same session) behind the report."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver, fields     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=16)
ap.add_argument("--width2d", type=int, default=4)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_histogram_window.txt"))
ap.add_argument("--append", default=None)
a = ap.parse_args()

OPT, XOPT = "cell_histogram_windows", "cell_extrema_windows"
ctx = hmg.Context(0)
lines = ["Per-cell histograms of cells larger than the LDS (context option \"cell_histogram_windows\", csrc/hmg_histogram_window.hip) "
         "and group sums on the device (hmg_cell_histogram_groups), one MI355X; medians of %d alternating calls after a warm-up, "
         "kernel times from device events" % a.reps]


def problem(tag, width, level):
    base, cond, g, op = driver.checkerboard_problem(ctx, tag, width, level, seed=0, lam=0.0)
    x = hmg.DeviceMatrix(g, level).rand(1)
    hmg.broadcast_interfaces(x, g, level)
    return base, g, x, fields.energy_form(cond), np.array([0.6, 0.0, 0.8]) if tag is hmg.Tet64 else np.array([0.6, 0.8])


def rules(g, x, xi, form, xopt):
    """67 bins (8 octaves x 8) and 1 027 bins (32 octaves x 32) that end at the octave of the median of the cells' maxima, and
    eight thresholds spread over the 8 octaves"""
    ctx.set_option(XOPT, xopt)
    qmax, _, _ = hmg.cell_extrema(x, g, xi, form)
    ctx.set_option(XOPT, 0)
    top = int(np.ceil(np.log2(np.median(qmax))))
    return {67: dict(emin=top - 8, emax=top, sub_bits=3), 1027: dict(emin=top - 32, emax=top, sub_bits=5)}, 2.0 ** np.arange(top - 8, top)


def medians(g, x, xi, form, thr, rule, hist_opts, xopt):
    """medians (ms) of hmg_cell_extrema with the thresholds thr ("cell_extrema_windows" = xopt) and, per value of
    "cell_histogram_windows" in hist_opts and per rule, of hmg_cell_histogram; and the window launches the timed histogram calls made"""
    def extrema():
        ctx.set_option(XOPT, xopt)
        hmg.cell_extrema(x, g, xi, form, thr)
        ctx.set_option(XOPT, 0)
        return ctx.counter("cell_extrema_kernel_ns") * 1e-6

    def histogram(opt, nb):
        ctx.set_option(OPT, opt)
        hmg.cell_histogram(x, g, xi, form, **rule[nb])
        ctx.set_option(OPT, 0)
        return ctx.counter("cell_histogram_kernel_ns") * 1e-6

    extrema()                                                         # warm-up: code objects, pool blocks, the element mask
    for opt in hist_opts:
        for nb in rule:
            histogram(opt, nb)
    ext, hist = [], {(opt, nb): [] for opt in hist_opts for nb in rule}
    n0 = ctx.counter("cell_histogram_window_launches")
    for _ in range(a.reps):
        ext.append(extrema())
        for key in hist:
            hist[key].append(histogram(*key))
    return statistics.median(ext), {k: statistics.median(t) for k, t in hist.items()}, ctx.counter("cell_histogram_window_launches") - n0


def head(what, g, level):
    ndof = g.nf(level) * g.ncells()
    lines.append(f"{what} = {g.ncells()} cells, level {level} ({g.nf(level)} nodes and {hmg.fine_elements(g, level)} fine elements per "
                 f"cell, {ndof} DOFs, {8 * ndof / 1e9:.3f} GB per vector)")
    return ndof


def row(name, ms, ndof, ref=None, ref_name=""):
    tail = f"   / {ref_name} {ms / ref:6.3f}" if ref else ""
    lines.append(f"  {name:<58}{ms:9.3f} ms   {8 * ndof / (ms * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF{tail}")


def wall(call):
    ctx.sync()
    t0 = time.perf_counter()
    out = call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


try:
    # 1. 3D level 7: window histogram against the window extrema with eight thresholds
    base, g, x, form, xi = problem(hmg.Tet64, a.width, 7)
    ndof = head(f"1. {a.width}^3 cubes x 6 tetrahedra", g, 7)
    rule, thr = rules(g, x, xi, form, 1)
    e, h, n = medians(g, x, xi, form, thr, rule, (1,), 1)
    assert n == 2 * a.reps
    row("k_cell_extrema_slab, 8 thresholds", e, ndof)
    for nb in rule:
        row(f"k_cell_histogram_slab, {nb} bins", h[(1, nb)], ndof, e, "extrema")
    # 4. group sums on the device against the rows brought down and summed on the host (the same grid and vector)
    ne = g.ncells()
    nel = hmg.fine_elements(g, 7)
    vol = fields.cell_volumes(base)
    w = vol / float(nel)
    lines.append(f"4. the grid of 1.: phase histograms, the whole call by the host clock (kernels, downloads, host sums)")
    ctx.set_option(OPT, 1)
    for ngroups in (2, 64):
        labels = (np.arange(ne) * 7919) % ngroups
        for nb in rule:
            def on_host():
                counts = hmg.cell_histogram(x, g, xi, form, **rule[nb])
                byl = fields.histogram_volume(counts, vol, nel, labels=labels)
                sums = np.stack([counts[labels == k].sum(axis=0) for k in range(ngroups)])
                return sums, byl

            def on_device():
                return hmg.cell_histogram_groups(x, g, labels, xi, form, w, **rule[nb])

            (_, (sums, byl)), (_, (lab, counts, volume)) = wall(on_host), wall(on_device)       # warm-up, and the results agree
            assert np.array_equal(sums, counts)
            worst = max(np.abs(volume[k] - byl[int(l)]).max() / np.abs(byl[int(l)]).max() for k, l in enumerate(lab))
            th, td, kg = [], [], []
            for _ in range(a.reps):
                th.append(wall(on_host)[0])
                td.append(wall(on_device)[0])
                kg.append(ctx.counter("cell_histogram_groups_kernel_ns") * 1e-6)
            mh, md = statistics.median(th), statistics.median(td)
            lines.append(f"  {ngroups:3d} groups, {nb:4d} bins: cell_histogram + host sums {mh:9.2f} ms   cell_histogram_groups {md:9.2f} ms"
                         f"   ratio {md / mh:6.3f}   (k_histogram_groups {statistics.median(kg):7.3f} ms; {ne * nb * 4 / 1e6:.1f} MB of rows "
                         f"stay on the device, {ngroups * nb * 16 / 1e3:.1f} KB come down; volumes agree to {worst:.1e})")
    ctx.set_option(OPT, 0)
    x.close()
    g.close()
    # 2. 3D level 6: the window kernel against the LDS-resident one
    base, g, x, form, xi = problem(hmg.Tet64, a.width, 6)
    ndof = head(f"2. {a.width}^3 cubes x 6 tetrahedra", g, 6)
    rule, thr = rules(g, x, xi, form, 0)
    e, h, n = medians(g, x, xi, form, thr, rule, (0, 2), 0)
    assert n == 2 * a.reps
    row("k_cell_extrema, 8 thresholds", e, ndof)
    for nb in rule:
        row(f"k_cell_histogram (option 0), {nb} bins", h[(0, nb)], ndof, e, "extrema")
        row(f"k_cell_histogram_slab (option 2), {nb} bins", h[(2, nb)], ndof, h[(0, nb)], "option 0")
    x.close()
    g.close()
    # 3. 2D level 10 on 32 cells
    base, g, x, form, xi = problem(hmg.Tri64, a.width2d, 10)
    ndof = head(f"3. {a.width2d}^2 squares x 2 triangles", g, 10)
    rule, thr = rules(g, x, xi, form, 1)
    e, h, n = medians(g, x, xi, form, thr, rule, (1,), 1)
    assert n == 2 * a.reps
    row("k_cell_extrema_rows, 8 thresholds", e, ndof)
    for nb in rule:
        row(f"k_cell_histogram_rows, {nb} bins", h[(1, nb)], ndof, e, "extrema")
    lines.append(f"  ({g.ncells()} workgroups on 256 CUs: the time of one cell's walk, not a bandwidth.  Workgroups per CU the kernel can "
                 "hold: two -- 50 VGPRs (eight waves per SIMD) and 80 912 B of LDS at 1 027 bins, 161 824 B of 163 840 B for two; "
                 "profiles/cell_histogram_window_kernel_resources.txt.  With one workgroup per cell and fewer cells than CUs here, one "
                 "is resident per CU in this run)")
    x.close()
    g.close()
except Exception as err:                                  # the file says what could not be produced
    lines.append(f"NOT PRODUCED from here on: {type(err).__name__}: {err}")
if a.append and os.path.exists(a.append):
    lines.append("bench.py --gpus 1 in the same session, this tree and its parent (no launch of a V-cycle changes: expected unchanged):")
    lines += ["  " + ln.rstrip("\n") for ln in open(a.append) if ln.strip()]
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
