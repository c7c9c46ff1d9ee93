#!/usr/bin/env python3
"""Timing of the per-cell histograms over the fine elements (hmg_cell_histogram, k_cell_histogram: 8 B/DOF, 8 LDS reads, 6
quadratic forms and up to 6 LDS integer adds per node) next to hmg_cell_extrema with 8 thresholds on the same vector, which is
the yardstick: the same grid, the same rows, one process.
  python tools/dev/cell_histogram_timing.py [--cases 3:16 3:8 2:64] [--reps 11] [--out profiles/cell_histogram.txt]
A case is dim:width: the width^dim checkerboard on 6 (2D: 8) levels.  Per case three vectors: (a) a consistent random vector --
many bins per wave; (b) v = 0 with xi -- every element of a cell in one bin, the same-address worst case; (c) a corrector of the
plain Dirichlet cell problem solved to 1e-6 on that grid.  Per vector the histogram with 67 bins (8 octaves, sub_bits 3) and with
1 027 bins (32 octaves, sub_bits 5) around the median of the cells' mean q, from each of the three ways of bringing counts into
LDS (option "cell_histogram_variant": 0 one add per element, 1 a node's elements combined first, 2 and the wave's first bin
summed across lanes), and the extrema call with thresholds at 8 edges of the 67-bin rule.
The kernels' times come from device events inside the calls (hmg_ctx_counter "cell_histogram_kernel_ns",
"cell_extrema_kernel_ns"), after a warm-up call of each; medians of `reps` synchronised calls that alternate all of them, with
the spread (max - min) / median.  All variants must give the same counts; the script checks it."""
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
ap.add_argument("--cases", nargs="+", default=["3:16", "3:8", "2:64"])
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--no-corrector", action="store_true", help="skip vector (c)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_histogram.txt"))
a = ap.parse_args()

VARIANTS = {0: "one add per element", 1: "node combined", 2: "node + wave combined"}
ctx = hmg.Context(0)
default_variant = ctx.counter("cell_histogram_variant")
lines = []


def med(t):
    m = statistics.median(t)
    return m, (max(t) - min(t)) / m


for case in a.cases:
    dim, width = (int(s) for s in case.split(":"))
    L = 6 if dim == 3 else 8
    eltype = hmg.Tet64 if dim == 3 else hmg.Tri64
    base, cond, g, op = driver.checkerboard_problem(ctx, eltype, width, L, seed=0, lam=0.0)
    ndof = g.nf(L) * g.ncells()
    nel = hmg.fine_elements(g, L)
    form = fields.energy_form(cond)
    xi = np.array([0.6, 0.0, 0.8]) if dim == 3 else np.array([0.6, 0.8])
    lines.append(f"{width}^{dim} cubes = {g.ncells()} cells, level {L} ({g.nf(L)} nodes and {nel} fine elements per cell, {ndof} DOFs, "
                 f"{8 * ndof / 1e9:.3f} GB per vector); medians of {a.reps} alternating calls after a warm-up, device events, "
                 f"spread = (max - min) / median")
    states = [hmg.LevelState(g, i + 1) for i in range(L)]
    x = states[-1].x
    vectors = ["a", "b"] + ([] if a.no_corrector else ["c"])
    t_a = {}
    for vec in vectors:
        if vec == "a":
            x.rand(1)
            hmg.broadcast_interfaces(x, g, L)
            what = "(a) consistent random vector"
        elif vec == "b":
            x.fill(0.0)
            what = "(b) v = 0 with xi: one bin per cell"
        else:
            cycles, rnorm, r0 = driver._dirichlet_solve(g, op, hmg.BaseLevel(g), states, x, None, xi, 3, 1e-6, 60, "cell_histogram_timing")
            what = f"(c) corrector, residual {rnorm / r0:.1e} after {cycles} V-cycles"
        mean, gram = hmg.cell_moments(x, g, xi)
        dens = fields.energy(cond, gram) / fields.cell_volumes(base)
        c = int(np.rint(np.log2(np.median(dens))))
        rules = {67: dict(emin=c - 4, emax=c + 4, sub_bits=3), 1027: dict(emin=c - 16, emax=c + 16, sub_bits=5)}
        E = hmg.histogram_edges(**rules[67])
        thr8 = np.nextafter(E[::8][:8], -np.inf)
        # warm-up: code objects, pool blocks, the element mask; and the variants' counts against each other
        hmg.cell_extrema(x, g, xi, form, thr8)
        bins_used = {}
        for nb, rule in rules.items():
            ref = None
            for var in VARIANTS:
                ctx.set_option("cell_histogram_variant", var)
                counts = hmg.cell_histogram(x, g, xi, form, **rule)
                assert counts.shape[1] == nb and (counts.sum(axis=1) == nel).all()
                if ref is None:
                    ref = counts
                assert np.array_equal(counts, ref), (case, vec, nb, var)
            bins_used[nb] = (int((ref > 0).sum(axis=1).max()), float(1.0 - ref[:, 1:-2].sum() / ref.sum()))
        ext, hist = [], {(nb, var): [] for nb in rules for var in VARIANTS}
        for _ in range(a.reps):
            hmg.cell_extrema(x, g, xi, form, thr8)
            ext.append(ctx.counter("cell_extrema_kernel_ns") * 1e-6)
            for nb, rule in rules.items():
                for var in VARIANTS:
                    ctx.set_option("cell_histogram_variant", var)
                    hmg.cell_histogram(x, g, xi, form, **rule)
                    hist[(nb, var)].append(ctx.counter("cell_histogram_kernel_ns") * 1e-6)
        ctx.set_option("cell_histogram_variant", default_variant)
        print(f"# {case} {what}: timed", file=sys.stderr, flush=True)
        e, es = med(ext)
        lines.append(f"  {what}; bins centred at 2^{c}")
        lines.append(f"    k_cell_extrema, 8 thresholds              {e:9.3f} ms  spread {es:5.3f}   {8 * ndof / (e * 1e-3) / 1e12:6.3f} TB/s on 8 B/DOF   (the yardstick)")
        for nb in rules:
            for var, name in VARIANTS.items():
                h, hs = med(hist[(nb, var)])
                t_a[(vec, nb, var)] = h
                tag = " (default)" if var == default_variant else ""
                lines.append(f"    k_cell_histogram, {nb:4d} bins, variant {var}{tag:10s} {h:9.3f} ms  spread {hs:5.3f}   "
                             f"{8 * ndof / (h * 1e-3) / 1e12:6.3f} TB/s   histogram / extrema {h / e:6.3f}   [{name}]")
            lines.append(f"      ({nb} bins: at most {bins_used[nb][0]} bins of a cell hold anything; {100 * bins_used[nb][1]:.2f} % of the elements "
                         f"outside the regular bins)")
    for nb in (67, 1027):
        lines.append("  (b) / (a), " + f"{nb} bins: " +
                     ", ".join(f"variant {var} {t_a[('b', nb, var)] / t_a[('a', nb, var)]:5.2f}" for var in VARIANTS))
    for st in states:
        st.close()
    g.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
