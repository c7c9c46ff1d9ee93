#!/usr/bin/env python3
"""Timing of point sampling (hmg_sample, hmg_sample_raster; k_sample: one thread per point) next to what it replaces, the download
of the whole vector (DeviceMatrix.to_host), on the same grid, the same vector, in one process.
  python tools/dev/sample_timing.py [--case 32:6 16:7] [--raster 4096] [--points 1000000] [--reps 3] [--out profiles/sample_timing.txt]
A case is width:level -- width^3 cubes x 6 tetrahedra sampled on that level (32:6 is config 3's grid).  Per case: an axis-aligned
raster and an oblique one of raster^2 pixels through the middle of the domain (the oblique one hangs over it) and `points` random
points of the domain's box.  Kernel and download times come from the counters "sample_kernel_ns" (device events) and
"sample_download_ns" (host clock), medians of `reps` calls after a warm-up call; the locator's build is the host clock around the
first hmg_grid_locate; to_host is timed once with the host clock.  The file records what was measured.
  python tools/dev/sample_timing.py --periodic [--case 32:6] [--reps 11] [--out profiles/sample_torus_timing.txt]
k_sample_torus against k_sample: per case the ordinary grid hypercube(width) and the torus periodic_mesh(width) -- the same cube
count, level and vector size -- in one process, the same rasters and points relative to each one's box (the oblique raster hangs
over the box: outside on the ordinary grid, the next period on the torus), the calls of the two grids alternating; per piece of
work and grid the median, the smallest and the largest kernel time of `reps` calls, the medians of download and whole call, and
the ratio of the kernel medians."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import homogenization_jl_amd as hmg          # noqa: E402
from homogenization_jl_amd import driver     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", nargs="+", default=["32:6", "16:7"])
ap.add_argument("--raster", type=int, default=4096)
ap.add_argument("--points", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_timing.txt"))
ap.add_argument("--periodic", action="store_true", help="the torus periodic_mesh(width) against hypercube(width), alternating calls")
a = ap.parse_args()

ctx = hmg.Context(0)
lines = []


def periodic_case(width, L):
    grids = {"ordinary": (hmg.ImplicitFineGrid(ctx, driver.hypercube(hmg.Tet64, width), L), 1.0),        # the box [1, 1 + width]^3
             "torus": (hmg.ImplicitFineGrid(ctx, driver.periodic_mesh(hmg.Tet64, width), L), 0.0)}       # the box [0, width)^3
    grids["torus"][0].set_periodic_sampling(True)
    n = a.raster
    step = width / n
    ostep = 1.2 * step
    rng = np.random.default_rng(0)
    unit = width * rng.random((a.points, 3))
    xi = np.array([0.6, 0.0, 0.8])
    e1, e2 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    work, vecs = {}, {}
    for kind, (g, lo) in grids.items():
        v = vecs[kind] = hmg.DeviceMatrix(g, L).rand(1)
        mid = lo + 0.5 * width
        t0 = time.perf_counter()
        hmg.locate(g, L, np.full((1, 3), mid))
        t_build = time.perf_counter() - t0
        lines.append(f"  {kind:8s} {g.ncells()} cells, level {L}, {8 * g.ld(L) * g.ncells() / 1e9:.3f} GB per vector; locator built in "
                     f"{t_build * 1e3:.1f} ms on the host, {hmg.locator_counter('sample_locator_bytes') / 1e6:.2f} MB, longest "
                     f"candidate list {hmg.locator_counter('sample_locator_max_candidates')} cells")
        pts = np.ascontiguousarray(lo + unit)
        work[kind] = {
            "axis-aligned raster": lambda v=v, g=g, lo=lo, mid=mid: hmg.sample_raster(
                v, g, (lo + 0.5 * step, lo + 0.5 * step, mid + 0.3 * step), (step, 0, 0), (0, step, 0), n, n, xi=xi),
            "oblique raster": lambda v=v, g=g, mid=mid: hmg.sample_raster(
                v, g, np.full(3, mid) - 0.5 * n * ostep * (e1 + e2), ostep * e1, ostep * e2, n, n, xi=xi),
            "random points": lambda v=v, g=g, pts=pts: hmg.sample(v, g, pts, xi=xi),
        }
    for name in work["ordinary"]:
        t = {kind: {"kernel": [], "download": [], "wall": []} for kind in work}
        found = {}
        for kind in work:
            found[kind] = int((work[kind][name]()["cell"] >= 0).sum())          # warm-up: device tables, pool block, code object
        for _ in range(a.reps):
            for kind in work:                                                   # alternating
                t0 = time.perf_counter()
                s = work[kind][name]()
                t[kind]["wall"].append(time.perf_counter() - t0)
                t[kind]["kernel"].append(ctx.counter("sample_kernel_ns") * 1e-9)
                t[kind]["download"].append(ctx.counter("sample_download_ns") * 1e-9)
        npts = s["cell"].size
        for kind in work:
            k = t[kind]["kernel"]
            lines.append(f"  {name:20s} {kind:8s} {npts:9d} points ({found[kind]} with a cell): kernel {statistics.median(k) * 1e3:8.3f} ms "
                         f"(min {min(k) * 1e3:.3f}, max {max(k) * 1e3:.3f}), download {statistics.median(t[kind]['download']) * 1e3:8.3f} ms, "
                         f"whole call {statistics.median(t[kind]['wall']) * 1e3:8.3f} ms")
        lines.append(f"  {name:20s} kernel, torus / ordinary: "
                     f"{statistics.median(t['torus']['kernel']) / statistics.median(t['ordinary']['kernel']):.3f}")
    for kind in grids:
        vecs[kind].close()
        grids[kind][0].close()
    ctx.release_memory()


if a.periodic:
    for case in a.case:
        width, L = (int(t) for t in case.split(":"))
        lines.append(f"{width}^3 cubes x 6 tetrahedra, level {L}: k_sample on hypercube({width}) against k_sample_torus on periodic_mesh({width}); "
                     f"medians of {a.reps} alternating calls after a warm-up")
        periodic_case(width, L)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

for case in a.case:
    width, L = (int(t) for t in case.split(":"))
    base = driver.hypercube(hmg.Tet64, width)                                  # the box [1, 1 + width]^3
    g = hmg.ImplicitFineGrid(ctx, base, L)
    v = hmg.DeviceMatrix(g, L).rand(1)
    ndof = g.nf(L) * g.ncells()
    lo, hi = 1.0, 1.0 + width
    mid = 0.5 * (lo + hi)
    n = a.raster
    step = (hi - lo) / n
    t0 = time.perf_counter()
    hmg.locate(g, L, np.full((1, 3), mid))
    t_build = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    pts = lo + (hi - lo) * rng.random((a.points, 3))
    xi = np.array([0.6, 0.0, 0.8])
    e1, e2 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    ostep = 1.2 * step
    work = {
        "axis-aligned raster": lambda: hmg.sample_raster(v, g, (lo + 0.5 * step, lo + 0.5 * step, mid + 0.3 * step), (step, 0, 0), (0, step, 0), n, n, xi=xi),
        "oblique raster": lambda: hmg.sample_raster(v, g, np.full(3, mid) - 0.5 * n * ostep * (e1 + e2), ostep * e1, ostep * e2, n, n, xi=xi),
        "random points": lambda: hmg.sample(v, g, pts, xi=xi),
    }
    lines.append(f"{width}^3 cubes x 6 tetrahedra = {g.ncells()} cells, level {L} ({g.nf(L)} nodes per cell, {ndof} DOFs, "
                 f"{8 * g.ld(L) * g.ncells() / 1e9:.3f} GB per vector); medians of {a.reps} calls after a warm-up")
    lines.append(f"  locator: built in {t_build * 1e3:.1f} ms on the host (with the level's lattice table), "
                 f"{hmg.locator_counter('sample_locator_bytes') / 1e6:.2f} MB, longest candidate list "
                 f"{hmg.locator_counter('sample_locator_max_candidates')} cells")
    total = {}
    for name, call in work.items():
        s = call()                                                             # warm-up: device tables, pool block, code object
        npts = s["cell"].size
        found = int((s["cell"] >= 0).sum())
        kern, down, wall = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall.append(time.perf_counter() - t0)
            kern.append(ctx.counter("sample_kernel_ns") * 1e-9)
            down.append(ctx.counter("sample_download_ns") * 1e-9)
        k, d, w = statistics.median(kern), statistics.median(down), statistics.median(wall)
        total[name] = w
        lines.append(f"  {name:20s} {npts:9d} points ({found} inside): kernel {k * 1e3:9.3f} ms = {npts / k / 1e9:6.3f} G points/s "
                     f"({32 * found / k / 1e9:7.1f} GB/s of 4 gathered doubles per inside point), download of value, gradient and cell "
                     f"({npts * 36 / 1e6:.0f} MB) {d * 1e3:9.3f} ms, whole call {w * 1e3:9.3f} ms")
    t0 = time.perf_counter()
    xh = v.to_host()
    t_host = time.perf_counter() - t0
    del xh
    lines.append(f"  DeviceMatrix.to_host() of the same vector: {t_host:.3f} s")
    for name, w in total.items():
        lines.append(f"    to_host / whole call, {name}: {t_host / w:.1f}")
    v.close()
    g.close()
    ctx.release_memory()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
