#!/usr/bin/env python3
"""Wall-clock of the whole driver to a tolerance: device path vs the CPU oracle, identical inputs.
  python tools/driver_bench.py --n 1 --dim 3 --refinements 4 --tolerance 1e-5 [--no-cpu] [--accelerate] [--contrast 100] [--smoother jacobi]
--accelerate: the V-cycle preconditions a flexible CG iteration (driver.checkerboard_homogenization(accelerate=True)); the CPU
oracle has the stationary iteration only, so --accelerate implies --no-cpu.
--smoother jacobi | chebyshev: the V-cycle's smoother is the Jacobi-preconditioned CG or the Chebyshev-Jacobi polynomial (driver keyword
smoother=); the CPU oracle has the
reference's smoother only, so it implies --no-cpu as well.
--tensor [--repeats R] [--warmup W]: the full homogenized tensor.  One run of driver.checkerboard_homogenization_tensor (d corrector
solves, one setup) against the d (d + 1) / 2 runs of the scalar driver that polarising by hand takes (xi = e_i and
(e_i + e_j) / sqrt 2), same field, same seed, in one process: W untimed rounds of both first (code objects, the pool of
level-vector memory), then R timed rounds that alternate the two; wall clock around whole runs, each of which ends in a device
synchronise.  Prints the times of every round, their medians, the ratio and the largest difference of the two tensors.
--polycrystal: the field is driver.generate_polycrystal (one rotated tensor per unit cube, principal conductivities 1 and
--contrast, in 3D 1, --contrast and their geometric mean) instead of the two-valued diagonal field; the CPU oracle knows diagonal
tensors only, so it implies --no-cpu.
--field-seed S: the seed of the coefficient field (default 5), e.g. for a figure over several fields.
--dirichlet-tensor: driver.dirichlet_homogenization_tensor on hypercube(n) (d solves of the plain Dirichlet cell problem on one grid,
then d (d + 1) / 2 per-cell moment passes): one line with the wall time of a run after --warmup untimed ones, the cycles and the
kernel counters of its last single-vector and its last pair pass ("cell_moments_kernel_ns", "cell_pair_moments_kernel_ns").
--large-cells (with --dirichlet-tensor): the driver's keyword large_cells=True -- a top level whose cell exceeds the LDS (3D level 7,
2D levels 9-11: --refinements 6 / 8-10) takes the window kernels; the line then carries "cell_moments_window_launches" too.
--extrema: driver.dirichlet_homogenization on hypercube(n) with extrema=True and thresholds at 1, 2 and 4 times the homogenized
energy density (one solve, the moment pass, then the pass over the fine elements): one line with the wall time of a run after
--warmup untimed ones, the largest concentration, the exceedance volume fractions and the kernel counters of the two passes
("cell_moments_kernel_ns", "cell_extrema_kernel_ns").  Top levels up to 6 in 3D (--refinements 5) and 8 in 2D; with --large-cells
(the driver's keyword large_cells=True) 3D level 7 and 2D levels 9-11 too, through the window kernels of both passes: the line then
carries "cell_moments_window_launches" and "cell_extrema_window_launches".
--locations (with --extrema): the driver's keyword locations=True -- the pass also reports which fine element holds each cell's
peak (hmg_cell_extrema_where); the ten hottest spots are printed in front of the line (cell, peak over the homogenized energy
density, position, the energy density sampled there), and the line carries "cell_extrema_where_kernel_ns" instead.
--slice N: driver.dirichlet_homogenization on hypercube(n) with slices=[one axis-aligned N x N raster through the middle of the
domain] (one solve, the moment pass, then hmg_sample_raster with the flux and the energy density per pixel): one line with the wall
time of a run after --warmup untimed ones, the pixels inside the domain, the largest sampled energy density over the homogenized
one and the counters "sample_kernel_ns", "sample_download_ns", "sample_locator_bytes", "sample_locator_max_candidates".
--histogram: driver.dirichlet_homogenization on hypercube(n) with histogram=True (one solve, the moment pass, then the histogram
pass over the fine elements with Q = sigma_c / energy_form, 259 bins over 2^-24 .. 2^8 times the mean energy density): the volume
fraction of every occupied bin as a text table, the intervals that hold the median and the 99 % quantile, then one line with the
wall time of a run after --warmup untimed ones and the counters "cell_histogram_kernel_ns", "cell_histogram_launches",
"cell_histogram_window_launches".  Top levels up to 6 in 3D (--refinements 5) and 8 in 2D; with --large-cells 3D level 7 and 2D
levels 9-11 too, through the histogram's window kernels.
--uniaxial: driver.uniaxial_homogenization_tensor on hypercube(n) (d solves on one grid, the two faces normal to e_k as the grid's
Dirichlet set in front of solve k): one line with the wall time of a run after --warmup untimed ones, the cycles and the tensor.
--periodic: driver.periodic_homogenization_tensor on periodic_mesh(n) (d solves of the periodic cell problem on a torus of n^d unit
cubes, n >= 3, lambda = 0, the level-1 solve on the complement of the constants): the same line.
--periodic --slice N: the same driver with slices=[one axis-aligned N x N raster over two periods per axis, from half a period in
front of the box, through the middle of the third axis]: every corrector u_k is sampled on it (hmg_sample_raster on the torus);
the line also carries the pixels, the pixels with a cell (all of them, on a torus), the largest difference of a gradient between
pixels one period apart, and the sampling counters of the last pass.
--blocks B: driver.block_homogenization_tensor(n, B) (the Dirichlet cell problems of all (n / B)^d blocks in d solves on one grid)
against the same number of dirichlet_homogenization_tensor(B) runs on the blocks' own meshes, in one process: the two wall times
after --warmup untimed rounds of both, their ratio and the largest relative difference of a block's tensor."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1)
ap.add_argument("--dim", type=int, default=3)
ap.add_argument("--refinements", type=int, default=4)
ap.add_argument("--tolerance", type=float, default=1e-5)
ap.add_argument("--no-cpu", action="store_true")
ap.add_argument("--accelerate", action="store_true")
ap.add_argument("--smoother", choices=("cg", "jacobi", "chebyshev"), default="cg")
ap.add_argument("--contrast", type=float, default=9.0, help="sigma takes the values 1 and this")
ap.add_argument("--tensor", action="store_true", help="one tensor run against d (d + 1) / 2 scalar runs")
ap.add_argument("--polycrystal", action="store_true", help="one rotated tensor per unit cube (implies --no-cpu)")
ap.add_argument("--field-seed", type=int, default=5, help="seed of the coefficient field")
ap.add_argument("--dirichlet-tensor", action="store_true", help="the Dirichlet tensor driver on hypercube(n): wall time, counters")
ap.add_argument("--large-cells", action="store_true", help="with --dirichlet-tensor, --extrema or --histogram: per-cell passes of cells larger than the LDS")
ap.add_argument("--extrema", action="store_true", help="the Dirichlet driver with the pass over the fine elements: wall time, counters")
ap.add_argument("--locations", action="store_true", help="with --extrema: where the peaks sit; prints the ten hottest spots")
ap.add_argument("--histogram", action="store_true", help="the Dirichlet driver with the histogram pass: volume fractions per bin, "
                "median and 99 % intervals, wall time, counters")
ap.add_argument("--slice", type=int, default=0, metavar="N", help="the Dirichlet driver with one axis-aligned N x N slice through the "
                "middle of the domain: wall time, sampling counters")
ap.add_argument("--uniaxial", action="store_true", help="the uniaxial tensor driver on hypercube(n): wall time, cycles, tensor")
ap.add_argument("--periodic", action="store_true", help="the periodic tensor driver on the torus periodic_mesh(n): wall time, cycles, tensor")
ap.add_argument("--blocks", type=int, default=0, metavar="B", help="block upscaling of hypercube(n) in blocks of B cubes per axis "
                "against one Dirichlet tensor run per block")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
width = 2 * (driver.compute_box_radius(0, a.n) + driver.compute_boundary_layer(1.0, a.n))
if a.polycrystal:
    principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
    sgrid = driver.generate_polycrystal(a.dim, width, a.field_seed, principal)
else:
    sgrid = driver.generate_conductivity(a.dim, width, a.field_seed, values=(1.0, a.contrast))
tag = hmg.Tet64 if a.dim == 3 else hmg.Tri64
ctx = hmg.Context(0)
if a.slice and not a.periodic:
    if a.polycrystal:
        principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
        sgrid = driver.generate_polycrystal(a.dim, a.n, a.field_seed, principal)
    else:
        sgrid = driver.generate_conductivity(a.dim, a.n, a.field_seed, values=(1.0, a.contrast))
    xi = np.ones(a.dim) / np.sqrt(a.dim)
    step = a.n / a.slice
    origin = np.full(a.dim, 1.0 + 0.5 * step)                   # hypercube(n) is the box [1, 1 + n]^dim
    if a.dim == 3:
        origin[2] = 1.0 + 0.5 * a.n + 0.3 * step                # the middle of the box, off the lattice planes
    du, dv = np.zeros(a.dim), np.zeros(a.dim)
    du[0] = dv[1] = step
    kw = dict(refinements=a.refinements, xi=xi, tolerance=a.tolerance, ctx=ctx, sigma_grid=sgrid, accelerate=a.accelerate,
              smoother=a.smoother, slices=[(origin, du, dv, a.slice, a.slice)])
    for _ in range(a.warmup):
        driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    t0 = time.perf_counter()
    r = driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    wall = time.perf_counter() - t0
    s = r["slices"][0]
    print(json.dumps({"config": f"dirichlet_homogenization({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance}, "
                                f"slices=[{a.slice} x {a.slice}])",
                      "accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal,
                      "warmup": a.warmup, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"],
                      "energy_form": r["energy_form"], "pixels": int(s["cell"].size), "pixels_inside": int((s["cell"] >= 0).sum()),
                      "max_energy_density_over_mean": float(np.nanmax(s["energy_density"]) / r["energy_form"]),
                      "sample_kernel_ns": ctx.counter("sample_kernel_ns"), "sample_download_ns": ctx.counter("sample_download_ns"),
                      "sample_locator_bytes": ctx.counter("sample_locator_bytes"),
                      "sample_locator_max_candidates": ctx.counter("sample_locator_max_candidates")}))
    sys.exit(0)
if a.extrema:
    if a.polycrystal:
        principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
        sgrid = driver.generate_polycrystal(a.dim, a.n, a.field_seed, principal)
    else:
        sgrid = driver.generate_conductivity(a.dim, a.n, a.field_seed, values=(1.0, a.contrast))
    xi = np.ones(a.dim) / np.sqrt(a.dim)
    kw = dict(refinements=a.refinements, xi=xi, tolerance=a.tolerance, ctx=ctx, sigma_grid=sgrid, accelerate=a.accelerate,
              smoother=a.smoother, extrema=True, thresholds=[1.0, 2.0, 4.0], fields=True, large_cells=a.large_cells,
              locations=a.locations)
    for _ in range(a.warmup):
        driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    t0 = time.perf_counter()
    r = driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    wall = time.perf_counter() - t0
    if a.locations:
        h = r["hot_spots"]
        for c, val, pt, smp in zip(h["cell"], h["value"], h["point"], h["sampled"]):
            print(f"hot spot: cell {int(c):7d}  peak / mean {val / r['energy_form']:10.4f}  at ({', '.join(f'{x:.6f}' for x in pt)})  "
                  f"sampled there / mean {smp / r['energy_form']:10.4f}")
    print(json.dumps({"config": f"dirichlet_homogenization({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance}, "
                                f"extrema=True{', large_cells=True' if a.large_cells else ''}"
                                f"{', locations=True' if a.locations else ''})",
                      "accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal,
                      "warmup": a.warmup, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"],
                      "energy_form": r["energy_form"], "max_concentration": float(r["concentration"].max()),
                      "min_energy_density_over_mean": float(r["min_energy_density"].min() / r["energy_form"]),
                      "exceedance_fraction_at_1_2_4": (r["exceedance"].sum(axis=0) / r["volume"]).tolist(),
                      "cell_moments_kernel_ns": ctx.counter("cell_moments_kernel_ns"),
                      ("cell_extrema_where_kernel_ns" if a.locations else "cell_extrema_kernel_ns"):
                          ctx.counter("cell_extrema_where_kernel_ns" if a.locations else "cell_extrema_kernel_ns"),
                      "large_cells": a.large_cells,
                      "cell_moments_window_launches": ctx.counter("cell_moments_window_launches"),
                      "cell_extrema_window_launches": ctx.counter("cell_extrema_window_launches")}))
    sys.exit(0)
if a.histogram:
    from homogenization_jl_amd import fields
    if a.polycrystal:
        principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
        sgrid = driver.generate_polycrystal(a.dim, a.n, a.field_seed, principal)
    else:
        sgrid = driver.generate_conductivity(a.dim, a.n, a.field_seed, values=(1.0, a.contrast))
    xi = np.ones(a.dim) / np.sqrt(a.dim)
    kw = dict(refinements=a.refinements, xi=xi, tolerance=a.tolerance, ctx=ctx, sigma_grid=sgrid, accelerate=a.accelerate,
              smoother=a.smoother, histogram=True, large_cells=a.large_cells)
    for _ in range(a.warmup):
        driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    t0 = time.perf_counter()
    r = driver.dirichlet_homogenization(a.n, tag, **kw)
    ctx.sync()
    wall = time.perf_counter() - t0
    h = r["energy_density_histogram"]
    E, vol = h["edges"], h["volume"]
    frac = vol / r["volume"]
    bounds = np.concatenate(([-np.inf], E, [np.inf]))
    print("energy density / mean           volume fraction")
    for b in np.flatnonzero(vol[:-1] > 0.0):
        print(f"[{bounds[b]:12.5e}, {bounds[b + 1]:12.5e})   {frac[b]:10.6f}  {'#' * int(round(60 * frac[b] / frac[:-1].max()))}")
    if vol[-1] > 0.0:
        print(f"NaN                            {frac[-1]:10.6f}")
        median = q99 = (float("nan"), float("nan"))
    else:
        median, q99 = fields.histogram_quantile(vol, E, 0.5), fields.histogram_quantile(vol, E, 0.99)
        print(f"median in [{median[0]:.5e}, {median[1]:.5e}), 99 % quantile in [{q99[0]:.5e}, {q99[1]:.5e}) times the mean")
    print(json.dumps({"config": f"dirichlet_homogenization({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance}, "
                                f"histogram=True{', large_cells=True' if a.large_cells else ''})",
                      "accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal,
                      "warmup": a.warmup, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"],
                      "energy_form": r["energy_form"], "bins": int(vol.shape[0]), "bins_occupied": int((vol > 0.0).sum()),
                      "median_interval": list(median), "q99_interval": list(q99),
                      "cell_moments_kernel_ns": ctx.counter("cell_moments_kernel_ns"),
                      "cell_histogram_kernel_ns": ctx.counter("cell_histogram_kernel_ns"),
                      "cell_histogram_launches": ctx.counter("cell_histogram_launches"), "large_cells": a.large_cells,
                      "cell_histogram_window_launches": ctx.counter("cell_histogram_window_launches")}))
    sys.exit(0)
if a.uniaxial or a.blocks or a.periodic:
    if a.polycrystal:
        principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
        sgrid = driver.generate_polycrystal(a.dim, a.n, a.field_seed, principal)
    else:
        sgrid = driver.generate_conductivity(a.dim, a.n, a.field_seed, values=(1.0, a.contrast))
    kw = dict(refinements=a.refinements, tolerance=a.tolerance, ctx=ctx, accelerate=a.accelerate, smoother=a.smoother)
    common = {"accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal, "warmup": a.warmup}

    def timed(run):
        for _ in range(a.warmup):
            run()
        ctx.sync()
        t0 = time.perf_counter()
        r = run()
        ctx.sync()
        return r, time.perf_counter() - t0

    if a.uniaxial:
        r, wall = timed(lambda: driver.uniaxial_homogenization_tensor(a.n, tag, sigma_grid=sgrid, **kw))
        print(json.dumps({"config": f"uniaxial_homogenization_tensor({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance})",
                          **common, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"], "tensor": r["tensor"].tolist(),
                          "max_abs_diff_to_flux_form": float(np.abs(r["tensor"] - r["tensor_flux"]).max())}))
        sys.exit(0)
    if a.periodic:
        extra, what = {}, ""
        if a.slice:
            if a.slice % 2:
                sys.exit("--periodic --slice N: N must be even (two periods, whole pixels per period)")
            step = 2.0 * a.n / a.slice
            origin = np.full(a.dim, -0.5 * a.n + 0.25 * step)        # the torus periodic_mesh(n) has the box [0, n)^dim
            if a.dim == 3:
                origin[2] = 0.5 * a.n + 0.3 * step                   # off the lattice planes
            du, dv = np.zeros(a.dim), np.zeros(a.dim)
            du[0] = dv[1] = step
            kw["slices"] = [(origin, du, dv, a.slice, a.slice)]
            what = f", slices=[{a.slice} x {a.slice}]"
        r, wall = timed(lambda: driver.periodic_homogenization_tensor(a.n, tag, sigma_grid=sgrid, **kw))
        if a.slice:
            per_k, h = r["slices"][0], a.slice // 2
            extra = {"pixels": int(per_k[0]["cell"].size), "pixels_inside": int((per_k[0]["cell"] >= 0).sum()),
                     "max_gradient_diff_one_period_apart": max(float(np.abs(s["gradient"][:h, :h] - s["gradient"][h:, h:]).max()) for s in per_k),
                     "sample_kernel_ns": ctx.counter("sample_kernel_ns"), "sample_download_ns": ctx.counter("sample_download_ns"),
                     "sample_locator_bytes": ctx.counter("sample_locator_bytes"),
                     "sample_locator_max_candidates": ctx.counter("sample_locator_max_candidates")}
        print(json.dumps({"config": f"periodic_homogenization_tensor({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance}{what})",
                          **common, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"], "tensor": r["tensor"].tolist(),
                          "max_abs_diff_to_flux_form": float(np.abs(r["tensor"] - r["tensor_flux"]).max()), **extra}))
        sys.exit(0)
    nb = a.n // a.blocks
    subs = {idx: np.ascontiguousarray(sgrid[tuple(slice(a.blocks * i, a.blocks * (i + 1)) for i in idx)]) for idx in np.ndindex(*(nb,) * a.dim)}
    r, wall = timed(lambda: driver.block_homogenization_tensor(a.n, a.blocks, tag, sigma_grid=sgrid, **kw))
    alone, wall_alone = timed(lambda: {idx: driver.dirichlet_homogenization_tensor(a.blocks, tag, sigma_grid=s, **kw)["tensor"]
                                       for idx, s in subs.items()})
    diff = max(float(np.abs(r["tensor"][idx] - t).max() / np.abs(t).max()) for idx, t in alone.items())
    print(json.dumps({"config": f"block_homogenization_tensor({a.n}, {a.blocks}, {tag}, refinements={a.refinements}, tolerance={a.tolerance})",
                      **common, "blocks": nb ** a.dim, "wall_s": wall, "wall_s_one_run_per_block": wall_alone, "ratio": wall_alone / wall,
                      "cycles": r["cycles"], "residual": r["residual"], "max_rel_diff_of_a_block_tensor": diff}))
    sys.exit(0)
if a.dirichlet_tensor:
    if a.polycrystal:
        principal = (1.0, a.contrast) if a.dim == 2 else (1.0, a.contrast, a.contrast ** 0.5)
        sgrid = driver.generate_polycrystal(a.dim, a.n, a.field_seed, principal)
    else:
        sgrid = driver.generate_conductivity(a.dim, a.n, a.field_seed, values=(1.0, a.contrast))
    kw = dict(refinements=a.refinements, tolerance=a.tolerance, ctx=ctx, sigma_grid=sgrid, accelerate=a.accelerate, smoother=a.smoother,
              large_cells=a.large_cells)
    for _ in range(a.warmup):
        driver.dirichlet_homogenization_tensor(a.n, tag, **kw)
    ctx.sync()
    t0 = time.perf_counter()
    r = driver.dirichlet_homogenization_tensor(a.n, tag, **kw)
    ctx.sync()
    wall = time.perf_counter() - t0
    print(json.dumps({"config": f"dirichlet_homogenization_tensor({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance})",
                      "accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal,
                      "warmup": a.warmup, "wall_s": wall, "cycles": r["cycles"], "residual": r["residual"],
                      "cell_moments_kernel_ns": ctx.counter("cell_moments_kernel_ns"),
                      "cell_moments_download_ns": ctx.counter("cell_moments_download_ns"),
                      "cell_pair_moments_kernel_ns": ctx.counter("cell_pair_moments_kernel_ns"),
                      "cell_pair_moments_download_ns": ctx.counter("cell_pair_moments_download_ns"),
                      "large_cells": a.large_cells, "cell_moments_window_launches": ctx.counter("cell_moments_window_launches"),
                      "tensor": r["tensor"].tolist(),
                      "max_abs_diff_to_flux_form": float(np.abs(r["tensor"] - r["tensor_flux"]).max())}))
    sys.exit(0)
if a.tensor:
    kw = dict(refinements=a.refinements, tolerance=a.tolerance, ctx=ctx, sigma_grid=sgrid, seed=7, accelerate=a.accelerate,
              smoother=a.smoother)
    E = np.eye(a.dim)
    pairs = [(i, j) for i in range(a.dim) for j in range(i + 1, a.dim)]

    def tensor_run():
        tm = {}
        t0 = time.perf_counter()
        S, hist = driver.checkerboard_homogenization_tensor(a.n, tag, timings=tm, **kw)
        ctx.sync()
        return time.perf_counter() - t0, S, len(hist), tm

    def scalar_runs():
        S, cycles = np.zeros((a.dim, a.dim)), 0
        t0 = time.perf_counter()
        for i in range(a.dim):
            S[i, i], h = driver.checkerboard_homogenization(a.n, tag, xi=E[i], **kw)
            cycles += len(h)
        for i, j in pairs:
            q, h = driver.checkerboard_homogenization(a.n, tag, xi=(E[i] + E[j]) / np.sqrt(2.0), **kw)
            S[i, j] = S[j, i] = q - 0.5 * (S[i, i] + S[j, j])
            cycles += len(h)
        ctx.sync()
        return time.perf_counter() - t0, S, cycles

    for _ in range(a.warmup):
        tensor_run()
        scalar_runs()
    tt, ts = [], []
    for _ in range(a.repeats):
        t, S_t, cyc_t, tm = tensor_run()
        tt.append(t)
        t, S_s, cyc_s = scalar_runs()
        ts.append(t)
    print(json.dumps({"config": f"checkerboard_homogenization_tensor({a.n}, {tag}, refinements={a.refinements}, "
                                f"tolerance={a.tolerance})", "width": width, "accelerate": a.accelerate, "smoother": a.smoother,
                      "contrast": a.contrast, "warmup": a.warmup, "repeats": a.repeats, "scalar_runs_per_round": a.dim + len(pairs),
                      "wall_s_tensor": tt, "wall_s_scalar_runs": ts, "median_s_tensor": float(np.median(tt)),
                      "median_s_scalar_runs": float(np.median(ts)), "ratio_scalar_over_tensor": float(np.median(ts) / np.median(tt)),
                      "vcycles_tensor": cyc_t, "vcycles_scalar_runs": cyc_s, "setup_s": tm["setup_s"], "solve_s": tm["solve_s"],
                      "pair_integrals_s": tm["pair_integrals_s"], "outer_steps": tm["outer_steps"],
                      "inexact_vcycles": tm["inexact_vcycles"], "Sigma": S_t.tolist(),
                      "max_abs_diff_to_polarised": float(np.abs(S_t - S_s).max())}))
    sys.exit(0)
tm = {}
t0 = time.perf_counter()
sig, hist = driver.checkerboard_homogenization(a.n, tag, refinements=a.refinements, tolerance=a.tolerance, ctx=ctx,
                                               sigma_grid=sgrid, seed=7, timings=tm, accelerate=a.accelerate,
                                               smoother=a.smoother)
ctx.sync()
t_gpu = time.perf_counter() - t0
out = {"config": f"checkerboard_homogenization({a.n}, {tag}, refinements={a.refinements}, tolerance={a.tolerance})",
       "width": width, "sigma_gpu": sig, "vcycles": len(hist), "wall_s_gpu_incl_setup": t_gpu,
       "accelerate": a.accelerate, "smoother": a.smoother, "contrast": a.contrast, "polycrystal": a.polycrystal, "field_seed": a.field_seed, "setup_s": tm["setup_s"], "solve_s": tm["solve_s"],
       "outer_steps": tm["outer_steps"], "inexact_vcycles": tm["inexact_vcycles"]}
if not (a.no_cpu or a.accelerate or a.smoother != "cg" or a.polycrystal):
    from oracle import oracle as O
    nf = hist and None
    impl_nf = {2: [3, 6, 15, 45, 153, 561], 3: [4, 10, 35, 165, 969, 6545]}[a.dim][a.refinements]
    ne = (2 if a.dim == 2 else 6) * width ** a.dim
    x0 = hmg.host_random((impl_nf, ne), 8)               # the device path's rand(seed + 1)
    t0 = time.perf_counter()
    sig_c, hist_c = O.checkerboard_homogenization(n=a.n, dim=a.dim, refinements=a.refinements, tolerance=a.tolerance,
                                                  sigma_grid=sgrid, x0=x0, sigma_values=(1.0, a.contrast))
    out.update({"sigma_cpu": sig_c, "vcycles_cpu": len(hist_c), "wall_s_cpu": time.perf_counter() - t0,
                "cpu_threads": O.available_cores(), "abs_diff_sigma": abs(sig - sig_c)})
print(json.dumps(out))
