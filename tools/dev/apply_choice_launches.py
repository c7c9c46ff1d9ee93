#!/usr/bin/env python3
"""Which kernel every operator apply takes, on small grids that reach every branch of the choice (csrc/hmg_apply.hip: apply_family,
apply_cell_shape, apply_cell_role).  Run one section under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 THIS SECTION`
(the trace alone, no counters), then `python3 THIS --list DIR/.../*kernel_trace.csv` prints the launches in order: kernel with its
template arguments, grid, workgroup, LDS bytes.  Two builds launch the same kernels if the two lists are the same text
(HMG_LIB_PATH selects the build).

Sections: cycles  -- 3D, 2 cubes per axis, 6 levels: V-cycles by default and with each A/B option off, the Jacobi smoother, integrals
          threads -- a plain apply and a residual on levels 3..6 for every apply_threads
          deep    -- 3D 7 levels and 2D 9 levels (cells larger than the LDS) on one and on two cubes / squares per axis, 2D 5 levels"""
import csv, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def list_trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = next(k for k in rows[0] if "LDS" in k.upper())
    for r in rows:
        print(f"{r['Kernel_Name']} | grid {r['Grid_Size_X']} | wg {r['Workgroup_Size_X']} | lds {r[lds]}")


if len(sys.argv) == 3 and sys.argv[1] == "--list":
    list_trace(sys.argv[2])
    sys.exit(0)

import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

section = sys.argv[1]
ctx = hmg.Context(0)


def problem(eltype, width, levels, smoother="cg", base_level=True):
    base, cond, g, op = driver.checkerboard_problem(ctx, eltype, width, levels, seed=0)
    if smoother != "cg":
        g.set_smoother(smoother)
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(1)
    st[-1].b.rand(2)
    return g, op, st, hmg.BaseLevel(g) if base_level else None


def cycles(g, op, st, bl, plan):
    for steps, steps_coarse in plan:
        hmg.vcycle(g, bl, [op] * len(st), st, len(st), steps, steps_coarse)
    ctx.sync()


def integrals(g, st):
    v, w = st[-1].x, st[-1].b
    xi = np.ones(g.base.dim)
    hmg.integrate_first_term(v, g, g.ncells(), xi)     # mode 0
    hmg.integrate_terms(v, w, g, g.ncells())           # mode 1
    hmg.integrate_pair_mass(v, w, g, g.ncells())       # mode 3
    ctx.sync()


PLAN = [(3, 2), (3, 2), (2, 2), (2, 2)]
if section == "cycles":
    g, op, st, bl = problem(hmg.Tet64, 2, 6)
    cycles(g, op, st, bl, PLAN)
    for option in ("weight_cache", "apply_wg512", "apply_wave", "apply_small", "fuse_cg"):
        ctx.set_option(option, 0)
        cycles(g, op, st, bl, PLAN)
        ctx.set_option(option, 1)
    integrals(g, st)
    g, op, st, bl = problem(hmg.Tet64, 2, 6, smoother="jacobi")
    cycles(g, op, st, bl, PLAN)
elif section == "threads":
    g, op, st, bl = problem(hmg.Tet64, 2, 6)
    for threads in (64, 192, 256, 512, 640, 1024):
        ctx.set_option("apply_threads", threads)
        for level in (3, 4, 5, 6):
            s = st[level - 1]
            s.x.rand(3)
            s.b.rand(4)
            hmg.mul(1.0, g, op, s.x, s.r)
            hmg.local_residual(g, op, s, level)
        ctx.sync()
    ctx.set_option("apply_threads", 0)
elif section == "deep":
    # (a base mesh of one cube / two triangles has no interior node, so no level-1 system and no V-cycle: it gets the smoother, the
    #  restriction and the integrals; the V-cycles run on two cubes / squares per axis)
    for eltype, levels in ((hmg.Tet64, 7), (hmg.Tri64, 9)):
        g, op, st, bl = problem(eltype, 1, levels, base_level=False)
        hmg.smoothing_steps(3, g, op, st[-1], levels)
        hmg.local_residual(g, op, st[-1], levels)
        hmg.restrict_to(st[-2].b, g, st[-1].r)
        integrals(g, st)
        g, op, st, bl = problem(eltype, 2, levels)
        cycles(g, op, st, bl, [(3, 2)])
        hmg.restrict_to(st[-2].b, g, st[-1].r)
        integrals(g, st)
    g, op, st, bl = problem(hmg.Tri64, 2, 5)
    cycles(g, op, st, bl, [(3, 2)])
else:
    sys.exit(f"unknown section {section!r}")
ctx.sync()
print(f"{section}: done")
