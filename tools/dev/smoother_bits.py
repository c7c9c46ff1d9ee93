#!/usr/bin/env python3
"""Do two builds of the library smooth to the same bits?  One SHA-256 per case over x, r and the 16 doubles of the scalar bank, from
seeded data.  Run once per build (HMG_LIB_PATH selects the library, HMG_LIB_AB=1 for an older one) and compare the outputs.

Grids: 2^3 cubes x 6 tetrahedra (48 cells) with top levels 3, 5 and 6, the level-6 grid shrunk to 47 cells (odd entry count: the
kernels' tail branches), 4^2 squares x 2 triangles with top level 5.  Over them: 1, 2 and 3 smoothing steps; the CG, Jacobi-CG and
Chebyshev smoothers; fuse_cg on and off; three V-cycles with x unread and with x read after each; hmg_smooth alone; hmg_vcycle_down
followed by hmg_vcycle_up; two hmg_fcg_steps.  The counters say that the deferred forms were taken where they should be."""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: the process holds one HIP runtime, torch's)
import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib, driver

GRIDS = (("tet n=2 L3", "Tet64", 2, 3, None), ("tet n=2 L5", "Tet64", 2, 5, None), ("tet n=2 L6", "Tet64", 2, 6, None),
         ("tet n=2 L6 47 cells", "Tet64", 2, 6, 47), ("tri n=4 L5", "Tri64", 4, 5, None))
SMOOTHERS = ("cg", "jacobi", "chebyshev")
OPS = ("vcycles", "vcycles_read", "smooth", "down_up", "fcg")
FORMS = ("lazy_x_form", "lazy_pre_form", "lazy_ap_form")

ctx = hmg.Context(0)
bank = torch.zeros(16, dtype=torch.float64, device="cuda:0")
_lib.check(_lib.load().hmg_ctx_set_scalar_bank(ctx.h, ctypes.c_void_p(bank.data_ptr())))


def start(g, levels):
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(3)
    st[-1].b.rand(4)
    hmg.broadcast_interfaces(st[-1].x, g, levels)
    hmg.apply_constraint(st[-1].x, levels, g)
    return st


def close(st):
    for s in st:
        s.close()


def run(g, bl, op, levels, steps, what):
    """the bytes a caller can observe behind `what`, and the counters read before anything was observed"""
    ops = [op] * levels
    # (the grid remembers whether the last cycle's x and r were read and finishes them at once if so: two cycles nobody reads, on
    #  states that go unread too, clear both memories)
    st = start(g, levels)
    for _ in range(2):
        hmg.vcycle(g, bl, ops, st, levels, steps, 2)
    close(st)
    st = start(g, levels)
    seen, extra = [], None
    if what in ("vcycles", "vcycles_read"):
        for _ in range(3):
            hmg.vcycle(g, bl, ops, st, levels, steps, 2)
            if what == "vcycles_read":
                seen.append(st[-1].x.to_host())
    elif what == "smooth":
        hmg.smoothing_steps(steps, g, op, st[-1], levels)
        extra = (st[-1].p, st[-1].Ap)
    elif what == "down_up":
        hmg.vcycle_down(g, ops, st, levels, steps)
        hmg.vcycle_up(g, ops, st, levels, steps)
        extra = (st[-2].b,)
    else:
        x = hmg.DeviceMatrix(g, levels)
        x.copyto(st[-1].x)
        fcg = hmg.FlexibleCG(g, bl, ops, st, levels, steps, 2).start(x, st[-1].b)
        fcg.step()
        fcg.step()
        seen += [x.to_host(), fcg.vec("R")]
        fcg.close()
        x.close()
    counters = {n: ctx.counter(n) for n in FORMS}
    ctx.sync()
    seen.append(bank.cpu().numpy())                      # ... as the last launch left it, then as the reads that settle leave it
    seen += [st[-1].x.to_host(), st[-1].r.to_host()] + [v.to_host() for v in extra or ()]
    ctx.sync()
    seen.append(bank.cpu().numpy())
    close(st)
    h = hashlib.sha256()
    for a in seen:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest(), counters


for fused in (1, 0):
    ctx.set_option("fuse_cg", fused)                     # (read when a grid is created)
    for name, tag, width, levels, cells in GRIDS:
        base, cond, g, op = driver.checkerboard_problem(ctx, getattr(hmg, tag), width, levels, seed=17, lam=0.8)
        if cells is not None:
            g.shrink(cells, g.nnodes_base())
            assert g.ncells() == cells
        bl = hmg.BaseLevel(g)
        for smoother in SMOOTHERS:
            g.set_smoother(smoother)
            for steps in (1, 2, 3):
                for what in OPS:
                    folds, reads = ctx.counter("coarse_x_folds"), ctx.counter("x_settled_read")
                    digest, counters = run(g, bl, op, levels, steps, what)
                    if (name, smoother, fused, steps) == ("tet n=2 L6", "cg", 1, 3) and what.startswith("vcycles"):
                        # (so that equal hashes cannot come from both builds missing the deferred paths)
                        assert ctx.counter("coarse_x_folds") > folds
                        assert counters["lazy_pre_form"] == 3, counters
                        if what == "vcycles":
                            assert counters["lazy_x_form"] == 3 and counters["lazy_ap_form"] == 1, counters
                        else:
                            assert ctx.counter("x_settled_read") > reads
                    print(f"{name:20s} {smoother:9s} fuse_cg={fused} steps={steps} {what:12s} {digest}", flush=True)
        g.close()
ctx.set_option("fuse_cg", 1)
