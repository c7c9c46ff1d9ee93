#!/usr/bin/env python3
"""Budgeted level-1 solves that ran out of their blind iteration budget (hmg_coarse_misses, api.BaseLevel.misses) during a
corrector solve to 1e-12: the torus -- singular level-1 matrix, solved on the complement of the constants -- against the box of the
same cubes with its Dirichlet boundary, on a laminate and on a seeded checkerboard, 2D (n = 4) and 3D (n = 3), 2 refinements,
every direction.
  python tools/periodic_coarse_misses.py"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

ctx = hmg.Context(0)
warnings.simplefilter("ignore")
for dim, n in ((2, 4), (3, 3)):
    tag = hmg.Tet64 if dim == 3 else hmg.Tri64
    layers = np.array([1.0, 9.0, 3.0, 0.5][:n])[:, None] * np.array([1.0, 2.0, 0.25][:dim])[None, :]
    fields = {"laminate": np.broadcast_to(layers.reshape((n,) + (1,) * (dim - 1) + (dim,)), (n,) * dim + (dim,)).copy(),
              "checkerboard": driver.generate_conductivity(dim, n, 5)}
    for name, sgrid in fields.items():
        for kind in ("torus", "box"):
            if kind == "torus":
                base = driver.periodic_mesh(tag, n)
                cond = np.repeat(sgrid.reshape(-1, dim), base.elements.shape[0] // n ** dim, axis=0)
            else:
                base = driver.hypercube(tag, n)
                cond = driver.conductivity_per_element(base, sgrid, (0.0,) * dim)
            g = hmg.ImplicitFineGrid(ctx, base, 3)
            op = hmg.L2PlusDivAGrad(g, 0.0, cond)
            bl = hmg.BaseLevel(g)
            st = [hmg.LevelState(g, i + 1) for i in range(3)]
            cycles = [driver._dirichlet_solve(g, op, bl, st, st[-1].x, None, np.eye(dim)[k], 3, 1e-12, 200, "")[0] for k in range(dim)]
            print(f"{dim}D n = {n}, {name}, {kind}: V-cycles {cycles}, level-1 solves that missed their budget {bl.misses()}", flush=True)
            for s in st:
                s.close()
            g.close()
