#!/usr/bin/env python3
"""Iterations of the level-1 PCG (hmg_coarse_solve) on the tori of 8^3 and 16^3 unit cubes: lambda = 0 -- the singular matrix,
solved on the complement of the constants -- against lambda = 1e-6 and 1e-3 -- regular, no projection --, right-hand sides with
and without a constant part, three solves each (profiles/periodic.txt).
  python tools/periodic_coarse_iterations.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
ctx = hmg.Context(0)
for n in (8, 16):
    mesh = driver.periodic_mesh(hmg.Tet64, n)
    cond = np.repeat(driver.generate_conductivity(3, n, 5).reshape(-1, 3), 6, axis=0)
    g = hmg.ImplicitFineGrid(ctx, mesh, 2)
    op = hmg.L2PlusDivAGrad(g, 0.0, cond)
    rng = np.random.default_rng(1)
    for lam in (0.0, 1e-6, 1e-3):
        op.lam = lam
        bl = hmg.BaseLevel(g)
        for const in (0.0, 5.0):
            b = hmg.DeviceMatrix(g, 1).from_host(np.asfortranarray(rng.standard_normal((4, mesh.elements.shape[0])) + const))
            x = hmg.DeviceMatrix(g, 1)
            its = []
            for _ in range(3):
                hmg._lib.check(hmg._lib.load().hmg_coarse_solve(g.h, b.h, x.h))
                its.append(bl.last_iterations())
            print(f"torus {n}^3, lambda {lam:g}, constant part {const:g}: level-1 iterations {its}", flush=True)
    g.close()
