#!/usr/bin/env python3
"""The table of DESIGN.md section 2 for the Chebyshev-Jacobi smoother, on the CPU with the oracle's own operations (no GPU):
V-cycles until the first-copy residual norm falls below 1e-8 of its start (capped at 200), and FCG iterations to the same, for
the six cases of that table -- -div(a grad u) = 1, lambda = 0, field and x0 from default_rng(3), three smoothing steps unless
the case says two -- with the smoothers "cg", "jacobi" and "chebyshev" at the ratios lambda_hi / lambda_lo in RATIOS, lambda_hi
the statement's rigorous bound (tests/_cheb_smoother_form.py).  The default ratio is the one with the fewest V-cycles in total,
the smaller one on a tie; a case that does not converge counts as the cap.

  python tools/dev/cheb_ratio_study.py [--no-fcg]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle as O                                                   # noqa: E402
from _fcg_form import fcg_local, local_problem                                   # noqa: E402
import _cheb_smoother_form as C                                                  # noqa: E402
import _pcg_smoother_form as J                                                   # noqa: E402

RATIOS = (8, 16, 30, 60, 100)
CAP = 200
CASES = [  # label, dim, n, grids, contrast, isotropic, steps
    ("3D n=4, 4 grids, sigma in {1, 9} per direction", 3, 4, 4, 9, False, 3),
    ("3D n=4, 4 grids, sigma in {1, 100} per direction", 3, 4, 4, 100, False, 3),
    ("3D n=4, 4 grids, sigma in {1, 100}, same in all directions", 3, 4, 4, 100, True, 3),
    ("3D as row 2, two smoothing steps", 3, 4, 4, 100, False, 2),
    ("2D n=8, 5 grids, sigma in {1, 9}", 2, 8, 5, 9, False, 3),
    ("2D n=8, 5 grids, sigma in {1, 100}", 2, 8, 5, 100, False, 3),
]


def problem(dim, n, grids, contrast, isotropic):
    rng = np.random.default_rng(3)
    pick = rng.random((n,) * dim + (1 if isotropic else dim,)) < 0.5
    sgrid = np.where(np.broadcast_to(pick, (n,) * dim + (dim,)), 1.0, float(contrast))
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, 0.0, sgrid)
    x0 = np.asfortranarray(rng.random(states[-1].x.shape))
    O.broadcast_interfaces(x0, implicit, grids)
    O.apply_constraint(x0, grids, constraint, implicit)
    return base, cond, implicit, constraint, ops, states, O.make_base_level(base, cond, 0.0), x0


def oracle_for(kind, ratio, implicit, ops, grids):
    if kind == "cg":
        return O
    dinvs = J.inverse_diagonals(O, implicit, ops, grids)
    if kind == "jacobi":
        return J.JacobiOracle(O, dinvs)
    return C.ChebOracle(O, dinvs, C.bounds_local(O, implicit, ops, grids, dinvs), float(ratio))


def vcycles(P, orc, steps):
    base, cond, implicit, constraint, ops, states, base_level, x0 = P
    grids, top = len(states), states[-1]
    top.x[...] = x0
    top.b.fill(0.0)
    O.local_rhs(top.b, implicit)
    start = J.first_copy_residual_norm(O, implicit, ops[-1], top, grids)
    for it in range(1, CAP + 1):
        orc.vcycle(implicit, base_level, ops, states, grids, steps)
        res = J.first_copy_residual_norm(O, implicit, ops[-1], top, grids)
        if not np.isfinite(res) or res > 1e6 * start:
            return None                                                          # diverged
        if res <= 1e-8 * start:
            return it
    return CAP + 1


def fcg_iterations(P, orc, steps):
    base, cond, implicit, constraint, ops, states, base_level, x0 = P
    grids, top = len(states), states[-1]
    b = np.zeros_like(top.b, order="F")
    O.local_rhs(b, implicit)

    def norm(x):
        top.x[...] = x
        top.b[...] = b
        return J.first_copy_residual_norm(O, implicit, ops[-1], top, grids)

    start = norm(x0)
    for it, (x, *_rest) in enumerate(fcg_local(orc, implicit, base_level, ops, states, grids, steps, x0, b), 1):
        res = norm(x)
        if not np.isfinite(res) or res > 1e6 * start:
            return None
        if res <= 1e-8 * start:
            return it
        if it >= CAP:
            return CAP + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-fcg", action="store_true")
    a = ap.parse_args()
    kinds = [("cg", None), ("jacobi", None)] + [("chebyshev", r) for r in RATIOS]
    show = lambda v: "diverged" if v is None else f">{CAP}" if v > CAP else str(v)
    total = {r: 0 for r in RATIOS}
    print("| case | " + " | ".join(k if r is None else f"cheb {r}" for k, r in kinds) + " |")
    for label, dim, n, grids, contrast, iso, steps in CASES:
        P = problem(dim, n, grids, contrast, iso)
        cells = []
        for kind, ratio in kinds:
            orc = oracle_for(kind, ratio, P[2], P[4], grids)
            v = vcycles(P, orc, steps)
            f = None if a.no_fcg else fcg_iterations(P, orc, steps)
            cells.append(show(v) + ("" if a.no_fcg else " / " + show(f)))
            if ratio is not None:
                total[ratio] += CAP + 1 if v is None else v
        print(f"| {label} | " + " | ".join(cells) + " |", flush=True)
    print("total V-cycles per ratio:", total)
    print("default ratio:", min(RATIOS, key=lambda r: (total[r], r)))


if __name__ == "__main__":
    main()
