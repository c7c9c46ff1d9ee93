#!/usr/bin/env python3
"""The outputs of hmg_cell_moments and hmg_cell_pair_moments as bits, to compare two builds of the library (HMG_LIB_PATH):
  python tools/dev/cell_moments_bits.py dump a.npz          (once per build, each in a fresh process)
  python tools/dev/cell_moments_bits.py compare a.npz b.npz [--out report.txt]
Grids and vectors are those of tests/test_gpu_cell_moments_window.py (fixed seeds): cube7 levels 3, 5, 6, 7; square9 levels 2, 3,
4, 8, 9; square10 level 10; square11 level 11; with and without xi; the context option "cell_moments_windows" at 0, 1 and 2 (0 only
where the level fits the LDS).  Per case: mean and gram of v, pair(v, w), pair(v, v).  compare: numpy.array_equal of every array."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OPT = "cell_moments_windows"
GRIDS = {"cube7": (3, 1, 7, (3, 5, 6, 7)), "square9": (2, 2, 9, (2, 3, 4, 8, 9)), "square10": (2, 1, 10, (10,)),
         "square11": (2, 1, 11, (11,))}


def dump(path):
    import homogenization_jl_amd as hmg
    from oracle import oracle as O
    import _cell_moments_form as F
    O.lib()
    ctx = hmg.Context(0)
    out = {}
    for name, (dim, n, grids, levels) in GRIDS.items():
        base = O.hypercube(dim, n)
        base.nodes = base.nodes + 0.2 * (np.random.default_rng(5).random(base.nodes.shape) - 0.5)
        implicit = O.ImplicitFineGrid.create(base, grids)
        g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids)
        xv, xw = np.array([0.6, -0.3, 0.5])[:dim], np.array([-0.2, 0.9, 0.4])[:dim]
        for level in levels:
            dv = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(100 + level)))
            dw = hmg.DeviceMatrix(g, level).from_host(F.consistent_random(O, implicit, level, np.random.default_rng(200 + level)))
            large = level > (6 if dim == 3 else 8)
            for value in ((1, 2) if large else (0, 1, 2)):
                ctx.set_option(OPT, value)
                for tag, a, b in (("", None, None), (" xi", xv, xw)):
                    key = f"{name} level {level} option {value}{tag}: "
                    out[key + "mean"], out[key + "gram"] = hmg.cell_moments(dv, g, a)
                    out[key + "pair(v, w)"] = hmg.cell_pair_moments(dv, dw, g, a, b)
                    out[key + "pair(v, v)"] = hmg.cell_pair_moments(dv, dv, g, a, b)
            ctx.set_option(OPT, 0)
            dv.close()
            dw.close()
        g.close()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(pa, pb, report):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    lines = [f"{k:<50} {str(a[k].shape):<14} {'equal' if np.array_equal(a[k], b[k]) else 'DIFFERENT'}" for k in a.files]
    bad = sum(line.endswith("DIFFERENT") for line in lines)
    lines.append(f"{len(lines)} arrays compared with numpy.array_equal: " + ("every array is equal" if bad == 0 else f"{bad} DIFFER"))
    print("\n".join(lines))
    if report:
        with open(report, "w") as f:
            f.write("\n".join(lines) + "\n")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3], sys.argv[5] if sys.argv[4:5] == ["--out"] else None) else 0)
