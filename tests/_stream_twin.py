"""CPU twins of the flat-pair streaming kernels (csrc/hmg_kernels.hip: k_fill ... k_cg_pupdate; csrc/hmg_fcg.hip) and the
ladder of vector lengths at which tests/test_gpu_stream_lengths.py runs them.  Checked without a device by
tests/test_stream_twin_host.py.

The kernels take one double2 per thread by flat index over the ld x ncells storage, 256 threads per block, no grid-stride loop;
thread 0 of block 0 finishes the last entry of an odd length.  With h = n >> 1 pairs a launch has nb = max(1, ceil(h / 256))
blocks; reductions leave one partial per block, finalized directly for nb <= 2048 and folded to 256 partials first above that.

Every update of those kernels is one explicit fma (axpy1 of csrc/hmg_stencil.hpp).  `fma` below is the correctly rounded
a x + y from exact rational arithmetic -- Python 3.10 has no math.fma --, so a kernel that multiplied and then added differs
from its twin in about a fifth of random entries.  Reductions are held exactly by integer data: entries from [-8, 8] without
zero make every product and every partial sum an integer far below 2^53, the same in any order and under any contraction.
"""
import math
from fractions import Fraction

import numpy as np

THREADS = 256            # per streaming block (SB of hmg_kernels.hip, FB of hmg_fcg.hip)
DIRECT_BLOCKS = 2048     # reduce_target / reduce_finish: up to this many partials are finalized directly
FOLD_BLOCKS = 256        # k_reduce_partials: block j of 256 sums the partials [j per, (j + 1) per), per = ceil(nb / 256)


# ---- one rounding per update ---------------------------------------------------------------------------------------------------
def fma1(a, x, y):
    """a x + y rounded once (float() of a Fraction rounds to nearest even)."""
    return float(Fraction(a) * Fraction(x) + Fraction(y))


def fma(a, x, y):
    """Elementwise fma1; scalars broadcast.  About 12 microseconds per entry."""
    a, x, y = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    out = np.empty(a.shape, dtype=np.float64)
    of, af, xf, yf = out.reshape(-1), a.reshape(-1).tolist(), x.reshape(-1).tolist(), y.reshape(-1).tolist()
    for i in range(len(af)):
        of[i] = fma1(af[i], xf[i], yf[i])
    return out


def axpy(a, x, y):
    """k_axpy: y = fma(a, x, y)"""
    return fma(a, x, y)


def xpby(r, b, p):
    """k_xpby, k_cg_pupdate: p = fma(b, p, r)"""
    return fma(b, p, r)


def xupd2(ax, beta, alpha, x, p, r):
    """xupd2 of csrc/hmg_stencil.hpp: (x + ax p) + alpha (r + beta p), three roundings in the kernels' order"""
    t1 = fma(ax, p, x)
    p2 = fma(beta, p, r)
    return fma(alpha, p2, t1)


def bits(a):
    """the bit patterns of an array of doubles, for comparisons that tell -0.0 from 0.0 and one NaN from another"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- exact reductions ----------------------------------------------------------------------------------------------------------
INT_BOUND = 8            # integer entries lie in [-8, 8] \ {0}: a product is at most 64 in magnitude


def integers(rng, shape):
    """Integer-valued doubles from [-8, 8] without zero (a dropped entry always changes a sum of squares)."""
    v = rng.integers(1, INT_BOUND + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return v.astype(np.float64)


def integer_sums_are_exact(n):
    """The premise of the exact reductions: n products of magnitude <= 64 cannot leave the integers a double holds."""
    return INT_BOUND * INT_BOUND * n < 2 ** 53


def int_dot(x, y):
    """Python's integer sum of the products of two integer-valued arrays"""
    xi, yi = np.asarray(x).reshape(-1).astype(np.int64), np.asarray(y).reshape(-1).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x).reshape(-1)) and np.array_equal(yi, np.asarray(y).reshape(-1)), "not integer data"
    return sum(int(a) * int(b) for a, b in zip(xi.tolist(), yi.tolist()))


def exact_dot(x, y):
    """(sum x_i y_i, sum |x_i y_i|) as Fractions"""
    s, sa = Fraction(0), Fraction(0)
    for a, b in zip(np.asarray(x).reshape(-1).tolist(), np.asarray(y).reshape(-1).tolist()):
        t = Fraction(a) * Fraction(b)
        s += t
        sa += abs(t)
    return s, sa


def dot_bound(n, sum_abs):
    """n u sum |x_i y_i|, u = 2^-53: what recursive summation in ANY order, with or without contracted products, stays within
    to first order (Higham, Accuracy and Stability of Numerical Algorithms, (3.5): gamma_n sum |x_i y_i|); nothing measured."""
    return Fraction(n, 2 ** 53) * sum_abs


# ---- the lengths ---------------------------------------------------------------------------------------------------------------
def length_class(ld, cells):
    """(ld, cells) -> the quantities the launch shape depends on"""
    n = ld * cells
    h = n >> 1
    return {"ld": ld, "cells": cells, "n": n, "odd": n & 1, "h": h, "hmod": h % THREADS, "nb": max(1, -(-h // THREADS))}


def classes_of(ld, cells):
    """Names of the length classes (ld, cells) belongs to."""
    c = length_class(ld, cells)
    n, h, nb, out = c["n"], c["h"], c["nb"], set()
    if c["odd"] and nb == 1 and h < THREADS:
        out.add("a: odd, below one block")
    if not c["odd"] and h == THREADS - 1:
        out.add("b: even, 255 pairs")
    if c["odd"] and h > 0 and c["hmod"] == 0:
        out.add("c: odd, every pair slot full")
    if h > THREADS and c["hmod"] == 1:
        out.add("d: one live thread in the last block, " + ("odd" if c["odd"] else "even"))
    if c["odd"] and ld & 1 and ld > 1 and nb > 1 and cells > 1:
        out.add("e: pairs straddle columns, several blocks")
    if not c["odd"] and h > 0 and c["hmod"] == 0:
        out.add("f: even, every pair slot full")
    if nb == DIRECT_BLOCKS:
        out.add("last length of the direct reduction" + (", odd, 255 pairs in the last block" if c["odd"] and c["hmod"] == 255 else ""))
    if nb == DIRECT_BLOCKS + 1:
        out.add("first length of the folded reduction" + (", blocks no multiple of 256" if nb % 256 else ""))
    if nb > DIRECT_BLOCKS and -(-nb // FOLD_BLOCKS) * (FOLD_BLOCKS - 1) < nb:
        out.add("folded reduction whose last fold block holds partials")
    return out


REQUIRED_CLASSES = ("a: odd, below one block", "b: even, 255 pairs", "c: odd, every pair slot full",
                    "d: one live thread in the last block, even", "d: one live thread in the last block, odd",
                    "e: pairs straddle columns, several blocks")
REQUIRED_SWITCH = ("last length of the direct reduction, odd, 255 pairs in the last block",
                   "first length of the folded reduction, blocks no multiple of 256",
                   "folded reduction whose last fold block holds partials")

NF = {2: [3, 6, 15, 45, 153, 561], 3: [4, 10, 35, 165, 969, 6545]}     # nodes of a cell, level 1 ...

# One grid per dimension, created at full size and shrunk to every prefix in turn (hmg_grid_shrink takes any prefix of the full
# mesh).  2D: 17 x 17 squares, 578 triangles, three levels.  3D: 2 x 2 x 2 cubes, 48 tetrahedra, four levels.
LADDER_MESH = {2: (17, 3), 3: (2, 4)}                                   # dim -> (cubes per axis, levels)
LADDER = (   # (dim, level, cells)
    (2, 1, 1), (2, 1, 2), (2, 1, 170), (2, 1, 171), (2, 3, 239), (2, 1, 342), (2, 1, 513), (2, 2, 256), (2, 3, 578),
    (3, 3, 47), (3, 4, 47), (3, 4, 48),
)
# The two reduction routes: 3D level 4 on 11 x 11 x 11 cubes (7986 cells).  At 2049 blocks the fold gives each of its 256 blocks 9
# partials, so only the first 228 hold any; at 7149 cells (2304 blocks, n odd) all 256 do, the last one the partials of the
# vector's end.
SWITCH_MESH = (3, 11, 4)                                                 # dim, cubes per axis, level (= levels)
SWITCH = ((3, 4, 6355), (3, 4, 6356), (3, 4, 7149))


def mesh_cells(dim, width):
    return width ** dim * (2 if dim == 2 else 6)


def ladder(entries=LADDER):
    """[(dim, level, cells, length_class)] of the entries"""
    return [(d, l, k, length_class(NF[d][l - 1], k)) for d, l, k in entries]


def ladder_classes(entries=LADDER):
    out = set()
    for d, l, k in entries:
        out |= classes_of(NF[d][l - 1], k)
    return out
