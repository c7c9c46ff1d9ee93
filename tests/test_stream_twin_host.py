"""The CPU twins and the length ladder of tests/_stream_twin.py, without a device: the fma twin rounds once where a * x + y rounds
twice, the integer premise of the exact reductions holds at every length used, and the ladder holds every length class the
device tests (tests/test_gpu_stream_lengths.py) are meant to run -- so a later change of meshes cannot silently lose one."""
from fractions import Fraction

import numpy as np

import _stream_twin as T


def test_fma_rounds_once_where_multiply_then_add_rounds_twice():
    u = 2.0 ** -52
    # (1 + u)(1 - u) - 1 = -u^2 exactly; the product rounds to 1 first, so the two-step form gives 0
    assert T.fma1(1.0 + u, 1.0 - u, -1.0) == -u * u
    assert (1.0 + u) * (1.0 - u) + -1.0 == 0.0
    # (1 + u)^2 - (1 + 2u) = u^2
    assert T.fma1(1.0 + u, 1.0 + u, -(1.0 + 2 * u)) == u * u
    assert (1.0 + u) * (1.0 + u) + -(1.0 + 2 * u) == 0.0
    # 0.1 * 10 is 1 + 2^-54 exactly: the product rounds to 1, the fma keeps the rest
    assert T.fma1(0.1, 10.0, -1.0) == 2.0 ** -54
    assert 0.1 * 10.0 + -1.0 == 0.0
    # (2^27 + 1)^2 = 2^54 + 2^28 + 1, where doubles are 4 apart: the product loses its 1, the sum with 2 is then a tie that goes
    # to even (down); exactly it is 3 above a double and goes up
    a = 2.0 ** 27 + 1.0
    assert T.fma1(a, a, 2.0) == 2.0 ** 54 + 2.0 ** 28 + 4.0
    assert a * a + 2.0 == 2.0 ** 54 + 2.0 ** 28
    # exact cases stay exact, signs of zero aside
    assert T.fma1(3.0, -7.0, 2.0) == -19.0 and T.fma1(0.0, 5.0, 0.25) == 0.25


def test_fma_differs_from_numpy_in_a_fifth_of_random_entries():
    """default_rng(0) normals, a = 0.37: multiply-then-add differs in 4065 of 20 000 entries, by one unit in the last place."""
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(20000), rng.standard_normal(20000)
    got, two = T.axpy(0.37, x, y), 0.37 * x + y
    differ = got != two
    assert differ.sum() == 4065
    assert np.abs(got - two).max() <= np.spacing(np.abs(got)).max()
    # and against exact arithmetic the twin is within half a unit, the two-step form is not
    for i in np.flatnonzero(differ)[:50]:
        exact = Fraction(0.37) * Fraction(float(x[i])) + Fraction(float(y[i]))
        assert abs(Fraction(float(got[i])) - exact) <= abs(Fraction(float(two[i])) - exact)


def test_twins_are_the_kernels_statements():
    rng = np.random.default_rng(1)
    x, p, r = rng.standard_normal(64), rng.standard_normal(64), rng.standard_normal(64)
    np.testing.assert_array_equal(T.xpby(r, -1.7, p), T.fma(-1.7, p, r))
    ax, beta, alpha = 0.31, -0.77, 1.9
    want = [T.fma1(alpha, T.fma1(beta, pv, rv), T.fma1(ax, pv, xv)) for xv, pv, rv in zip(x, p, r)]
    np.testing.assert_array_equal(T.xupd2(ax, beta, alpha, x, p, r), want)
    assert T.fma(2.0, x.reshape(8, 8), 1.0).shape == (8, 8)
    assert np.array_equal(T.bits(np.array([0.0])), [0]) and T.bits(np.array([-0.0]))[0] != 0


def test_integer_data_sums_exactly_in_any_order():
    rng = np.random.default_rng(2)
    x, y = T.integers(rng, 4097), T.integers(rng, 4097)
    assert x.min() >= -8 and x.max() <= 8 and not (x == 0).any() and set(np.unique(np.abs(x))) == set(range(1, 9))
    want = T.int_dot(x, y)
    assert float(np.dot(x, y)) == want == float(np.dot(x[::-1], y[::-1])) == float(sum(x[i::7] @ y[i::7] for i in range(7)))
    s, sa = T.exact_dot(x, y)
    assert s == want and sa == np.abs(x * y).sum()
    assert T.int_dot(x, x) != T.int_dot(x[:-1], x[:-1])                  # a dropped entry shows
    assert T.dot_bound(4, Fraction(8)) == Fraction(32, 2 ** 53)


def test_integer_premise_holds_at_every_length_used():
    for d, l, k, c in T.ladder() + T.ladder(T.SWITCH):
        assert T.integer_sums_are_exact(c["n"]), (d, l, k)
        assert 9 * 64 * c["n"] < 2 ** 53                                 # ... and for the a = 3 update on the switch grid
    assert not T.integer_sums_are_exact(2 ** 47)


def test_length_class_arithmetic():
    c = T.length_class(3, 171)
    assert (c["n"], c["odd"], c["h"], c["hmod"], c["nb"]) == (513, 1, 256, 0, 1)
    c = T.length_class(3, 1)
    assert (c["n"], c["odd"], c["h"], c["hmod"], c["nb"]) == (3, 1, 1, 1, 1)
    c = T.length_class(1, 1)
    assert (c["n"], c["h"], c["nb"]) == (1, 0, 1)                        # no pair at all: one block, the tail thread only
    c = T.length_class(3, 342)
    assert (c["n"], c["odd"], c["hmod"], c["nb"]) == (1026, 0, 1, 3)
    c = T.length_class(165, 6355)
    assert (c["n"], c["odd"], c["hmod"], c["nb"]) == (1048575, 1, 255, 2048)
    c = T.length_class(165, 6356)
    assert (c["n"], c["odd"], c["nb"], c["nb"] % 256) == (1048740, 0, 2049, 1)


def test_ladder_holds_every_class():
    """The worked examples: which entry stands for which class, and that the meshes have the cells."""
    assert T.classes_of(3, 1) == {"a: odd, below one block"}
    assert T.classes_of(3, 170) == {"b: even, 255 pairs"}
    assert "c: odd, every pair slot full" in T.classes_of(3, 171) and "c: odd, every pair slot full" in T.classes_of(15, 239)
    assert T.length_class(15, 239)["n"] == 3585 and T.length_class(15, 239)["nb"] == 7
    assert T.classes_of(3, 342) == {"d: one live thread in the last block, even"}
    assert "d: one live thread in the last block, odd" in T.classes_of(3, 513)
    assert T.length_class(3, 513)["n"] == 1539
    assert T.classes_of(35, 47) == T.classes_of(165, 47) == {"e: pairs straddle columns, several blocks"}
    assert T.length_class(35, 47)["n"] == 1645 and T.length_class(165, 47)["n"] == 7755
    assert "f: even, every pair slot full" in T.classes_of(6, 256)
    have = T.ladder_classes()
    for name in T.REQUIRED_CLASSES:
        assert name in have, name
    for d, l, k in T.LADDER:
        width, levels = T.LADDER_MESH[d]
        assert 1 <= k <= T.mesh_cells(d, width) and 1 <= l <= levels, (d, l, k)
    assert T.mesh_cells(2, 17) == 578 and T.mesh_cells(3, 2) == 48


def test_switch_lengths_stand_on_both_sides_of_the_route_change():
    have = T.ladder_classes(T.SWITCH)
    for name in T.REQUIRED_SWITCH:
        assert name in have, name
    dim, width, level = T.SWITCH_MESH
    assert T.mesh_cells(dim, width) == 7986 and T.NF[dim][level - 1] == 165
    lo, hi, full = (c for _, _, _, c in T.ladder(T.SWITCH))
    assert lo["nb"] == T.DIRECT_BLOCKS and hi["nb"] == T.DIRECT_BLOCKS + 1
    # 2049 partials in 256 ranges of 9: ranges 228 ... 255 are empty, a fold that lost its last block would not show there
    assert -(-hi["nb"] // T.FOLD_BLOCKS) * 228 >= hi["nb"]
    assert "folded reduction whose last fold block holds partials" not in T.classes_of(165, 6356)
    assert (full["n"], full["odd"], full["nb"]) == (1179585, 1, 2304) and 9 * 255 < full["nb"] <= 9 * 256
    # the scratch of the folded route is sized from the full grid when a vector is created: entries / 512 + 2 blocks
    assert T.length_class(165, 7986)["nb"] <= 165 * 7986 // 512 + 2
