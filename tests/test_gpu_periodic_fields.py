"""
The per-cell field kernels on a torus -- hmg_cell_moments, hmg_cell_pair_moments, hmg_cell_extrema, hmg_cell_extrema_where,
hmg_cell_histogram and the window kernels of cells larger than the LDS -- against the CPU statements of their own GPU tests.

The statements take the fine nodes' positions from the oracle's implicit grid, which knows no period.  On the torus restated
as DISJOINT SIMPLICES (tests/_periodic_form.py: every cell with d + 1 nodes of its own at its unwrapped, minimal-image corners)
that is exactly right: the per-cell kernels read one cell at a time, and the disjoint cell is the torus cell.  So each kernel is
held three ways:

  1. against the statement on the disjoint simplices, with the comparison functions and bounds of the kernel's existing test
     (imported from there, not copied);
  2. against the TWIN -- an ordinary device grid on the same disjoint simplices, the vector downloaded and uploaded --, equal bit
     for bit: kernel, level tables, element mask and column are the same, and the per-cell rows come from the same jinv
     (tests/test_periodic_host.py holds its bits on a general torus);
  3. the same bits in a second call.

The tori are general ones (nodes off the lattice, a stretched box): 3 x 3 x 3 on levels 3 and 6, 4 x 3 on levels 5 and 8, and
on level 9 through the window kernels (moments and extrema).  The vectors are torus functions with independent standard normal
values at the torus fine nodes, laid out by position (_periodic_form.fine_ids).  Not DeviceMatrix.rand followed by the interface
sum: rand draws from [0, 1), so the sum leaves a corner node -- 24 copies -- at 12 and an interior node at 0.5, a spike at every
corner whose gradients are orders above the rest; against that maximum the statements' own preconditions (no element value
within MARGIN of a threshold, slack at no more than 2 % of the (cell, edge) pairs) fail at 3D level 6 before the device is looked at.
"""
import contextlib

import numpy as np
import pytest

import homogenization_jl_amd as hmg

import _cell_extrema_form as X
import _cell_histogram_form as H
import _cell_moments_form as F
import _cell_pair_moments_form as P
import _tensor_sigma_form as T
from _periodic_form import DEN, disjoint, fine_ids, general_torus
from test_gpu_cell_extrema import check as check_extrema
from test_gpu_cell_extrema_where import check_against_statement
from test_gpu_cell_histogram import check_rows
from test_gpu_cell_moments import TOL, errs

pytestmark = pytest.mark.gpu

GRIDS = {"tet": ((3, 3, 3), 5, 6), "tri": ((4, 3), 6, 9)}               # name: shape, seed of general_torus, levels of the grid
CASES = [("tet", 3), ("tet", 6), ("tri", 5), ("tri", 8)]
LARGE = [("tri", 9)]
WINDOW_OPTIONS = ("cell_moments_windows", "cell_extrema_windows")
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def windows(ctx, level):
    """the window options at 1 around the calls on a level whose cells do not fit the LDS (2D: 9 and up), back at their values
    behind; nothing on the other levels"""
    names = WINDOW_OPTIONS if level >= 9 else ()
    prev = {n: ctx.counter(n) for n in names}
    try:
        for n in names:
            ctx.set_option(n, 1)
        yield
    finally:
        for n in names:
            ctx.set_option(n, prev[n])


class Case:
    """one (grid, level): the vectors on the torus grid and on the twin, xi, the form, and the statements -- each computed once,
    shared and never changed"""

    def __init__(self, O, mesh, impl, g, twin, level):
        self.O, self.mesh, self.impl, self.g, self.twin, self.level = O, mesh, impl, g, twin, level
        ids, n = fine_ids(g, level, DEN)                                 # the torus fine node behind every entry, by position
        self.v = np.asfortranarray(np.random.default_rng(500 + level).standard_normal(n)[ids])
        self.w = np.asfortranarray(np.random.default_rng(600 + level).standard_normal(n)[ids])
        self.dv = hmg.DeviceMatrix(g, level).from_host(self.v)
        self.dw = hmg.DeviceMatrix(g, level).from_host(self.w)
        self.tv = hmg.DeviceMatrix(twin, level).from_host(self.v)
        self.tw = hmg.DeviceMatrix(twin, level).from_host(self.w)
        rng = np.random.default_rng(700 + level)
        self.xi, self.eta = rng.standard_normal(mesh.dim), rng.standard_normal(mesh.dim)
        self.form = T.random_spd(rng, mesh.elements.shape[0], mesh.dim)
        for a in (self.v, self.w, self.xi, self.eta, self.form):
            a.setflags(write=False)
        self.vol = F.cell_volumes(O, impl.base)
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            out = make()
            for a in (out if isinstance(out, tuple) else (out,)):
                a.setflags(write=False)
            self._made[key] = out
        return self._made[key]

    def moments(self, which):
        return self.once(("moments", which), lambda: F.element_form(self.O, self.impl, self.level, self.v if which == "v" else self.w))

    def pair(self):
        return self.once("pair", lambda: P.element_form(self.O, self.impl, self.level, self.v, self.w))

    def q(self):
        grad = self.once("grad", lambda: X.element_gradients(self.O, self.impl, self.level, self.v))
        return self.once("q", lambda: X.element_values(grad, self.xi, self.form))

    def close(self):
        for d in (self.dv, self.dw, self.tv, self.tw):
            d.close()


@pytest.fixture(scope="module")
def cases(oracle, ctx):
    def get(name, level):
        O = oracle
        if name not in _cache:
            shape, seed, levels = GRIDS[name]
            mesh = general_torus(shape, seed)
            nodes, elements = disjoint(mesh)
            _cache[name] = (mesh, O.ImplicitFineGrid.create(O.Mesh(nodes, elements), levels), hmg.ImplicitFineGrid(ctx, mesh, levels),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(nodes, elements + 1), levels))
        if (name, level) not in _cache:
            _cache[(name, level)] = Case(O, *_cache[name], level)
        return _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, tuple):
            val.close()
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
            val[3].close()
    _cache.clear()


def thresholds(q):
    """four thresholds from X.gap_thresholds.  The counts are compared exactly, so no element value may lie within MARGIN (of
    the largest value) of a threshold -- asserted on the statement by test_gpu_cell_extrema.check.  Among the 5.3 million values
    of 162 cells on 3D level 6 the lower quantiles have no such gap (the values there are small against the largest, and dense: the
    widest gap near the 10 % quantile is 1.5e-9 of it, too close to the bound), so there the thresholds sit at upper quantiles."""
    if q.size > 4_000_000:
        return X.gap_thresholds(q, quantiles=(0.85, 0.95, 0.99, 0.999))
    return X.gap_thresholds(q)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.size > 0
    assert a.tobytes() == b.tobytes()


def three_ways(call, c, vectors, twin_vectors):
    """the call on the torus grid, its twin's result equal bit for bit, and the same bits in a second call"""
    got = call(*vectors, c.g)
    for a, b in zip(got, call(*twin_vectors, c.twin)):
        same_bits(a, b)
    for a, b in zip(got, call(*vectors, c.g)):
        same_bits(a, b)
    return got


@pytest.mark.parametrize("name,level", CASES + LARGE)
def test_cell_moments(ctx, cases, name, level):
    c = cases(name, level)
    n0 = ctx.counter("cell_moments_window_launches")
    with windows(ctx, level):
        mean, gram = three_ways(lambda dv, g: hmg.cell_moments(dv, g), c, (c.dv,), (c.tv,))
        mu, gu = three_ways(lambda dv, g: hmg.cell_moments(dv, g, c.xi), c, (c.dv,), (c.tv,))
    assert (ctx.counter("cell_moments_window_launches") > n0) == (level >= 9)
    want_mean, want_gram = c.moments("v")
    e1, e2 = errs(mean, gram, want_mean, want_gram)
    wm, wg = F.with_xi(want_mean, want_gram, c.vol, c.xi)
    e3, e4 = errs(mu, gu, wm, wg)
    print(f"torus {name} level {level}: mean {e1:.2e} gram {e2:.2e}; with xi mean {e3:.2e} gram {e4:.2e}")
    assert e1 <= TOL and e2 <= TOL and e3 <= TOL and e4 <= TOL
    np.testing.assert_array_equal(gram, np.swapaxes(gram, 1, 2))
    np.testing.assert_array_equal(hmg.fields.cell_volumes(c.mesh), hmg.fields.cell_volumes(c.twin.base))


@pytest.mark.parametrize("name,level", CASES + LARGE)
def test_cell_pair_moments(ctx, cases, name, level):
    c = cases(name, level)
    with windows(ctx, level):
        (S,) = three_ways(lambda dv, dw, g: (hmg.cell_pair_moments(dv, dw, g),), c, (c.dv, c.dw), (c.tv, c.tw))
        (Su,) = three_ways(lambda dv, dw, g: (hmg.cell_pair_moments(dv, dw, g, c.xi, c.eta),), c, (c.dv, c.dw), (c.tv, c.tw))
    mv, mw, pair = c.pair()
    gv, gw = c.moments("v")[1], c.moments("w")[1]
    sc = P.scale(gv, gw)
    gu, gz = F.with_xi(mv, gv, c.vol, c.xi)[1], F.with_xi(mw, gw, c.vol, c.eta)[1]
    e1 = np.abs(S - pair).max() / sc
    e2 = np.abs(Su - P.with_xi(mv, mw, pair, c.vol, c.xi, c.eta)).max() / min(sc, P.scale(gu, gz))
    print(f"torus {name} level {level}: pair {e1:.2e}; with xi_v and xi_w {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    np.testing.assert_array_equal(S, np.swapaxes(S, 1, 2))


@pytest.mark.parametrize("name,level", CASES + LARGE)
def test_cell_extrema(ctx, cases, name, level):
    c = cases(name, level)
    q = c.q()
    thr = thresholds(q)
    assert thr.shape == (4,)
    n0 = ctx.counter("cell_extrema_window_launches")
    with windows(ctx, level):
        got = three_ways(lambda dv, g: hmg.cell_extrema(dv, g, c.xi, c.form, thr), c, (c.dv,), (c.tv,))
    assert (ctx.counter("cell_extrema_window_launches") > n0) == (level >= 9)
    check_extrema(got, q, thr, f"torus {name} level {level}")          # (asserts X.margin > MARGIN on the statement first)
    assert q.shape[1] == hmg.fine_elements(c.g, level)


@pytest.mark.parametrize("name,level", CASES + LARGE)
def test_cell_extrema_where(ctx, cases, name, level):
    c = cases(name, level)
    q = c.q()
    thr = thresholds(q)
    with windows(ctx, level):
        new = three_ways(lambda dv, g: hmg.cell_extrema_where(dv, g, c.xi, c.form, thr), c, (c.dv,), (c.tv,))
        old = hmg.cell_extrema(c.dv, c.g, c.xi, c.form, thr)
    for a, b in zip(old, new[:3]):
        same_bits(a, b)
    assert new[3].dtype == new[4].dtype == np.int32
    assert new[3].shape == new[4].shape == (c.mesh.elements.shape[0], c.mesh.dim + 1)
    elements = c.impl.reference.levels[level - 1].elements
    check_against_statement(f"torus {name} level {level}", q, elements, new[3], new[4])


@pytest.mark.parametrize("name,level", CASES)
def test_cell_histogram(ctx, cases, name, level):
    c = cases(name, level)
    q = c.q()
    rule = H.quantile_rule(q)
    kw = dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])
    (counts,) = three_ways(lambda dv, g: (hmg.cell_histogram(dv, g, c.xi, c.form, **kw),), c, (c.dv,), (c.tv,))
    check_rows(counts, q, rule, hmg.fine_elements(c.g, level), f"torus {name} level {level}")
    assert (counts[:, 0] > 0).any() and (counts[:, -2] > 0).any()      # both end bins are populated
