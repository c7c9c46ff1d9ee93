"""GPU tests of the per-cell histograms of cells larger than the LDS (context option "cell_histogram_windows",
csrc/hmg_histogram_window.hip: k_cell_histogram_slab for 3D level 7, k_cell_histogram_rows for 2D levels 9-11) against the CPU
statement of tests/_cell_histogram_form.py and, exactly, against the extrema window kernels' threshold counts.

Grids and inputs are those of tests/test_gpu_cell_extrema_window.py -- the smallest with several slabs / bands, X.perturbed_cube:
(3, 1) on level 7 (6 cells, 9 slabs), (2, 2) on level 9 (8 cells), (2, 1) on levels 10 and 11 (2 cells; level 11: rows of 1 025
nodes, wider than the workgroup); consistent_random with default_rng(300 + level), a random xi, T.random_spd, the rule from
H.quantile_rule(q).  The same grids carry the levels of the kernel-against-kernel check of option value 2: 3D level 6 (one slab),
2D levels 2 (m = 2: no interior), 3, 4 and 8 (a single band).

Against the statement (check_rows of tests/test_gpu_cell_histogram.py with the margin as an argument): with delta relative to
max|q| every cell and every edge E must have  #(q >= E + delta) <= tail <= #(q >= E - delta)  -- after the assertion, on the
statement alone, that at most 2 % of the (cell, edge) pairs have any slack between the two counts.  delta = 1e-9 max|q| (the
project's MARGIN) for cube7 and square9; delta = 1e-10 max|q| for square10 and square11: at 1e-9 the 2 % cap fails on the statement
alone there (3 of 146 and 5 of 130 pairs, measured on the CPU with exactly these inputs), because 1e-9 times the 10^6 elements of a
cell is no longer small.  1e-10 is still ten times the device's 1e-11 bound and 200 times the 4.4e-13 by which the two CPU
transcriptions of the statement differ (tests/test_gpu_cell_extrema_window.py).
Against the extrema: for a q that is no NaN and a finite positive edge E, q >= E <=> q > nextafter(E, -inf), so the tails at eight
edges EQUAL cell_extrema's counts (taken with "cell_extrema_windows" = 1) for those predecessors as thresholds.
Where two kernels serve one level -- option 2 against option 0 -- every count is equal.
The context is this module's own; the option is at its default 0 between the tests."""
import contextlib

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist
from homogenization_jl_amd import driver, fields
import _cell_extrema_form as X
import _cell_histogram_form as H
import _cell_moments_form as F
import _tensor_sigma_form as T
from _periodic_form import disjoint

pytestmark = pytest.mark.gpu
SLACK_PAIRS = 0.02
OPT, COUNTER = "cell_histogram_windows", "cell_histogram_window_launches"
XOPT = "cell_extrema_windows"
# name: dim, n, finest level
GRIDS = {"cube7": (3, 1, 7), "square9": (2, 2, 9), "square10": (2, 1, 10), "square11": (2, 1, 11)}
LARGE = [("cube7", 7), ("square9", 9), ("square10", 10), ("square11", 11)]
FITTING = [("cube7", 6), ("square9", 2), ("square9", 3), ("square9", 4), ("square9", 8)]
MARGINS = {"cube7": 1e-9, "square9": 1e-9, "square10": 1e-10, "square11": 1e-10}
WIDEST = 1027
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    assert c.counter(OPT) == 0
    yield c
    assert c.counter(OPT) == 0 and c.counter(XOPT) == 0
    c.close()


@contextlib.contextmanager
def option(ctx, value, name=OPT):
    prev = ctx.counter(name)
    ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, prev)


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per grid: perturbed oracle mesh, implicit grid, device grid; per (grid, level): a consistent random vector, xi, an SPD form;
    per (grid, level, "q"): the statement's element values -- computed once, shared, never changed"""
    def get(name, level, values=False):
        O = oracle
        if name not in _cache:
            dim, n, grids = GRIDS[name]
            base = X.perturbed_cube(O, dim, n)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            rng = np.random.default_rng(300 + level)
            v = F.consistent_random(O, implicit, level, rng)
            xi = rng.standard_normal(base.dim)
            form = T.random_spd(rng, base.nelements(), base.dim)
            for a in (v, xi, form):
                a.setflags(write=False)
            _cache[(name, level)] = (v, xi, form)
        out = (base, implicit, g) + _cache[(name, level)]
        if values:
            if (name, level, "q") not in _cache:
                gr = X.element_gradients(O, implicit, level, out[3])
                gr.setflags(write=False)
                q = X.element_values(gr, out[4], out[5])
                q.setflags(write=False)
                _cache[(name, level, "q")] = (gr, q)
            out += _cache[(name, level, "q")]
        return out
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def kw(rule):
    return dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])


def widest_rule(rule):
    """1 027 bins (32 octaves in 32 sub-bins each: the largest LDS) around the middle of `rule`"""
    mid = (rule[0] + rule[1]) // 2
    out = (mid - 16, mid + 16, 5)
    assert H.nbins(*out) == WIDEST
    return out


def check_rows(counts, q, rule, nel, margin, what):
    """counts (Ne, nbins) of the device against the statement's element values q (Ne, nt) under the rule (emin, emax, sub_bits)"""
    E = H.edges(*rule)
    with np.errstate(invalid="ignore"):
        delta = margin * np.nanmax(np.abs(q))
        lower, upper = H.tail_bounds(q, E, delta)
    slack = int((lower != upper).sum())
    print(f"{what}: rule {rule}, delta {margin:g} max|q|, {slack} of {lower.size} (cell, edge) pairs have slack")
    assert slack <= SLACK_PAIRS * lower.size                           # (on the statement alone)
    assert counts.shape == (q.shape[0], H.nbins(*rule)) and counts.dtype == np.int64
    assert q.shape[1] == nel
    np.testing.assert_array_equal(counts.sum(axis=1), nel)
    assert (counts >= 0).all()
    tail = H.tail(counts)
    np.testing.assert_array_equal(tail, fields.histogram_tail(counts))
    bad = int(((tail < lower) | (tail > upper)).sum())
    with np.errstate(invalid="ignore"):
        exact = int((counts != H.cell_counts(q, E)).sum())
    print(f"{what}: {bad} tails outside their interval; {exact} of {counts.size} counts differ from the statement's own")
    assert bad == 0


def check_against_extrema(ctx, g, dv, xi, form, counts, rule, what):
    """the tails at eight edges spread over the range EQUAL hmg_cell_extrema's counts for the edges' predecessors, taken through
    the extrema window kernels where the level needs them"""
    E = H.edges(*rule)
    idx = np.unique(np.rint(np.linspace(0, len(E) - 1, 8)).astype(int))
    thr = np.nextafter(E[idx], -np.inf)
    with option(ctx, 1, XOPT):
        _, _, want = hmg.cell_extrema(dv, g, xi, form, thr)
    got = H.tail(counts)[:, idx]
    print(f"{what}: {int((got != want).sum())} of {got.size} tails differ from cell_extrema's counts at {len(idx)} edges")
    np.testing.assert_array_equal(got, want)


def rule_around_the_peaks(ctx, g, dv, xi, form):
    """13 octaves in 8 sub-bins each, up to the octave of the median of the cells' maxima (hmg_cell_extrema through its window
    kernels): a rule that resolves the values without the statement"""
    with option(ctx, 1, XOPT):
        qmax, _, _ = hmg.cell_extrema(dv, g, xi, form)
    top = int(np.ceil(np.log2(np.median(qmax))))
    return (top - 13, top, 3)


# ---- option 1 against the statement ----

@pytest.mark.parametrize("name,level", LARGE)
def test_device_against_the_statement(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad, q = shapes(name, level, values=True)
    nel = hmg.fine_elements(g, level)
    rule = H.quantile_rule(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with option(ctx, 1):
        n0, l0 = ctx.counter(COUNTER), ctx.counter("cell_histogram_launches")
        counts = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
        assert ctx.counter(COUNTER) == n0 + 1 and ctx.counter("cell_histogram_launches") == l0 + 1
        assert ctx.counter("cell_histogram_kernel_ns") > 0
        check_rows(counts, q, rule, nel, MARGINS[name], f"{name} level {level}")
        assert (counts[:, -1] == 0).all()                                  # no NaN
        assert (counts[:, 0] > 0).any() and (counts[:, -2] > 0).any()      # both end bins are populated
        # the same ints in a second run, and no allocation in it
        a0 = ctx.counter("device_allocs")
        np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, **kw(rule)), counts)
        assert ctx.counter("device_allocs") == a0
        assert ctx.counter(COUNTER) == n0 + 2
    dv.close()


# ---- exact, against the extrema window kernels ----

@pytest.mark.parametrize("name,level", LARGE)
def test_tails_equal_the_extrema_window_counts(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad, q = shapes(name, level, values=True)
    nel = hmg.fine_elements(g, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    small = H.quantile_rule(q)
    for rule in (small, widest_rule(small)):
        with option(ctx, 1):
            counts = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
        assert counts.shape == (base.nelements(), H.nbins(*rule))
        np.testing.assert_array_equal(counts.sum(axis=1), nel)
        check_against_extrema(ctx, g, dv, xi, form, counts, rule, f"{name} level {level} rule {rule}")
    assert counts.shape[1] == WIDEST and (counts[:, 1:-2] > 0).sum() > 4 * base.nelements()   # (the widest rule resolves something)
    dv.close()


# ---- two kernels on one level: the same ints ----

@pytest.mark.parametrize("name,level", FITTING)
def test_window_kernels_give_the_counts_of_the_lds_kernel(ctx, shapes, name, level):
    """option value 2 sends a level that fits the LDS through the window kernels; value 1 leaves it to k_cell_histogram"""
    base, implicit, g, v, xi, form = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    qmax, qmin, _ = hmg.cell_extrema(dv, g, xi, form)
    small = (int(np.floor(np.log2(np.median(qmin)))), int(np.ceil(np.log2(np.median(qmax)))), 3)
    assert small[0] < small[1]
    res, launches = [], []
    for value in (0, 1, 2):
        with option(ctx, value):
            n0 = ctx.counter(COUNTER)
            res.append((hmg.cell_histogram(dv, g, xi, form, **kw(small)), hmg.cell_histogram(dv, g, xi, form, **kw(widest_rule(small))),
                        hmg.cell_histogram(dv, g, None, None, **kw(small))))
            launches.append(ctx.counter(COUNTER) - n0)
    print(f"{name} level {level}: window launches at option 0, 1, 2: {launches}; occupied bins at option 0 "
          f"{[int((r.sum(axis=0) > 0).sum()) for r in res[0]]}")
    assert launches == [0, 0, 3]
    assert (res[0][0].sum(axis=0) > 0).sum() > 2 and res[0][1].shape[1] == WIDEST
    for a0, a1, a2 in zip(*res):
        np.testing.assert_array_equal(a0.sum(axis=1), hmg.fine_elements(g, level))
        np.testing.assert_array_equal(a0, a1)
        np.testing.assert_array_equal(a0, a2)
    dv.close()


# ---- edge data ----

EDGE = [("cube7", 7), ("square9", 9)]


@pytest.mark.parametrize("name,level", EDGE)
def test_zero_vector(ctx, shapes, name, level):
    base, implicit, g, v, xi, form = shapes(name, level)
    d, nel = base.dim, hmg.fine_elements(g, level)
    dv = hmg.DeviceMatrix(g, level)                                   # zero-filled
    with option(ctx, 1):
        counts = hmg.cell_histogram(dv, g, emin=-8, emax=8)
        assert (counts[:, 0] == nel).all() and (counts[:, 1:] == 0).all()   # q = 0 everywhere: below every edge
        # a xi whose |xi|^2 sits in the middle of a bin, identity form: the whole cell in that one bin (every lane of every wave
        # adds to the same address)
        E = H.edges(-2, 2, 3)
        target = 0.5 * (E[17] + E[18])
        xi1 = np.full(d, np.sqrt(target / d))
        b = int(H.bins(np.array([xi1 @ xi1]), E)[0])
        assert b == 18 and E[17] * (1 + 1e-3) < xi1 @ xi1 < E[18] * (1 - 1e-3)
        counts = hmg.cell_histogram(dv, g, xi1, emin=-2, emax=2, sub_bits=3)
        want = np.zeros_like(counts)
        want[:, b] = nel
        np.testing.assert_array_equal(counts, want)
        # ... and a form per cell: each cell's elements in the one bin of its own constant value xi . Q_c xi (values within 1e-3
        # of an edge are moved off it by scaling the cell's form)
        E = H.edges(-6, 10, 3)
        qc = np.einsum("k,ekl,l->e", xi, form, xi)
        near = np.abs(qc[:, None] / E[None, :] - 1.0).min(axis=1) < 1e-3
        scaled = np.where(near[:, None, None], form * 1.01, form)
        qc = np.einsum("k,ekl,l->e", xi, scaled, xi)
        assert (np.abs(qc[:, None] / E[None, :] - 1.0).min(axis=1) > 1e-3).all() and E[0] < qc.min() and qc.max() < E[-1]
        counts = hmg.cell_histogram(dv, g, xi, scaled, emin=-6, emax=10, sub_bits=3)
        want = np.zeros_like(counts)
        want[np.arange(qc.size), H.bins(qc, E)] = nel
        np.testing.assert_array_equal(counts, want)
    dv.close()


@pytest.mark.parametrize("name,level", EDGE)
def test_indefinite_form(ctx, shapes, name, level):
    """negative values land in the below-range bin; the tails are still the extrema window kernels'"""
    base, implicit, g, v, xi, form, grad, _ = shapes(name, level, values=True)
    d = base.dim
    Q = form - np.einsum("ekk->e", form)[:, None, None] / d * np.eye(d)[None]
    Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
    q = X.element_values(grad, xi, Q)
    assert q.min() < 0.0 < q.max()
    rule = H.quantile_rule(q[q > 0.0])
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with option(ctx, 1):
        counts = hmg.cell_histogram(dv, g, xi, Q, **kw(rule))
    check_rows(counts, q, rule, hmg.fine_elements(g, level), MARGINS[name], f"{name} level {level} indefinite form")
    below = (q < -MARGINS[name] * np.abs(q).max()).sum(axis=1)
    assert (below > 0).all() and (counts[:, 0] >= below).all() and (counts[:, -1] == 0).all()
    check_against_extrema(ctx, g, dv, xi, Q, counts, rule, f"{name} level {level} indefinite form")
    dv.close()


def cell_values(O, implicit, level, cell, column, xi, form):
    """the statement's element values of ONE cell with `column` in its place (X.element_gradients on that cell alone)"""
    ref = implicit.reference.levels[level - 1]
    XT = implicit.construct_full_grid(level)[cell][ref.elements, :]
    D = XT[:, 1:, :] - XT[:, :1, :]
    VT = column[ref.elements]
    grad = np.linalg.solve(D, (VT[:, 1:] - VT[:, :1])[..., None])[..., 0]
    return X.element_values(grad[None], xi, None if form is None else form[cell:cell + 1])[0]


@pytest.mark.parametrize("name,level", EDGE)
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_non_finite_entries(oracle, ctx, shapes, name, level, what):
    """A NaN, and separately an inf, planted at one interior node and at one corner node of one cell: the counts against
    H.cell_counts of the statement's values of that cell, NaN bin included.  The elements that do not touch the node keep their
    statement values bit for bit (asserted): their tails lie in the intervals of the statement, and nothing but the elements that
    touch the node has moved against the clean run.  NaN: the NaN bin EQUALS the statement's.  inf: a difference with an infinite
    entry is +-inf and the form of it +inf or, where inf - inf is met on the way, NaN -- which of the two depends on the order of
    the operations, and the statement solves for the gradient where the device takes successive differences; so there the SUM of
    the two last bins is held against the statement's (to one finite element next to the last edge), every element that touches
    the node is in one of the two, and the difference of every count from H.cell_counts is printed."""
    base, implicit, g, v, xi, form, grad, q = shapes(name, level, values=True)
    ne, nel = base.nelements(), hmg.fine_elements(g, level)
    cell = ne // 2
    rule = H.quantile_rule(q)
    E = H.edges(*rule)
    lay, h2s = g.table_i32("layout", level), g.table_i32("hier2slot", level)
    off_int = int(lay[10])
    rows = {"interior": int(np.flatnonzero(h2s >= off_int)[-1]), "corner": int(np.flatnonzero(h2s == 0)[0])}
    others = np.arange(ne) != cell
    ref_el = implicit.reference.levels[level - 1].elements
    with option(ctx, 1):
        dv = hmg.DeviceMatrix(g, level).from_host(v)
        clean = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
        for case, row in rows.items():
            touching = (ref_el == row).any(axis=1)
            assert 0 < touching.sum() < nel
            bad = np.array(v, order="F")
            bad[row, cell] = np.nan if what == "nan" else np.inf
            with np.errstate(invalid="ignore", over="ignore"):
                qb = cell_values(oracle, implicit, level, cell, bad[:, cell], xi, form)
                np.testing.assert_array_equal(qb[~touching], q[cell][~touching])
                assert not np.isfinite(qb[touching]).any()
                want = H.cell_counts(qb[None], E)[0]
            dv.from_host(bad)
            counts = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
            diff = int((counts[cell] != want).sum())
            print(f"{name} level {level}, {what} at a {case} node: cell {cell} last two bins {counts[cell, -2:]} (statement "
                  f"{want[-2:]}, {int(touching.sum())} elements touch the node); {diff} of {want.size} counts differ from the statement's")
            np.testing.assert_array_equal(counts.sum(axis=1), nel)
            np.testing.assert_array_equal(counts[others], clean[others])   # every other cell: the clean run's ints
            if what == "nan":
                assert counts[cell, -1] == want[-1] == touching.sum()
                moved = clean[cell, :-1] - counts[cell, :-1]           # what the NaN elements held in the clean run
                assert (moved >= 0).all() and moved.sum() == touching.sum()
            else:
                moved = clean[cell, :-2] - counts[cell, :-2]
                gained = int(counts[cell, -2:].sum() - clean[cell, -2:].sum())
                assert (moved >= 0).all() and int(moved.sum()) == gained
                assert counts[cell, -2:].sum() >= touching.sum() >= gained
                assert abs(int(counts[cell, -2:].sum()) - int(want[-2:].sum())) <= 1     # (a finite value next to the last edge)
            # the elements that do not touch the node: the cell's tails below the two last bins lie in the statement's intervals
            qf = np.where(touching, -np.inf, qb)[None]
            lower, upper = H.tail_bounds(qf, E, MARGINS[name] * np.abs(q).max())
            # (a tail counts the touching elements that became +inf, not those in the NaN bin -- all of which touch the node)
            tail = H.tail(counts[cell:cell + 1]) - (int(touching.sum()) - int(counts[cell, -1]))
            assert ((tail >= lower) & (tail <= upper)).all()
        dv.close()


# ---- grids ----

@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_partitioned_grid_is_indexed_by_local_cell(ctx, shapes, name, level):
    base, implicit, g1, v, xi, form = shapes(name, level)
    ne = base.nelements()
    gbase = hmg.Mesh(base.nodes, base.elements + 1)
    owner = (np.arange(ne) % 2).astype(np.int32)
    d1 = hmg.DeviceMatrix(g1, level).from_host(v)
    rule = rule_around_the_peaks(ctx, g1, d1, xi, form)
    with option(ctx, 1):
        whole = hmg.cell_histogram(d1, g1, xi, form, **kw(rule))
        d1.close()
        assert (whole[:, 1:-2] > 0).sum() > 4 * ne                     # (the rule resolves something)
        for rank in (0, 1):
            g = hdist.PartitionedGrid(ctx, gbase, level, owner, rank, 2)
            loc = g.local_cells
            np.testing.assert_array_equal(loc, np.flatnonzero(owner == rank))
            dv = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v[:, loc]))
            n0 = ctx.counter(COUNTER)
            part = hmg.cell_histogram(dv, g, xi, form[loc], **kw(rule))
            assert ctx.counter(COUNTER) == n0 + 1
            assert part.dtype == whole.dtype
            np.testing.assert_array_equal(part, whole[loc])
            with pytest.raises(ValueError):
                hmg.cell_histogram(dv, g, xi, form, **kw(rule))        # a form of global length
            dv.close()
            g.close()


@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_shrunk_grid(oracle, ctx, shapes, name, level):
    base, implicit, _, v, xi, form = shapes(name, level)
    ne = base.nelements()
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)       # (a grid of its own: it is shrunk)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    rule = rule_around_the_peaks(ctx, g, dv, xi, form)
    with option(ctx, 1):
        full = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
        g.shrink(ne - 1, base.nodes.shape[0])
        assert g.ncells() == ne - 1
        part = hmg.cell_histogram(dv, g, xi, form[:ne - 1], **kw(rule))
    assert part.shape == (ne - 1, full.shape[1]) and (full[:, 1:-2] > 0).sum() > 4 * ne
    np.testing.assert_array_equal(part, full[:ne - 1])
    dv.close()
    g.close()


def test_periodic_grid(ctx):
    """A torus (driver.periodic_mesh, Tri64, n = 3, level 9: 18 cells) against an ordinary grid of the same cells as disjoint
    simplices (the corners are the minimal-image ones), bit for bit: the vector is taken as stored, the rows come from the same
    corners.  Then the invariants and the exact cross-check against the extrema window kernels, which serve the torus too."""
    level = 9
    mesh = driver.periodic_mesh(hmg.Tri64, 3)
    nodes, elements = disjoint(mesh)
    g = hmg.ImplicitFineGrid(ctx, mesh, level)
    twin = hmg.ImplicitFineGrid(ctx, hmg.Mesh(nodes, elements + 1), level)
    assert g.ncells() == twin.ncells() == 18
    rng = np.random.default_rng(41)
    v = np.asfortranarray(rng.standard_normal((g.nf(level), g.ncells())))
    xi, form = rng.standard_normal(2), T.random_spd(rng, g.ncells(), 2)
    dv, tv = hmg.DeviceMatrix(g, level).from_host(v), hmg.DeviceMatrix(twin, level).from_host(v)
    rule = rule_around_the_peaks(ctx, g, dv, xi, form)
    with option(ctx, 1):
        n0 = ctx.counter(COUNTER)
        counts = hmg.cell_histogram(dv, g, xi, form, **kw(rule))
        np.testing.assert_array_equal(hmg.cell_histogram(tv, twin, xi, form, **kw(rule)), counts)
        np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, **kw(rule)), counts)
        assert ctx.counter(COUNTER) == n0 + 3
    assert counts.shape == (18, H.nbins(*rule)) and counts.dtype == np.int64
    np.testing.assert_array_equal(counts.sum(axis=1), hmg.fine_elements(g, level))
    assert (counts[:, -1] == 0).all() and (counts[:, 1:-2] > 0).sum() > 4 * 18
    check_against_extrema(ctx, g, dv, xi, form, counts, rule, "torus level 9")
    for o in (dv, tv, g, twin):
        o.close()


# ---- refusals and bookkeeping ----

@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_option_0_refuses_and_names_the_option(ctx, shapes, name, level):
    base, implicit, g, v, xi, form = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    assert ctx.counter(OPT) == 0
    n0, l0 = ctx.counter(COUNTER), ctx.counter("cell_histogram_launches")
    match = f"hmg_cell_histogram: one cell of level {level} .*does not fit the LDS"
    with pytest.raises(hmg._lib.HmgError, match=match) as err:
        hmg.cell_histogram(dv, g, emin=-4, emax=4)
    assert OPT in str(err.value)
    # the extrema's option alone has no say
    with option(ctx, 1, XOPT):
        with pytest.raises(hmg._lib.HmgError, match=match) as err:
            hmg.cell_histogram(dv, g, emin=-4, emax=4)
        assert OPT in str(err.value)
    assert ctx.counter(COUNTER) == n0 and ctx.counter("cell_histogram_launches") == l0
    # after the refusals a served level works on the same grid, with the option still at 0 ...
    d2 = hmg.DeviceMatrix(g, 2)
    counts = hmg.cell_histogram(d2, g, np.ones(base.dim), emin=-4, emax=4)
    assert counts.sum() == g.ncells() * hmg.fine_elements(g, 2)
    assert ctx.counter(COUNTER) == n0 and ctx.counter("cell_histogram_launches") == l0 + 1
    d2.close()
    # ... and the refused level with the option at 1; a second call allocates nothing
    with option(ctx, 1):
        first = hmg.cell_histogram(dv, g, xi, form, emin=-4, emax=12)
        a0 = ctx.counter("device_allocs")
        np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, emin=-4, emax=12), first)
        assert ctx.counter("device_allocs") == a0
        assert ctx.counter(COUNTER) == n0 + 2 and ctx.counter("cell_histogram_kernel_ns") > 0
    dv.close()


# ---- the Dirichlet driver ----

def test_driver_on_2d_level_9(ctx):
    """driver.dirichlet_homogenization(1, Tri64, refinements=8): top level 9, two cells (the smallest case of
    tests/test_gpu_dirichlet_large_cells.py: a uniform medium, the corrector is zero and no cycle runs)."""
    xi = np.array([0.6, 0.8])
    args = dict(ctx=ctx, seed=2, tolerance=1e-10, fields=True, histogram=True)
    names = ("cell_moments_windows", XOPT, OPT)
    n0 = ctx.counter(COUNTER)
    r = driver.dirichlet_homogenization(1, hmg.Tri64, 8, xi, large_cells=True, **args)
    assert ctx.counter(COUNTER) == n0 + 1
    assert [ctx.counter(n) for n in names] == [0, 0, 0]                # restored
    h = r["energy_density_histogram"]
    counts, vol = h["counts"], h["volume"]
    np.testing.assert_array_equal(h["edges"], H.edges(-24, 8, 3))
    assert counts.shape == (2, 259) and counts.dtype == np.int64 and vol.shape == (259,)
    np.testing.assert_array_equal(counts.sum(axis=1), 4 ** 8)
    err = abs(vol.sum() - r["volume"]) / r["volume"]
    print(f"driver on 2D level 9: histogram volume {vol.sum():.15g} of {r['volume']:.15g} ({err:.2e}); occupied bins "
          f"{np.flatnonzero(counts.sum(axis=0))}")
    assert err <= 1e-12 and vol[-1] == 0.0
    # the tails equal the extrema counts: the corrector is zero (no cycle ran), so the driver's pass is the one on a zero vector
    assert r["cycles"] == 0
    g = hmg.ImplicitFineGrid(ctx, r["base"], 9)
    dv = hmg.DeviceMatrix(g, 9)
    form = fields.energy_form(r["cond"]) / r["energy_form"]
    with option(ctx, 1):
        np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, emin=-24, emax=8), counts)
    check_against_extrema(ctx, g, dv, xi, form, counts, (-24, 8, 3), "driver on 2D level 9")
    dv.close()
    g.close()
    # a caller's own value survives
    ctx.set_option(OPT, 2)
    try:
        driver.dirichlet_homogenization(1, hmg.Tri64, 2, xi, ctx=ctx, seed=2, histogram=True, large_cells=True)
        assert [ctx.counter(n) for n in names] == [0, 0, 2]
    finally:
        ctx.set_option(OPT, 0)
    # without large_cells: the refusal, behind the solve (here: of the moment pass, the first one on the level)
    with pytest.raises(hmg._lib.HmgError, match="one cell of level 9 .*does not fit the LDS"):
        driver.dirichlet_homogenization(1, hmg.Tri64, 8, xi, **args)
    # ... and of the histogram pass itself, with the other two passes let through
    with option(ctx, 1, "cell_moments_windows"):
        with pytest.raises(hmg._lib.HmgError, match="hmg_cell_histogram: one cell of level 9 .*does not fit the LDS"):
            driver.dirichlet_homogenization(1, hmg.Tri64, 8, xi, **args)
    assert [ctx.counter(n) for n in names] == [0, 0, 0]
