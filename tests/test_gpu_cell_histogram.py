"""GPU tests of the per-cell histograms over the fine elements (hmg_cell_histogram, csrc/hmg_histogram.hip) against the CPU statement
of tests/_cell_histogram_form.py and, exactly, against hmg_cell_extrema's threshold counts.

Shapes, vectors and forms are those of tests/test_gpu_cell_extrema.py: the perturbed 2 x 2 x 2 cube (48 cells) on levels 2 to 6
(every thread-count instantiation; level 6 with the LDS above 48 KB), the perturbed 2 x 2 square on levels 2, 5 and 8, 6 000 cells
on level 2 (the cell loop), a shrunk, a partitioned and a periodic grid.

Against the statement: the device's values carry the project's 1e-11 bound relative to the largest value, so an element next to
an edge may sit on either side of it.  With delta = 1e-9 max|q| (MARGIN of the extrema tests) every cell and every edge E must
have  #(q >= E + delta) <= tail <= #(q >= E - delta),  tail the device's number of elements at or above E -- after an assertion on
the statement alone that at most 2 % of the (cell, edge) pairs have any slack between the two counts.
Against hmg_cell_extrema: for a q that is no NaN and a finite positive edge E, q >= E <=> q > nextafter(E, -inf); so the tails at
eight edges EQUAL cell_extrema's counts for those eight predecessors as thresholds: the kernel has the extrema kernels' value
bits."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist
from homogenization_jl_amd import driver, fields
import _cell_extrema_form as X
import _cell_histogram_form as H
import _cell_moments_form as F
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
SLACK_PAIRS = 0.02


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


MESHES = {"cube": (3, 2, 6), "square": (2, 2, 8), "cube10": (3, 10, 2)}
CASES = [("cube", 2), ("cube", 3), ("cube", 4), ("cube", 5), ("cube", 6), ("square", 2), ("square", 5), ("square", 8)]
_cache = {}


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per mesh: oracle mesh and implicit grid, device grid; per (mesh, level): a consistent random vector, xi, an SPD form and
    the statement's element gradients -- computed once, shared, never changed (the recipe of tests/test_gpu_cell_extrema.py)"""
    def get(name, level):
        O = oracle
        if name not in _cache:
            dim, n, grids = MESHES[name]
            base = X.perturbed_cube(O, dim, n)
            _cache[name] = (base, O.ImplicitFineGrid.create(base, grids),
                            hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), grids))
        base, implicit, g = _cache[name]
        if (name, level) not in _cache:
            rng = np.random.default_rng(300 + level)
            v = F.consistent_random(O, implicit, level, rng)
            xi = rng.standard_normal(base.dim)
            form = T.random_spd(rng, base.nelements(), base.dim)
            grad = X.element_gradients(O, implicit, level, v)
            for a in (v, xi, form, grad):
                a.setflags(write=False)
            _cache[(name, level)] = (v, xi, form, grad)
        return (base, implicit, g) + _cache[(name, level)]
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def check_rows(counts, q, rule, nel, what):
    """counts (Ne, nbins) of the device against the statement's element values q (Ne, nt) under the rule (emin, emax, sub_bits)"""
    E = H.edges(*rule)
    delta = MARGIN * np.abs(q).max()
    lower, upper = H.tail_bounds(q, E, delta)
    slack = int((lower != upper).sum())
    print(f"{what}: rule {rule}, {slack} of {lower.size} (cell, edge) pairs have slack")
    assert slack <= SLACK_PAIRS * lower.size                           # (on the statement alone)
    assert counts.shape == (q.shape[0], H.nbins(*rule)) and counts.dtype == np.int64
    assert q.shape[1] == nel
    np.testing.assert_array_equal(counts.sum(axis=1), nel)
    assert (counts >= 0).all() and (counts[:, -1] == 0).all()          # no NaN
    tail = H.tail(counts)
    np.testing.assert_array_equal(tail, fields.histogram_tail(counts))
    bad = int(((tail < lower) | (tail > upper)).sum())
    exact = int((counts != H.cell_counts(q, E)).sum())
    print(f"{what}: {bad} tails outside their interval; {exact} of {counts.size} counts differ from the statement's own")
    assert bad == 0


def check_against_extrema(g, dv, xi, form, counts, rule, what):
    """the tails at eight edges spread over the range EQUAL hmg_cell_extrema's counts for the edges' predecessors"""
    E = H.edges(*rule)
    idx = np.unique(np.rint(np.linspace(0, len(E) - 1, 8)).astype(int))
    thr = np.nextafter(E[idx], -np.inf)
    _, _, want = hmg.cell_extrema(dv, g, xi, form, thr)
    got = H.tail(counts)[:, idx]
    print(f"{what}: {int((got != want).sum())} of {got.size} tails differ from cell_extrema's counts at {len(idx)} edges")
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name,level", CASES)
def test_device_against_the_statement(shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    q = X.element_values(grad, xi, form)
    rule = H.quantile_rule(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    counts = hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2])
    check_rows(counts, q, rule, hmg.fine_elements(g, level), f"{name} level {level}")
    assert (counts[:, 0] > 0).any() and (counts[:, -2] > 0).any()      # both end bins are populated
    # the same bits in a second run
    np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2]), counts)
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 3), ("cube", 6), ("square", 5), ("square", 8)])
def test_tails_equal_the_extrema_counts(shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    rule = H.quantile_rule(X.element_values(grad, xi, form))
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    counts = hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2])
    check_against_extrema(g, dv, xi, form, counts, rule, f"{name} level {level}")
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 3), ("square", 5)])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_every_variant_gives_the_same_counts(shapes, ctx, name, level, variant):
    """the option "cell_histogram_variant" (how counts reach the LDS histogram) changes no count; the widest rule too"""
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    q = X.element_values(grad, xi, form)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    prev = ctx.counter("cell_histogram_variant")
    try:
        for rule in (H.quantile_rule(q), (-10, 22, 5)):
            want = hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2])
            ctx.set_option("cell_histogram_variant", variant)
            got = hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2])
            ctx.set_option("cell_histogram_variant", prev)
            np.testing.assert_array_equal(got, want)
            check_against_extrema(g, dv, xi, form, got, rule, f"{name} level {level} variant {variant} rule {rule}")
        assert got.shape[1] == 1027
    finally:
        ctx.set_option("cell_histogram_variant", prev)
    dv.close()


# ---- special values ----

@pytest.mark.parametrize("name,level", [("cube", 4), ("square", 5)])
def test_zero_vector(shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    d, nel = base.dim, hmg.fine_elements(g, level)
    dv = hmg.DeviceMatrix(g, level)                                   # zero-filled
    counts = hmg.cell_histogram(dv, g, emin=-8, emax=8)
    assert (counts[:, 0] == nel).all() and (counts[:, 1:] == 0).all()   # q = 0 everywhere: below every edge
    # ... and with a xi whose |xi|^2 sits in the middle of a bin, identity form: the whole cell in that one bin (every lane of
    # every wave adds to the same address)
    E = H.edges(-2, 2, 3)
    target = 0.5 * (E[17] + E[18])
    xi1 = np.full(d, np.sqrt(target / d))
    b = int(H.bins(np.array([xi1 @ xi1]), E)[0])
    assert b == 18 and E[17] * (1 + 1e-3) < xi1 @ xi1 < E[18] * (1 - 1e-3)
    counts = hmg.cell_histogram(dv, g, xi1, emin=-2, emax=2, sub_bits=3)
    want = np.zeros_like(counts)
    want[:, b] = nel
    np.testing.assert_array_equal(counts, want)
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 3), ("square", 5)])
def test_indefinite_form(shapes, name, level):
    """the recipe of test_forms_and_threshold_counts: negative values land in bin 0, the tails are still cell_extrema's"""
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    d = base.dim
    Q = form - np.einsum("ekk->e", form)[:, None, None] / d * np.eye(d)[None]
    Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
    q = X.element_values(grad, xi, Q)
    assert q.min() < 0.0 < q.max()
    rule = H.quantile_rule(q[q > 0.0])
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    counts = hmg.cell_histogram(dv, g, xi, Q, emin=rule[0], emax=rule[1], sub_bits=rule[2])
    check_rows(counts, q, rule, hmg.fine_elements(g, level), f"{name} level {level} indefinite form")
    assert (counts[:, 0] >= (q < -MARGIN * np.abs(q).max()).sum(axis=1)).all()
    check_against_extrema(g, dv, xi, Q, counts, rule, f"{name} level {level} indefinite form")
    dv.close()


@pytest.mark.parametrize("name,level", [("cube", 4), ("square", 5)])
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_non_finite_entries(shapes, name, level, what):
    base, implicit, g, v, xi, form, grad = shapes(name, level)
    nel = hmg.fine_elements(g, level)
    rule = H.quantile_rule(X.element_values(grad, xi, form))
    kw = dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    clean = hmg.cell_histogram(dv, g, xi, form, **kw)
    cell, node = 5, v.shape[0] // 2
    touching = int((implicit.reference.levels[level - 1].elements == node).any(axis=1).sum())
    assert 0 < touching < nel
    bad = v.copy()
    bad[node, cell] = np.nan if what == "nan" else np.inf
    dv.from_host(bad)
    counts = hmg.cell_histogram(dv, g, xi, form, **kw)
    np.testing.assert_array_equal(counts.sum(axis=1), nel)
    others = np.arange(counts.shape[0]) != cell
    np.testing.assert_array_equal(counts[others], clean[others])       # every other cell: the clean run's bits
    if what == "nan":
        assert counts[cell, -1] == touching                            # every existing element that touches the node
        assert (counts[cell, :-1] <= clean[cell, :-1]).all()
    else:
        # an infinite gradient: q = +inf (the top bin), or inf - inf = NaN on the way -- every element that touches the node
        # sits in one of the two, and nothing else has moved
        moved = clean[cell, :-2] - counts[cell, :-2]
        gained = int(counts[cell, -2:].sum() - clean[cell, -2:].sum())
        assert (moved >= 0).all() and int(moved.sum()) == gained
        assert counts[cell, -2:].sum() >= touching >= gained
    dv.close()


# ---- shapes ----

def test_more_cells_than_resident_workgroups(shapes):
    base, implicit, g, v, xi, form, grad = shapes("cube10", 2)
    assert base.nelements() == 6000 > 16 * 256
    q = X.element_values(grad, xi, form)
    rule = H.quantile_rule(q)
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    counts = hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2])
    check_rows(counts, q, rule, 8, "6000 cells level 2")
    check_against_extrema(g, dv, xi, form, counts, rule, "6000 cells level 2")
    dv.close()


def test_shrunk_grid(oracle, ctx):
    O = oracle
    base = X.perturbed_cube(O, 3, 2)
    level = 3
    implicit = O.ImplicitFineGrid.create(base, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    rng = np.random.default_rng(11)
    v = F.consistent_random(O, implicit, level, rng)
    xi, form = rng.standard_normal(3), T.random_spd(rng, 48, 3)
    q = X.element_values(X.element_gradients(O, implicit, level, v), xi, form)
    rule = H.quantile_rule(q)
    kw = dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    full = hmg.cell_histogram(dv, g, xi, form, **kw)
    g.shrink(47, base.nodes.shape[0])
    assert g.ncells() == 47
    part = hmg.cell_histogram(dv, g, xi, form[:47], **kw)
    assert part.shape == (47, full.shape[1])
    np.testing.assert_array_equal(part, full[:47])
    check_rows(part, q[:47], rule, 64, "47 of 48 cells")
    dv.close()
    g.close()


@pytest.mark.parametrize("name,level", [("cube", 3), ("square", 5)])
def test_partitioned_grid_is_indexed_by_local_cell(ctx, shapes, name, level):
    base, implicit, g1, v, xi, form, grad = shapes(name, level)
    ne = base.nelements()
    gbase = hmg.Mesh(base.nodes, base.elements + 1)
    owner = (np.arange(ne) % 2).astype(np.int32)
    rule = H.quantile_rule(X.element_values(grad, xi, form))
    kw = dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])
    d1 = hmg.DeviceMatrix(g1, level).from_host(v)
    whole = hmg.cell_histogram(d1, g1, xi, form, **kw)
    d1.close()
    for rank in (0, 1):
        g = hdist.PartitionedGrid(ctx, gbase, level, owner, rank, 2)
        loc = g.local_cells
        dv = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v[:, loc]))
        part = hmg.cell_histogram(dv, g, xi, form[loc], **kw)
        assert part.dtype == whole.dtype
        np.testing.assert_array_equal(part, whole[loc])
        with pytest.raises(ValueError):
            hmg.cell_histogram(dv, g, xi, form, **kw)                  # a form of global length
        dv.close()
        g.close()


def test_periodic_grid(ctx):
    """A torus (driver.periodic_mesh, Tri64, n = 3, level 4): the invariants -- shape, row sums, an empty NaN bin, the same bits
    twice -- and the exact cross-check against hmg_cell_extrema, which serves the torus with the same rows.  The histogram of a
    torus against the statement (on the cells as disjoint simplices, whose corners are the minimal-image ones) and against an
    ordinary grid of those simplices, bit for bit, is tests/test_gpu_periodic_fields.py::test_cell_histogram."""
    level = 4
    mesh = driver.periodic_mesh(hmg.Tri64, 3)
    g = hmg.ImplicitFineGrid(ctx, mesh, level)
    dv = hmg.DeviceMatrix(g, level)
    dv.rand(41)
    rng = np.random.default_rng(41)
    xi, form = rng.standard_normal(2), T.random_spd(rng, g.ncells(), 2)
    qmax, qmin, _ = hmg.cell_extrema(dv, g, xi, form)
    rule = (int(np.floor(np.log2(np.median(qmin)))), int(np.ceil(np.log2(np.median(qmax)))), 3)
    kw = dict(emin=rule[0], emax=rule[1], sub_bits=rule[2])
    counts = hmg.cell_histogram(dv, g, xi, form, **kw)
    nel = hmg.fine_elements(g, level)
    assert counts.shape == (g.ncells(), H.nbins(*rule)) and counts.dtype == np.int64
    np.testing.assert_array_equal(counts.sum(axis=1), nel)
    assert (counts[:, -1] == 0).all() and (counts[:, 1:-2] > 0).any()
    check_against_extrema(g, dv, xi, form, counts, rule, "torus level 4")
    np.testing.assert_array_equal(hmg.cell_histogram(dv, g, xi, form, **kw), counts)
    dv.close()
    g.close()


# ---- refusals and bookkeeping ----

@pytest.mark.parametrize("dim,level", [(3, 7), (2, 9)])
@pytest.mark.parametrize("windows", [0, 1])
def test_larger_cells_are_refused_whatever_the_window_option_says(oracle, ctx, dim, level, windows):
    base = oracle.hypercube(dim, 1)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    dv = hmg.DeviceMatrix(g, level)
    prev = ctx.counter("cell_extrema_windows")
    ctx.set_option("cell_extrema_windows", windows)
    try:
        with pytest.raises(hmg._lib.HmgError, match=f"hmg_cell_histogram: one cell of level {level} .*does not fit the LDS"):
            hmg.cell_histogram(dv, g, emin=-4, emax=4)
    finally:
        ctx.set_option("cell_extrema_windows", prev)
    # ... and a level that is served goes on working on the same grid
    d2 = hmg.DeviceMatrix(g, 2)
    counts = hmg.cell_histogram(d2, g, np.ones(dim), emin=-4, emax=4)
    assert counts.sum() == g.ncells() * hmg.fine_elements(g, 2) == counts[:, int(H.bins(np.array([float(dim)]), H.edges(-4, 4, 3))[0])].sum()
    for o in (dv, d2, g):
        o.close()


def test_bad_arguments_are_refused(shapes, ctx):
    base, implicit, g, v, xi, form, grad = shapes("cube", 2)
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    L = hmg._lib
    lib = L.load()
    counts = np.zeros((g.ncells(), 67), dtype=np.int64)
    pc = counts.ctypes.data_as(L.p_i64)
    n0 = ctx.counter("cell_histogram_launches")
    # a vector of another grid
    g2 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(L.HmgError, match="hmg_cell_histogram: .*another grid"):
        hmg.cell_histogram(dv, g2, emin=-4, emax=4)
    g2.close()
    # null arguments: the C entry point itself
    assert lib.hmg_cell_histogram(g.h, None, None, None, -4, 4, 3, pc) != 0
    assert "hmg_cell_histogram: null vector" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_histogram(g.h, dv.h, None, None, -4, 4, 3, None) != 0
    assert "hmg_cell_histogram: null counts" in lib.hmg_last_error().decode()
    # bin parameters outside the rule, each named; more regular bins than the LDS holds next to a cell
    for kw, msg in ((dict(emin=4, emax=4), "emin = 4 is not below emax = 4"), (dict(emin=-1023, emax=4), "emin = -1023 is outside"),
                    (dict(emin=0, emax=1024), "emax = 1024 is outside"), (dict(emin=0, emax=4, sub_bits=6), "sub_bits = 6"),
                    (dict(emin=0, emax=33, sub_bits=5), "1056 regular bins"), (dict(emin=-1022, emax=1023, sub_bits=0), "2045 regular bins")):
        sb = kw.get("sub_bits", 3)
        assert lib.hmg_cell_histogram(g.h, dv.h, None, None, kw["emin"], kw["emax"], sb, pc) != 0
        assert "hmg_cell_histogram: " + msg in lib.hmg_last_error().decode()
    # non-finite form and xi
    bad = form.copy()
    bad[5, 1, 1] = np.inf
    with pytest.raises(L.HmgError, match="hmg_cell_histogram: the form of cell 5 is not finite"):
        hmg.cell_histogram(dv, g, form=bad, emin=-4, emax=4)
    for x in (np.nan, np.inf):
        with pytest.raises(L.HmgError, match="hmg_cell_histogram: xi is not finite"):
            hmg.cell_histogram(dv, g, xi=np.array([1.0, x, 0.0]), emin=-4, emax=4)
    assert ctx.counter("cell_histogram_launches") == n0                # nothing was launched
    # ... and the next call succeeds
    q = X.element_values(grad, xi, form)
    rule = H.quantile_rule(q)
    check_rows(hmg.cell_histogram(dv, g, xi, form, emin=rule[0], emax=rule[1], sub_bits=rule[2]), q, rule, 8, "after the refusals")
    assert ctx.counter("cell_histogram_launches") == n0 + 1
    dv.close()


def test_allocations_settle_and_counters_count(shapes, ctx):
    """the first call on a level uploads its element mask and makes the pool blocks; a second call allocates nothing"""
    base, implicit, g, v, xi, form, _ = shapes("cube", 4)
    dv = hmg.DeviceMatrix(g, 4).from_host(v)
    hmg.cell_histogram(dv, g, xi, form, emin=-8, emax=8)
    n0, l0 = ctx.counter("device_allocs"), ctx.counter("cell_histogram_launches")
    hmg.cell_histogram(dv, g, xi, form, emin=-8, emax=8)
    assert ctx.counter("device_allocs") == n0
    assert ctx.counter("cell_histogram_launches") == l0 + 1
    assert ctx.counter("cell_histogram_kernel_ns") > 0
    dv.close()


# ---- the Dirichlet driver ----

@pytest.mark.parametrize("eltype,refinements,xi", [(hmg.Tri64, 3, [0.6, 0.8]), (hmg.Tet64, 2, [0.6, 0.0, 0.8])])
def test_driver(ctx, eltype, refinements, xi):
    n = refinements
    xi = np.array(xi)
    kw = dict(ctx=ctx, seed=2, values=(1.0, 9.0))
    plain = driver.dirichlet_homogenization(2, eltype, n, xi, fields=True, **kw)
    r = driver.dirichlet_homogenization(2, eltype, n, xi, fields=True, histogram=True, **kw)
    assert set(r) == set(plain) | {"energy_density_histogram"} and "energy_density_histogram" not in plain
    for k in plain:                                                   # every other entry keeps its bits
        if k != "base":
            np.testing.assert_array_equal(np.asarray(plain[k]), np.asarray(r[k]))
    h = r["energy_density_histogram"]
    E, counts, vol = h["edges"], h["counts"], h["volume"]
    np.testing.assert_array_equal(E, H.edges(-24, 8, 3))
    assert counts.shape == (r["volumes"].shape[0], len(E) + 2) and vol.shape == (len(E) + 2,)
    np.testing.assert_allclose(vol.sum(), r["volume"], rtol=1e-13)
    assert vol[-1] == 0.0 and vol[-2] == 0.0                           # the top and the NaN bin are empty
    # the form is sigma_c / energy_form: the volume-weighted mean of q is 1, and it lies between the means of the bins' ends
    lo = np.concatenate(([0.0], E))                                    # (sigma is positive definite: bin 0 starts at 0)
    hi = np.concatenate((E, [np.inf]))
    low, high = float(vol[:-1] @ lo), float(vol[:-2] @ hi[:-1])
    print(f"{eltype}: sum vol lo = {low / r['volume']:.6f}, sum vol hi = {high / r['volume']:.6f} of the volume")
    assert low <= r["volume"] * (1 + 1e-10)
    assert high >= r["volume"] * (1 - 1e-10)
    med = fields.histogram_quantile(vol, E, 0.5)
    assert 0.0 < med[0] < med[1] < np.inf
    # a dict names the rule
    r2 = driver.dirichlet_homogenization(2, eltype, n, xi, histogram={"emin": -24, "emax": 8, "sub_bits": 3}, **kw)
    np.testing.assert_array_equal(r2["energy_density_histogram"]["counts"], counts)
    with pytest.raises(ValueError):
        driver.dirichlet_homogenization(2, eltype, n, xi, histogram={"emin": -24}, **kw)
