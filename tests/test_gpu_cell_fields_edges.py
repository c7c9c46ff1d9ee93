"""GPU tests of the edges of the per-cell field calls (hmg_cell_moments, hmg_cell_pair_moments, hmg_cell_extrema; include/hmg.h):

  partitioned grids   all three on the LOCAL cells of a dist.PartitionedGrid -- Delaunay meshes in 3D and 2D, three owners, one
                      process, no communicator: the rows of the unpartitioned grid at grid.local_cells, bit for bit, where the
                      unpartitioned extrema are held against the statement (the first meshes of that test that are no perturbed
                      cubes); `form` per local cell, a form of global length refused; after a shrink the prefix of the local
                      rows; the synthetic-cut rehearsal grid (cut-first cell lists); the window kernels on a partition
  NaN                 the rule of hmg_cell_extrema: maximum and minimum of a cell are NaN exactly when q_T is NaN on one of its
                      existing elements -- against numpy's max / min of the statement's element values; an infinite value stays
                      a value; the cells next to it keep their bits
  level 1             served by all three (one element per cell), against the statements
  strict thresholds   counts are of q_T > t: at t = a value itself no element of that value counts, one ulp below all do

Bound against a statement: 1e-11 of the largest magnitude, the project's (tests/test_gpu_cell_extrema.py, test_gpu_cell_moments.py);
everything else is bit for bit."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist, fields
import _cell_extrema_form as X
import _cell_moments_form as F
import _cell_pair_moments_form as P
import _meshes
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
MARGIN = 1e-9


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def equal_bits(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b, err_msg=what)


def extrema_against_statement(got, q, thr, what):
    """(qmax, qmin, counts) of the device against the statement's element values q: 1e-11 of the largest maximum, counts equal
    where no element lies within 1e-9 of a threshold (asserted on the statement alone)"""
    wmax, wmin, wcounts = X.extrema(q, thr)
    scale = np.abs(wmax).max()
    if len(thr):
        mg = X.margin(q, thr)
        print(f"{what}: no element within {mg:.2e} of a threshold (relative to the largest value)")
        assert mg > MARGIN
    e1, e2 = np.abs(got[0] - wmax).max() / scale, np.abs(got[1] - wmin).max() / scale
    print(f"{what}: max {e1:.2e} min {e2:.2e} of the largest maximum {scale:.3e}")
    assert e1 <= TOL and e2 <= TOL
    np.testing.assert_array_equal(got[2], wcounts)


# ---- partitioned grids ----

def three_calls(g, dv, dw, xi, xw, form, thr):
    return (hmg.cell_moments(dv, g, xi), hmg.cell_pair_moments(dv, dw, g, xi, xw), hmg.cell_extrema(dv, g, xi, form, thr))


def at_cells(res, cells):
    return tuple(tuple(a[cells] for a in r) if isinstance(r, tuple) else r[cells] for r in res)


def flat(res):
    return tuple(a for r in res for a in (r if isinstance(r, tuple) else (r,)))


@pytest.mark.parametrize("dim,npts,levels,lower", [(3, 60, 3, 2), (2, 70, 5, 4)])
def test_partitioned_delaunay_grid_gives_the_rows_of_its_local_cells(oracle, ctx, dim, npts, levels, lower):
    O = oracle
    dm = _meshes.delaunay_mesh(O, dim, npts, 13)
    ne = dm.nelements()
    gbase = hmg.Mesh(dm.nodes, dm.elements + 1)
    owner = ((np.arange(ne) * 2654435761 >> 7) % 3).astype(np.int32)
    implicit = O.ImplicitFineGrid.create(dm, levels)
    g1 = hmg.ImplicitFineGrid(ctx, gbase, levels)
    g = hdist.PartitionedGrid(ctx, gbase, levels, owner, 1, 3)
    loc = g.local_cells
    np.testing.assert_array_equal(loc, np.flatnonzero(owner == 1))
    assert 0 < loc.size < ne and g.ncells() == loc.size
    for level in (levels, lower):
        rng = np.random.default_rng(1)
        v, w = F.consistent_random(O, implicit, level, rng), F.consistent_random(O, implicit, level, rng)
        xi, xw = rng.standard_normal(dim), rng.standard_normal(dim)
        form = T.random_spd(rng, ne, dim)
        q = X.element_values(X.element_gradients(O, implicit, level, v), xi, form)
        # (the slivers of a Delaunay mesh spread the element values over ten decades, and a margin is measured against the LARGEST
        #  value: only the upper quantiles have gaps that show at that scale)
        thr = X.gap_thresholds(q, quantiles=(0.90, 0.99, 0.999, 0.9999))
        d1v, d1w = hmg.DeviceMatrix(g1, level).from_host(v), hmg.DeviceMatrix(g1, level).from_host(w)
        dv = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v[:, loc]))
        dw = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(w[:, loc]))
        whole = three_calls(g1, d1v, d1w, xi, xw, form, thr)
        extrema_against_statement(whole[2], q, thr, f"{dim}D Delaunay mesh level {level}, unpartitioned")
        part = three_calls(g, dv, dw, xi, xw, form[loc], thr)
        assert part[0][0].shape == (loc.size, dim) and part[1].shape == (loc.size, dim, dim) and part[2][2].shape == (loc.size, 4)
        equal_bits(flat(part), flat(at_cells(whole, loc)), f"{dim}D level {level}: partitioned against unpartitioned at local_cells")
        # the form is per LOCAL cell: the global one is refused
        with pytest.raises(ValueError, match="form must have shape"):
            hmg.cell_extrema(dv, g, xi, form, thr)
        for o in (d1v, d1w, dv, dw):
            o.close()
    g.close()
    g1.close()


@pytest.mark.parametrize("dim,n,levels,radius", [(3, 4, 3, 1.0), (2, 6, 5, 2.0)])
def test_partitioned_grid_after_a_shrink_gives_the_prefix_of_its_rows(oracle, ctx, dim, n, levels, radius):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(dim, n, origin=(-n / 2.0,) * dim))
    ne = m.nelements()
    gbase = hmg.Mesh(m.nodes, m.elements + 1)
    owner = ((np.arange(ne) * 2654435761 >> 7) % 3).astype(np.int32)
    implicit = O.ImplicitFineGrid.create(m, levels)
    g = hdist.PartitionedGrid(ctx, gbase, levels, owner, 1, 3)
    hmg.L2PlusDivAGrad(g, 0.0, np.ones((ne, dim)))                     # (a shrink re-forms the operator's tables; the GLOBAL field)
    rng = np.random.default_rng(60 + dim)
    v, w = F.consistent_random(O, implicit, levels, rng), F.consistent_random(O, implicit, levels, rng)
    xi, xw = rng.standard_normal(dim), rng.standard_normal(dim)
    form = T.random_spd(rng, ne, dim)
    thr = X.gap_thresholds(X.element_values(X.element_gradients(O, implicit, levels, v), xi, form))
    loc = g.local_cells.copy()
    dv = hmg.DeviceMatrix(g, levels).from_host(np.asfortranarray(v[:, loc]))
    dw = hmg.DeviceMatrix(g, levels).from_host(np.asfortranarray(w[:, loc]))
    before = three_calls(g, dv, dw, xi, xw, form[loc], thr)
    keep_e, keep_n = O.find_elements_in_radius(m, radius), O.find_nodes_in_radius(m, radius)
    assert 0 < keep_e < ne
    g.shrink(keep_e, keep_n)
    k = g.ncells()
    assert 0 < k < loc.size and k == int((loc < keep_e).sum())
    np.testing.assert_array_equal(g.local_cells, loc[:k])
    after = three_calls(g, dv, dw, xi, xw, form[loc[:k]], thr)
    assert after[2][0].shape == (k,)
    equal_bits(flat(after), flat(at_cells(before, slice(0, k))), f"{dim}D: after the shrink against the prefix")
    for o in (dv, dw, g):
        o.close()


def test_synthetic_cut_rehearsal_grid_gives_the_plain_grids_bits(oracle):
    """cut-first cell lists, every cell local: the per-cell calls walk the columns, not those lists.  (A context of its own,
    closed at the end, as in tests/test_gpu_dist.py: the rehearsal makes a 1-rank communicator.)"""
    O = oracle
    L = 4
    ctx = hmg.Context(0)
    try:
        prob = hdist.partitioned_checkerboard(ctx, 4, L, 1, 0, backend="rccl", synthetic_cut=True)
        g = prob.implicit
        g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
        ne = g1.ncells()
        np.testing.assert_array_equal(g.local_cells, np.arange(ne))
        assert g.table_i32("cut_counts").sum() > 0
        mesh = O.Mesh(prob.global_base.nodes, prob.global_base.elements - 1)
        implicit = O.ImplicitFineGrid.create(mesh, L)
        rng = np.random.default_rng(70)
        xi, xw = rng.standard_normal(3), rng.standard_normal(3)
        form = fields.energy_form(prob.cond)
        for level in (L, 2):
            v, w = F.consistent_random(O, implicit, level, rng), F.consistent_random(O, implicit, level, rng)
            res = []
            for grid in (g, g1):
                dv, dw = hmg.DeviceMatrix(grid, level).from_host(v), hmg.DeviceMatrix(grid, level).from_host(w)
                res.append(three_calls(grid, dv, dw, xi, xw, form, [1.0, 10.0, 100.0]))
                dv.close()
                dw.close()
            equal_bits(flat(res[0]), flat(res[1]), f"synthetic cut, level {level}")
    finally:
        ctx.close()


def test_window_kernels_on_a_partitioned_grid(oracle, ctx):
    """2D level 9 (a cell larger than the LDS) through the row-band kernel, the cells alternating between two owners; the
    unpartitioned grid's results at this shape are held against the statement by tests/test_gpu_cell_moments_window.py"""
    O = oracle
    levels = 9
    base = X.perturbed_cube(O, 2, 2)
    ne = base.nelements()
    gbase = hmg.Mesh(base.nodes, base.elements + 1)
    owner = (np.arange(ne) % 2).astype(np.int32)
    implicit = O.ImplicitFineGrid.create(base, levels)
    rng = np.random.default_rng(80)
    v, w = F.consistent_random(O, implicit, levels, rng), F.consistent_random(O, implicit, levels, rng)
    xi, xw = rng.standard_normal(2), rng.standard_normal(2)
    prev = ctx.counter("cell_moments_windows")
    ctx.set_option("cell_moments_windows", 1)
    try:
        g1 = hmg.ImplicitFineGrid(ctx, gbase, levels)
        d1v, d1w = hmg.DeviceMatrix(g1, levels).from_host(v), hmg.DeviceMatrix(g1, levels).from_host(w)
        whole = (hmg.cell_moments(d1v, g1, xi), hmg.cell_pair_moments(d1v, d1w, g1, xi, xw))
        for rank in (0, 1):
            g = hdist.PartitionedGrid(ctx, gbase, levels, owner, rank, 2)
            loc = g.local_cells
            np.testing.assert_array_equal(loc, np.flatnonzero(owner == rank))
            dv = hmg.DeviceMatrix(g, levels).from_host(np.asfortranarray(v[:, loc]))
            dw = hmg.DeviceMatrix(g, levels).from_host(np.asfortranarray(w[:, loc]))
            n0 = ctx.counter("cell_moments_window_launches")
            part = (hmg.cell_moments(dv, g, xi), hmg.cell_pair_moments(dv, dw, g, xi, xw))
            assert ctx.counter("cell_moments_window_launches") == n0 + 2
            equal_bits(flat(part), flat(at_cells(whole, loc)), f"window kernels, rank {rank}")
            for o in (dv, dw, g):
                o.close()
        for o in (d1v, d1w, g1):
            o.close()
    finally:
        ctx.set_option("cell_moments_windows", prev)


# ---- NaN and inf in hmg_cell_extrema ----

NAN_GRIDS = [(3, 1, 2), (3, 1, 4), (2, 2, 5)]                           # dim, n of the perturbed cube, level
_nan = {}


@pytest.fixture(scope="module")
def nan_shapes(oracle, ctx):
    """per grid: a consistent random vector, xi, an SPD form, the statement's element values and the device's results on them
    (computed once, read only); the host rows of the vertex slots and of the slots that are no vertex"""
    def get(dim, n, level):
        O = oracle
        key = (dim, n, level)
        if key not in _nan:
            base = X.perturbed_cube(O, dim, n)
            implicit = O.ImplicitFineGrid.create(base, level)
            g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
            rng = np.random.default_rng(90 + level)
            v = F.consistent_random(O, implicit, level, rng)
            xi, form = rng.standard_normal(dim), T.random_spd(rng, base.nelements(), dim)
            q = X.element_values(X.element_gradients(O, implicit, level, v), xi, form)
            thr = X.gap_thresholds(q)
            dv = hmg.DeviceMatrix(g, level).from_host(v)
            clean = hmg.cell_extrema(dv, g, xi, form, thr)
            dv.close()
            extrema_against_statement(clean, q, thr, f"{dim}D level {level}, clean")
            lay, h2s = g.table_i32("layout", level), g.table_i32("hier2slot", level)
            ncorner, off_int, nint = int(lay[2]), int(lay[10]), int(lay[7])
            vertex = np.flatnonzero(h2s < ncorner)
            inner = np.flatnonzero(h2s >= off_int) if nint else np.flatnonzero(h2s >= ncorner)   # (3D level 2 has no cell interior)
            assert vertex.size == dim + 1 and inner.size > 0
            for a in (v, xi, form, q, thr) + clean:
                a.setflags(write=False)
            _nan[key] = (base, implicit, g, v, xi, form, q, thr, clean, vertex, inner)
        return _nan[key]
    yield get
    for val in _nan.values():
        val[2].close()
    _nan.clear()


def statement_with_nan(q, thr):
    """numpy's max / min propagate a NaN; a NaN compares false"""
    with np.errstate(invalid="ignore"):
        return X.extrema(q, thr)


@pytest.mark.parametrize("dim,n,level", NAN_GRIDS)
@pytest.mark.parametrize("case", ["vertex", "inner", "column"])
def test_nan_in_a_column_gives_nan_extrema_of_that_cell_alone(oracle, nan_shapes, dim, n, level, case):
    base, implicit, g, v, xi, form, q, thr, clean, vertex, inner = nan_shapes(dim, n, level)
    ne = base.nelements()
    cell = ne // 2
    bad = np.array(v, order="F")
    if case == "vertex":
        bad[vertex[1], cell] = np.nan
    elif case == "inner":
        bad[inner[-1], cell] = np.nan
    else:
        bad[:, cell] = np.nan
    with np.errstate(invalid="ignore"):
        qb = X.element_values(X.element_gradients(oracle, implicit, level, bad), xi, form)
    nan_el = np.isnan(qb)
    assert not nan_el[np.arange(ne) != cell].any() and nan_el[cell].any()        # (the vector as stored: no other column changed)
    np.testing.assert_array_equal(qb[~nan_el], q[~nan_el])
    assert nan_el[cell].all() == (case == "column" or level == 1)
    wmax, wmin, wcounts = statement_with_nan(qb, thr)
    assert np.isnan(wmax[cell]) and np.isnan(wmin[cell])
    dv = hmg.DeviceMatrix(g, level).from_host(bad)
    qmax, qmin, counts = hmg.cell_extrema(dv, g, xi, form, thr)
    dv.close()
    print(f"{dim}D level {level}, {case}: cell {cell} max {qmax[cell]} min {qmin[cell]} counts {counts[cell]} (statement {wcounts[cell]}; "
          f"{int(nan_el[cell].sum())} of {nan_el.shape[1]} elements NaN)")
    assert np.isnan(qmax[cell]) and np.isnan(qmin[cell])
    np.testing.assert_array_equal(counts, wcounts)                       # (the NaN elements are counted nowhere)
    others = np.arange(ne) != cell
    for a, b in zip((qmax, qmin), clean[:2]):
        np.testing.assert_array_equal(a[others], b[others])             # the neighbours keep their bits
    # with numpy's rule on both sides: the whole arrays
    np.testing.assert_allclose(qmax, wmax, rtol=0, atol=TOL * np.nanmax(np.abs(wmax)), equal_nan=True)
    np.testing.assert_allclose(qmin, wmin, rtol=0, atol=TOL * np.nanmax(np.abs(wmax)), equal_nan=True)
    # ... and what the driver makes of it: a NaN peak gives a NaN concentration, not -inf
    assert np.isnan(fields.concentration(qmax, 1.0)[cell]) and np.isfinite(fields.concentration(qmax, 1.0)[others]).all()


@pytest.mark.parametrize("dim,n,level", NAN_GRIDS)
def test_an_infinite_value_stays_a_value(oracle, nan_shapes, dim, n, level):
    """one cell's column is HUGE * (i + j + k) of the node's lattice coordinates: exact, constant along two of the three basis
    directions of the Kuhn lattice, so that every element of the cell has the gradient (HUGE, 0, 0) in the kernel's coordinates
    and q_T = Q~_00 HUGE^2 overflows to +inf without any inf - inf; in the statement the squares of the physical gradient's
    components overflow and are summed (form None).  +inf is the maximum AND the minimum of that cell, every element exceeds every
    threshold, and no NaN appears."""
    base, implicit, g, v, _, _, _, _, _, vertex, inner = nan_shapes(dim, n, level)
    ne = base.nelements()
    cell = ne // 2
    huge = 2.0 ** 530
    lattice = np.rint(implicit.reference.levels[level - 1].nodes * 2 ** (level - 1))
    bad = np.array(v, order="F")
    bad[:, cell] = huge * lattice.sum(axis=1)
    with np.errstate(over="ignore"):
        qb = X.element_values(X.element_gradients(oracle, implicit, level, bad))
    assert np.isposinf(qb[cell]).all() and np.isfinite(np.delete(qb, cell, axis=0)).all()
    thr = X.gap_thresholds(np.delete(qb, cell, axis=0))
    wmax, wmin, wcounts = X.extrema(qb, thr)
    dv = hmg.DeviceMatrix(g, level).from_host(bad)
    qmax, qmin, counts = hmg.cell_extrema(dv, g, None, None, thr)
    dv.close()
    print(f"{dim}D level {level}: cell {cell} max {qmax[cell]} min {qmin[cell]} counts {counts[cell]}")
    assert np.isposinf(qmax[cell]) and np.isposinf(qmin[cell])
    assert (counts[cell] == hmg.fine_elements(g, level)).all()
    others = np.arange(ne) != cell
    scale = wmax[others].max()
    assert np.abs(qmax[others] - wmax[others]).max() <= TOL * scale and np.abs(qmin[others] - wmin[others]).max() <= TOL * scale
    assert X.margin(qb[others], thr) > MARGIN
    np.testing.assert_array_equal(counts, wcounts)


@pytest.mark.parametrize("dim,n,level", NAN_GRIDS)
def test_an_infinite_entry(oracle, nan_shapes, dim, n, level):
    """a +inf ENTRY of the column: the elements around the node have differences +inf and -inf, and what an expression makes of
    those (inf, -inf or inf - inf = NaN) depends on its order of evaluation -- the kernel's, in lattice coordinates, is not the
    statement's.  What does not depend on it: the cell's maximum and minimum are both NaN or neither is; if neither, the elements
    at the node are infinite, so the maximum is +inf or the minimum -inf; the other elements are counted as before or, where they
    touch the node, differently; and the other cells keep their bits."""
    base, implicit, g, v, xi, form, q, thr, clean, vertex, inner = nan_shapes(dim, n, level)
    ne = base.nelements()
    cell = ne // 2
    bad = np.array(v, order="F")
    bad[inner[-1], cell] = np.inf
    dv = hmg.DeviceMatrix(g, level).from_host(bad)
    qmax, qmin, counts = hmg.cell_extrema(dv, g, xi, form, thr)
    dv.close()
    with np.errstate(invalid="ignore", over="ignore"):
        qb = X.element_values(X.element_gradients(oracle, implicit, level, bad), xi, form)
        wmax, wmin, _ = statement_with_nan(qb, thr)
    print(f"{dim}D level {level}: cell {cell} max {qmax[cell]} min {qmin[cell]} counts {counts[cell]}; statement max {wmax[cell]} "
          f"min {wmin[cell]}")
    assert np.isnan(qmax[cell]) == np.isnan(qmin[cell])
    assert np.isnan(qmax[cell]) or np.isposinf(qmax[cell]) or np.isneginf(qmin[cell])
    # at these shapes both orders of evaluation meet an inf - inf on some element at the node: NaN in the statement, NaN here
    scale = np.nanmax(np.abs(wmax[np.isfinite(wmax)]))
    np.testing.assert_allclose(qmax, wmax, rtol=0, atol=TOL * scale, equal_nan=True)
    np.testing.assert_allclose(qmin, wmin, rtol=0, atol=TOL * scale, equal_nan=True)
    touched = int((~np.isfinite(qb[cell])).sum())                        # the elements at the node
    assert 0 < touched < qb.shape[1] or level == 1
    assert (np.abs(counts[cell] - clean[2][cell]) <= touched).all()
    others = np.arange(ne) != cell
    for a, b in zip((qmax, qmin, counts), clean):
        np.testing.assert_array_equal(a[others], b[others])


# ---- level 1 ----

@pytest.mark.parametrize("dim", [3, 2])
def test_level_1_is_served(oracle, ctx, dim):
    O = oracle
    base = X.perturbed_cube(O, dim, 2)
    ne = base.nelements()
    implicit = O.ImplicitFineGrid.create(base, 2)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 2)
    rng = np.random.default_rng(20 + dim)
    v, w = F.consistent_random(O, implicit, 1, rng), F.consistent_random(O, implicit, 1, rng)
    assert v.shape == (dim + 1, ne) and hmg.fine_elements(g, 1) == 1
    xi, xw = rng.standard_normal(dim), rng.standard_normal(dim)
    form = T.random_spd(rng, ne, dim)
    vol = F.cell_volumes(O, base)
    dv, dw = hmg.DeviceMatrix(g, 1).from_host(v), hmg.DeviceMatrix(g, 1).from_host(w)
    # moments
    mean, gram = hmg.cell_moments(dv, g, xi)
    mv, gv = F.reference_form(O, implicit, 1, v)
    wm, wg = F.with_xi(mv, gv, vol, xi)
    e1, e2 = np.abs(mean - wm).max() / np.abs(wm).max(), np.abs(gram - wg).max() / np.abs(wg).max()
    print(f"{dim}D level 1: mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    # pair moments
    S = hmg.cell_pair_moments(dv, dw, g, xi, xw)
    _, mw, pair = P.reference_form(O, implicit, 1, v, w)
    gw = F.reference_form(O, implicit, 1, w)[1]
    sc = min(P.scale(gv, gw), P.scale(wg, F.with_xi(mw, gw, vol, xw)[1]))
    e = np.abs(S - P.with_xi(mv, mw, pair, vol, xi, xw)).max() / sc
    print(f"{dim}D level 1: pair {e:.2e}")
    assert e <= TOL
    # extrema: the cell is its only element
    q = X.element_values(X.element_gradients(O, implicit, 1, v), xi, form)
    assert q.shape == (ne, 1)
    thr = X.gap_thresholds(q, quantiles=(0.25, 0.75))
    got = hmg.cell_extrema(dv, g, xi, form, thr)
    extrema_against_statement(got, q, thr, f"{dim}D level 1")
    np.testing.assert_array_equal(got[0], got[1])
    assert set(np.unique(got[2])) <= {0, 1} and 0 < got[2].sum() < got[2].size
    # ... which is the energy density of the moments: Q : G / |c|
    dens = np.einsum("ekl,ekl->e", form, gram) / vol
    assert np.abs(got[0] - dens).max() <= 1e-10 * np.abs(dens).max()
    # the next call on level 2 of the same grid
    v2 = F.consistent_random(O, implicit, 2, rng)
    d2 = hmg.DeviceMatrix(g, 2).from_host(v2)
    m2, g2 = hmg.cell_moments(d2, g)
    wm2, wg2 = F.reference_form(O, implicit, 2, v2)
    assert np.abs(m2 - wm2).max() <= TOL * np.abs(wm2).max() and np.abs(g2 - wg2).max() <= TOL * np.abs(wg2).max()
    q2 = X.element_values(X.element_gradients(O, implicit, 2, v2), xi, form)
    extrema_against_statement(hmg.cell_extrema(d2, g, xi, form), q2, [], f"{dim}D level 2 after level 1")
    for o in (dv, dw, d2, g):
        o.close()


# ---- strict thresholds ----

@pytest.mark.parametrize("dim,level", [(3, 2), (3, 6), (2, 5), (2, 8)])
def test_a_threshold_at_a_value_does_not_count_it(oracle, ctx, dim, level):
    """v = 0, xi = e_1, form None: every element of a cell evaluates ONE expression of the cell's row, q = |xi|^2 = 1 to rounding"""
    base = oracle.hypercube(dim, 1)
    ne = base.nelements()
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    dv = hmg.DeviceMatrix(g, level).fill(0.0)
    xi = np.eye(dim)[0]
    qmax, qmin, _ = hmg.cell_extrema(dv, g, xi)
    np.testing.assert_array_equal(qmax, qmin)
    assert np.abs(qmax - 1.0).max() <= TOL
    nel = hmg.fine_elements(g, level)
    values = np.unique(qmax)
    print(f"{dim}D level {level}: {values.size} distinct values, 1 + {values - 1.0}")
    for qv in values:
        below = np.nextafter(qv, -np.inf)
        a, b, counts = hmg.cell_extrema(dv, g, xi, None, [below, qv])
        np.testing.assert_array_equal(a, qmax)
        np.testing.assert_array_equal(b, qmin)
        hit = qmax == qv
        assert hit.any()
        assert (counts[hit, 0] == nel).all() and (counts[hit, 1] == 0).all()
        np.testing.assert_array_equal(counts[:, 0], nel * (qmax > below))
        np.testing.assert_array_equal(counts[:, 1], nel * (qmax > qv))
    dv.close()
    g.close()
