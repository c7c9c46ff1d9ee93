"""GPU tests of the per-cell extrema of cells larger than the LDS (context option "cell_extrema_windows",
csrc/hmg_extrema_window.hip: k_cell_extrema_slab for 3D level 7, k_cell_extrema_rows for 2D levels 9-11) against the CPU statement
of tests/_cell_extrema_form.py (pinned by tests/test_cell_extrema_statement.py).

Shapes: the smallest with several slabs / bands, X.perturbed_cube: (3, 1) on level 7 (6 cells, 9 slabs), (2, 2) on level 9 (8
cells), (2, 1) on levels 10 and 11 (2 cells; level 11: rows of 1 025 nodes, wider than the workgroup).  The same grids carry the
levels of the kernel-against-kernel check of option value 2: 3D level 6 (one slab), 2D levels 2 (m = 2: no interior), 3, 4 and 8
(a single band).  Inputs as in tests/test_gpu_cell_extrema.py: consistent_random with default_rng(300 + level), a random xi,
T.random_spd, X.gap_thresholds.
Bounds: maxima and minima within 1e-11 of the largest statement maximum over the cells, counts EQUAL, after an assertion on the
statement alone that no element lies within MARGIN = 1e-9 of the largest value of a threshold (on the CPU, at exactly these shapes:
the statement and an independent successive-difference transcription agree to 4.4e-13 or better and the margin against the four gap
thresholds is 1.9e-8 or more).  Where two kernels serve one level -- option 2 against option 0 -- the results are compared bit for
bit: maxima, minima and counts do not depend on order, and both kernels evaluate a node with one function.
The context is this module's own; the option is at its default 0 between the tests."""
import contextlib

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist
from homogenization_jl_amd import driver
import _cell_extrema_form as X
import _cell_moments_form as F
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
MARGIN = 1e-9
OPT, COUNTER = "cell_extrema_windows", "cell_extrema_window_launches"
# name: dim, n, finest level
GRIDS = {"cube7": (3, 1, 7), "square9": (2, 2, 9), "square10": (2, 1, 10), "square11": (2, 1, 11)}
LARGE = [("cube7", 7), ("square9", 9), ("square10", 10), ("square11", 11)]
FITTING = [("cube7", 6), ("square9", 2), ("square9", 3), ("square9", 4), ("square9", 8)]
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    assert c.counter(OPT) == 0
    yield c
    c.close()


@contextlib.contextmanager
def option(ctx, value):
    prev = ctx.counter(OPT)
    ctx.set_option(OPT, value)
    try:
        yield
    finally:
        ctx.set_option(OPT, prev)


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per grid: perturbed oracle mesh, implicit grid, device grid; per (grid, level): a consistent random vector, xi, an SPD form;
    per (grid, level, "grad"): the statement's element gradients -- computed once, shared, never changed"""
    def get(name, level, grad=False):
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
        if grad:
            if (name, level, "grad") not in _cache:
                gr = X.element_gradients(O, implicit, level, out[3])
                gr.setflags(write=False)
                _cache[(name, level, "grad")] = gr
            out += (_cache[(name, level, "grad")],)
        return out
    yield get
    for k, val in list(_cache.items()):
        if isinstance(k, str):
            val[2].close()
    _cache.clear()


def check(got, q, thr, what):
    """got = (qmax, qmin, counts) of the device against the statement's element values q and thresholds thr"""
    wmax, wmin, wcounts = X.extrema(q, thr)
    scale = np.abs(wmax).max()
    if len(thr):
        mg = X.margin(q, thr)
        print(f"{what}: no element within {mg:.2e} of a threshold (relative to the largest value)")
        assert mg > MARGIN                                             # (on the statement alone)
    qmax, qmin, counts = got
    e1, e2 = np.abs(qmax - wmax).max() / scale, np.abs(qmin - wmin).max() / scale
    print(f"{what}: max {e1:.2e} min {e2:.2e} of the largest maximum {scale:.3e}; counts differ in "
          f"{int((counts != wcounts).sum())} of {counts.size}")
    assert qmax.shape == wmax.shape and qmin.shape == wmin.shape and counts.shape == wcounts.shape
    assert e1 <= TOL and e2 <= TOL
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(counts, wcounts)


def equal_bits(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)


# ---- option 1 against the statement ----

@pytest.mark.parametrize("name,level", LARGE)
def test_device_against_the_statement(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level, grad=True)
    q = X.element_values(grad, xi, form)
    assert q.shape[1] == hmg.fine_elements(g, level)
    thr = X.gap_thresholds(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with option(ctx, 1):
        n0 = ctx.counter(COUNTER)
        got = hmg.cell_extrema(dv, g, xi, form, thr)
        assert ctx.counter(COUNTER) == n0 + 1
        assert ctx.counter("cell_extrema_kernel_ns") > 0
        check(got, q, thr, f"{name} level {level}")
        # the same bits in a second run, and no allocation in it
        a0 = ctx.counter("device_allocs")
        again = hmg.cell_extrema(dv, g, xi, form, thr)
        assert ctx.counter(COUNTER) == n0 + 2
        assert ctx.counter("device_allocs") == a0
        equal_bits(got, again)
    dv.close()


@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_without_form_without_xi_and_eight_thresholds(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level, grad=True)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with option(ctx, 1):
        n0 = ctx.counter(COUNTER)
        q = X.element_values(grad, xi, None)
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, xi, None, thr), q, thr, f"{name} level {level} form None")
        q = X.element_values(grad, None, form)
        thr = X.gap_thresholds(q)
        check(hmg.cell_extrema(dv, g, None, form, thr), q, thr, f"{name} level {level} xi None")
        q = X.element_values(grad, xi, form)
        thr = X.gap_thresholds(q, quantiles=(0.02, 0.10, 0.30, 0.50, 0.70, 0.90, 0.97, 0.995))
        assert thr.shape == (8,)
        check(hmg.cell_extrema(dv, g, xi, form, thr), q, thr, f"{name} level {level} eight thresholds")
        got = hmg.cell_extrema(dv, g, xi, form)
        assert got[2].shape == (base.nelements(), 0)
        check(got, q, [], f"{name} level {level} no thresholds")
        assert ctx.counter(COUNTER) == n0 + 4
    dv.close()


@pytest.mark.parametrize("name,level", LARGE)
def test_linear_field_and_far_thresholds(oracle, ctx, shapes, name, level):
    base, implicit, g, _, xi, form = shapes(name, level)
    gvec = np.array([0.7, -1.3, 0.45])[:base.dim]
    dv = hmg.DeviceMatrix(g, level).from_host(F.linear_interpolant(oracle, implicit, level, gvec))
    want = np.einsum("k,ekl,l->e", xi + gvec, form, xi + gvec)
    with option(ctx, 1):
        qmax, qmin, counts = hmg.cell_extrema(dv, g, xi, form, [0.5 * want.min(), 2.0 * want.max()])
    e1, e2 = np.abs(qmax - want).max() / want.max(), np.abs(qmin - want).max() / want.max()
    print(f"{name} level {level}: linear field, max {e1:.2e} min {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    # a threshold below the minimum counts every fine element, one above the maximum none
    assert (counts[:, 0] == hmg.fine_elements(g, level)).all()
    assert (counts[:, 1] == 0).all()
    dv.close()


# ---- two kernels on one level: the same bits ----

@pytest.mark.parametrize("name,level", FITTING)
def test_window_kernels_give_the_bits_of_the_lds_kernel(ctx, shapes, name, level):
    """option value 2 sends a level that fits the LDS through the window kernels; value 1 leaves it to k_cell_extrema"""
    base, implicit, g, v, xi, form = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    # thresholds between the smallest minimum and the largest maximum (equal bits of the values give equal counts wherever they lie)
    qmax, qmin, _ = hmg.cell_extrema(dv, g, xi, form)
    thr = np.linspace(qmin.min(), qmax.max(), 10)[1:9]
    res, launches = [], []
    for value in (0, 1, 2):
        with option(ctx, value):
            n0 = ctx.counter(COUNTER)
            res.append((hmg.cell_extrema(dv, g, xi, form, thr), hmg.cell_extrema(dv, g, None, None, thr[:3]),
                        hmg.cell_extrema(dv, g, xi, form)))
            launches.append(ctx.counter(COUNTER) - n0)
    total = base.nelements() * hmg.fine_elements(g, level)
    print(f"{name} level {level}: window launches at option 0, 1, 2: {launches}; counts at option 0 {res[0][0][2].sum(axis=0)} of {total}")
    assert launches == [0, 0, 3]
    assert 0 < res[0][0][2][:, -1].sum() and res[0][0][2][:, 0].sum() < total                # (the thresholds separate something)
    for a0, a1, a2 in zip(*res):
        equal_bits(a0, a1)
        equal_bits(a0, a2)
    dv.close()


# ---- NaN and inf ----

def cell_values(O, implicit, level, cell, column, xi, form):
    """the statement's element values of ONE cell with `column` in its place (X.element_gradients on that cell alone)"""
    ref = implicit.reference.levels[level - 1]
    XT = implicit.construct_full_grid(level)[cell][ref.elements, :]
    D = XT[:, 1:, :] - XT[:, :1, :]
    VT = column[ref.elements]
    grad = np.linalg.solve(D, (VT[:, 1:] - VT[:, :1])[..., None])[..., 0]
    return X.element_values(grad[None], xi, None if form is None else form[cell:cell + 1])[0]


@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_nan_and_inf(oracle, ctx, shapes, name, level):
    """a NaN at one interior slot of one cell, and separately at one surface slot (the last one in storage order: a face node in
    3D, an edge node in 2D), makes that cell's extrema NaN and leaves the other cells' bits; the counts are the statement's q > t
    with NaN comparing false.  An infinite VALUE is a value: the column HUGE * (i + j + k) of tests/test_gpu_cell_fields_edges.py
    gives q_T = +inf on every element of the cell without any inf - inf."""
    base, implicit, g, v, xi, form, grad = shapes(name, level, grad=True)
    ne = base.nelements()
    cell = ne // 2
    q = X.element_values(grad, xi, form)
    thr = X.gap_thresholds(q)
    lay, h2s = g.table_i32("layout", level), g.table_i32("hier2slot", level)
    off_int = int(lay[10])
    rows = {"interior": int(np.flatnonzero(h2s >= off_int)[-1]), "surface": int(np.flatnonzero(h2s == off_int - 1)[0])}
    others = np.arange(ne) != cell
    with option(ctx, 1):
        dv = hmg.DeviceMatrix(g, level).from_host(v)
        clean = hmg.cell_extrema(dv, g, xi, form, thr)
        dv.close()
        for case, row in rows.items():
            bad = np.array(v, order="F")
            bad[row, cell] = np.nan
            qb = q.copy()
            with np.errstate(invalid="ignore"):
                qb[cell] = cell_values(oracle, implicit, level, cell, bad[:, cell], xi, form)
                nan_el = np.isnan(qb[cell])
                assert 0 < nan_el.sum() < nan_el.size
                np.testing.assert_array_equal(qb[cell][~nan_el], q[cell][~nan_el])
                wmax, wmin, wcounts = X.extrema(qb, thr)
            dv = hmg.DeviceMatrix(g, level).from_host(bad)
            qmax, qmin, counts = hmg.cell_extrema(dv, g, xi, form, thr)
            dv.close()
            print(f"{name} level {level}, NaN at a {case} slot: cell {cell} max {qmax[cell]} min {qmin[cell]} counts {counts[cell]} "
                  f"(statement {wcounts[cell]}; {int(nan_el.sum())} of {nan_el.size} elements NaN)")
            assert np.isnan(qmax[cell]) and np.isnan(qmin[cell])
            np.testing.assert_array_equal(counts, wcounts)
            for a, b in zip((qmax, qmin), clean[:2]):
                np.testing.assert_array_equal(a[others], b[others])
        # an infinite value
        huge = 2.0 ** 530
        lattice = np.rint(implicit.reference.levels[level - 1].nodes * 2 ** (level - 1))
        bad = np.array(v, order="F")
        bad[:, cell] = huge * lattice.sum(axis=1)
        q0 = X.element_values(grad)
        with np.errstate(over="ignore"):
            qc = cell_values(oracle, implicit, level, cell, bad[:, cell], None, None)
        assert np.isposinf(qc).all()
        thr0 = X.gap_thresholds(q0[others])
        assert X.margin(q0[others], thr0) > MARGIN
        dv = hmg.DeviceMatrix(g, level).from_host(bad)
        qmax, qmin, counts = hmg.cell_extrema(dv, g, None, None, thr0)
        dv.close()
        print(f"{name} level {level}, infinite values: cell {cell} max {qmax[cell]} min {qmin[cell]} counts {counts[cell]}")
        assert np.isposinf(qmax[cell]) and np.isposinf(qmin[cell])
        assert (counts[cell] == hmg.fine_elements(g, level)).all()
        wmax, wmin, wcounts = X.extrema(q0[others], thr0)
        scale = wmax.max()
        assert np.abs(qmax[others] - wmax).max() <= TOL * scale and np.abs(qmin[others] - wmin).max() <= TOL * scale
        np.testing.assert_array_equal(counts[others], wcounts)


# ---- partitioned grids ----

@pytest.mark.parametrize("name,level", [("cube7", 7), ("square9", 9)])
def test_partitioned_grid_gives_the_rows_of_the_whole_grid(ctx, shapes, name, level):
    base, implicit, g1, v, xi, form = shapes(name, level)
    ne = base.nelements()
    assert ne == (6 if name == "cube7" else 8)
    gbase = hmg.Mesh(base.nodes, base.elements + 1)
    owner = (np.arange(ne) % 2).astype(np.int32)
    thr = np.array([0.5, 2.0]) * float(np.einsum("k,ekl,l->e", xi, form, xi).mean())
    with option(ctx, 1):
        d1 = hmg.DeviceMatrix(g1, level).from_host(v)
        whole = hmg.cell_extrema(d1, g1, xi, form, thr)
        d1.close()
        for rank in (0, 1):
            g = hdist.PartitionedGrid(ctx, gbase, level, owner, rank, 2)
            loc = g.local_cells
            np.testing.assert_array_equal(loc, np.flatnonzero(owner == rank))
            dv = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v[:, loc]))
            n0 = ctx.counter(COUNTER)
            part = hmg.cell_extrema(dv, g, xi, form[loc], thr)
            assert ctx.counter(COUNTER) == n0 + 1
            equal_bits(part, tuple(a[loc] for a in whole))
            dv.close()
            g.close()


# ---- the option ----

def test_option_0_refuses_and_names_the_option(ctx, shapes):
    base, implicit, g, v, xi, form = shapes("cube7", 7)
    dv = hmg.DeviceMatrix(g, 7).from_host(v)
    assert ctx.counter(OPT) == 0
    n0 = ctx.counter(COUNTER)
    with pytest.raises(hmg._lib.HmgError, match="hmg_cell_extrema: one cell of level 7 .*does not fit the LDS") as err:
        hmg.cell_extrema(dv, g)
    assert OPT in str(err.value)
    assert ctx.counter(COUNTER) == n0
    with pytest.raises(hmg._lib.HmgError, match="0, 1 or 2"):
        ctx.set_option(OPT, 3)
    with pytest.raises(hmg._lib.HmgError, match="0, 1 or 2"):
        ctx.set_option(OPT, -1)
    assert ctx.counter(OPT) == 0
    # ... and the moments' option has no say
    prev = ctx.counter("cell_moments_windows")
    ctx.set_option("cell_moments_windows", 1)
    try:
        with pytest.raises(hmg._lib.HmgError, match="does not fit the LDS"):
            hmg.cell_extrema(dv, g)
    finally:
        ctx.set_option("cell_moments_windows", prev)
    dv.close()


# ---- the Dirichlet driver ----

def test_driver_on_3d_level_7(ctx):
    kw = dict(refinements=6, ctx=ctx, extrema=True, thresholds=[1.0, 2.0], fields=True)
    ctx.set_option("cell_moments_windows", 0)
    n0, m0 = ctx.counter(COUNTER), ctx.counter("cell_moments_window_launches")
    r = driver.dirichlet_homogenization(1, hmg.Tet64, large_cells=True, **kw)
    assert ctx.counter(COUNTER) == n0 + 1 and ctx.counter("cell_moments_window_launches") == m0 + 1
    assert ctx.counter(OPT) == 0 and ctx.counter("cell_moments_windows") == 0          # both back at their previous values
    assert {"peak_energy_density", "min_energy_density", "concentration", "exceedance"} <= set(r)
    ne = r["volumes"].shape[0]
    assert r["peak_energy_density"].shape == (ne,) and r["exceedance"].shape == (ne, 2)
    dens = r["energy"] / r["volumes"]
    slack = 1e-10 * dens
    print("3D level 7: concentration up to", r["concentration"].max(), "exceedance", r["exceedance"].sum(axis=0) / r["volume"],
          "min / mean", (r["min_energy_density"] / dens).max(), "max / mean", (r["peak_energy_density"] / dens).min())
    assert (r["peak_energy_density"] + slack >= dens).all() and (dens + slack >= r["min_energy_density"]).all()
    assert (r["exceedance"] >= 0.0).all() and (r["exceedance"] <= r["volumes"][:, None] * (1 + 1e-14)).all()
    # a caller's own values survive too
    ctx.set_option(OPT, 2)
    try:
        driver.dirichlet_homogenization(1, hmg.Tet64, refinements=1, ctx=ctx, extrema=True, large_cells=True)
        assert ctx.counter(OPT) == 2 and ctx.counter("cell_moments_windows") == 0
    finally:
        ctx.set_option(OPT, 0)
    # without large_cells: the refusal, behind the solve
    with pytest.raises(hmg._lib.HmgError, match="one cell of level 7 .*does not fit the LDS"):
        driver.dirichlet_homogenization(1, hmg.Tet64, **kw)
    assert ctx.counter(OPT) == 0 and ctx.counter("cell_moments_windows") == 0
