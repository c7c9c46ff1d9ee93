"""GPU tests of the located per-cell extrema (hmg_cell_extrema_where; the located instantiations in csrc/hmg_extrema.hip and
csrc/hmg_extrema_window.hip) against hmg_cell_extrema, the CPU statement of tests/_cell_extrema_form.py, the locator and the tie
rule of include/hmg.h.

Shapes: X.perturbed_cube -- (3, 2): 48 tets on levels 2, 3, 4 (one wave); (3, 1): 6 tets on levels 5 (256 threads), 6 (512
threads; option 2: one slab) and 7 (option 1: 9 slabs); (2, 2): 8 triangles on levels 2, 5 and 8 (option 2: row bands); (2, 1): 2
triangles on level 9 (option 1) -- and (3, 10): 6 000 tets on level 2, more than the resident workgroups.  Inputs as in
tests/test_gpu_cell_extrema.py: consistent_random with default_rng(300 + level), a random xi, T.random_spd, X.gap_thresholds.
Bounds: `out` EQUAL to hmg_cell_extrema's; `where` EQUAL to the statement's argmax / argmin element in every cell whose two
largest (smallest) statement values differ by more than MARGIN = 1e-9 of the cell's largest |q| -- the statement and the device
agree to 1e-11 of the largest maximum (TOL of tests/test_gpu_cell_extrema.py), a hundred times less --, with at most one cell in
fifty left out (asserted on the statement alone; none falls out for these inputs); values recomputed at the reported element within
TOL of the largest maximum.  Ties are exact by construction (equal operands give equal bits), so their tests compare ints."""
import contextlib

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist
from homogenization_jl_amd import driver, fields
import _cell_extrema_form as X
import _cell_moments_form as F
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
MARGIN = 1e-9
OPT, WCOUNT, LCOUNT = "cell_extrema_windows", "cell_extrema_window_launches", "cell_extrema_where_launches"
# name: dim, n, finest level
GRIDS = {"cube": (3, 2, 4), "cube1": (3, 1, 7), "square": (2, 2, 8), "square1": (2, 1, 9), "cube10": (3, 10, 2),
         # ... and the same cubes unperturbed (X.perturbed_cube with amplitude 0): integer geometry, for the ties
         "ucube": (3, 2, 4), "ucube1": (3, 1, 7), "usquare": (2, 2, 8), "usquare1": (2, 1, 9)}
LDS_CASES = [("cube", 2), ("cube", 3), ("cube", 4), ("cube1", 6), ("square", 2), ("square", 5), ("square", 8)]
# every kernel family: (grid, level, option): the LDS kernels of 64, 256 and 512 threads in 2D and 3D, slabs and row bands
FAMILIES = [("ucube", 2, 0), ("ucube1", 5, 0), ("ucube1", 6, 0), ("ucube1", 6, 2), ("ucube1", 7, 1), ("usquare", 2, 0),
            ("usquare", 5, 0), ("usquare", 6, 0), ("usquare", 8, 0), ("usquare", 5, 2), ("usquare", 8, 2), ("usquare1", 9, 1)]
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
            base = X.perturbed_cube(O, dim, n, amplitude=0.0 if name.startswith("u") else 0.12)
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


def equal_ints(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.int32
    np.testing.assert_array_equal(a, b)


def valid_codes(g, level):
    mask = g.table_i32("elem_mask", level)
    nperm = 6 if g.base.dim == 3 else 2
    s, k = np.nonzero((mask[:, None] >> np.arange(nperm)[None, :]) & 1)
    return (s * 8 + k).astype(np.int32)                                # ascending


def lowest_code_element(g, level):
    """the tie rule's element where every element ties: that of the lowest valid code, from "elem_mask" and "hier2slot\""""
    mask, h2s = g.table_i32("elem_mask", level), g.table_i32("hier2slot", level)
    slot = int(np.flatnonzero(mask)[0])
    k = int(np.flatnonzero((mask[slot] >> np.arange(8)) & 1)[0])
    nodes = hmg.element_vertices(g, level, [slot * 8 + k])[0]
    assert h2s[nodes[0]] == slot
    return nodes


def check_against_statement(what, q, elements, where_max, where_min):
    """where_* against the statement's argmax / argmin element of q (Ne, nt) wherever the extremum is separated by MARGIN"""
    ne = q.shape[0]
    scale = np.abs(q).max(axis=1)
    part = np.partition(q, (0, 1, q.shape[1] - 2, q.shape[1] - 1), axis=1) if q.shape[1] > 1 else None
    left_out = 0
    for sign, where, arg in ((1, where_max, q.argmax(axis=1)), (-1, where_min, q.argmin(axis=1))):
        if part is None:
            clear = np.ones(ne, dtype=bool)
        else:
            gap = part[:, -1] - part[:, -2] if sign > 0 else part[:, 1] - part[:, 0]
            clear = gap > MARGIN * scale
        left_out += int((~clear).sum())
        want = np.sort(elements[arg], axis=1)
        got = np.sort(where, axis=1)
        bad = np.flatnonzero(clear & (got != want).any(axis=1))
        assert bad.size == 0, (what, sign, bad[:5], got[bad[:5]], want[bad[:5]])
    print(f"{what}: {left_out} of {2 * ne} extrema closer than {MARGIN:.0e} to the runner-up and left out")
    assert left_out * 50 <= 2 * ne                                     # (on the statement alone)


def value_at(v, xi, form, cells, nodes, gw):
    """q of u = xi.x + v on the elements `nodes` of `cells`, from locate's gradient weights"""
    grad = np.einsum("nk,nkd->nd", v[nodes, cells[:, None]], gw) + (0.0 if xi is None else xi)
    Q = np.broadcast_to(np.eye(grad.shape[1]), (cells.shape[0],) + (grad.shape[1],) * 2) if form is None else form[cells]
    return np.einsum("nk,nkl,nl->n", grad, Q, grad)


def check_values_and_locator(what, g, level, v, xi, form, got):
    """q recomputed on the host at the reported elements equals the extrema; the locator finds the same cell and vertex set at the
    elements' centroids"""
    qmax, qmin, _, wmax, wmin = got
    ne = qmax.shape[0]
    cells = np.arange(ne)
    scale = np.abs(qmax).max()
    for name, ext, where in (("max", qmax, wmax), ("min", qmin, wmin)):
        pts = fields.element_centroids(g, level, cells, where)
        cell, nodes, w, gw = hmg.locate(g, level, pts)
        assert (w > 0.0).all()                                         # interior points: the element's own vertices
        np.testing.assert_array_equal(cell, cells)
        np.testing.assert_array_equal(np.sort(nodes, axis=1), np.sort(where, axis=1))
        err = np.abs(value_at(v, xi, form, cells, nodes, gw) - ext).max() / scale
        print(f"{what}: {name} recomputed at the reported element within {err:.2e} of the largest maximum")
        assert err <= TOL


# ---- the old call's bits, the statement, the value, the locator ----

@pytest.mark.parametrize("name,level", LDS_CASES)
def test_same_bits_as_cell_extrema_and_the_statements_elements(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level, grad=True)
    elements = implicit.reference.levels[level - 1].elements
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    q = X.element_values(grad, xi, form)
    thr = X.gap_thresholds(q)
    n0, k0 = ctx.counter(LCOUNT), ctx.counter("cell_extrema_kernel_ns")
    for args in ((xi, form, thr), (None, None, None)):
        old = hmg.cell_extrema(dv, g, *args)
        k0 = ctx.counter("cell_extrema_kernel_ns")
        new = hmg.cell_extrema_where(dv, g, *args)
        assert ctx.counter("cell_extrema_kernel_ns") == k0 and ctx.counter("cell_extrema_where_kernel_ns") > 0
        for a, b in zip(old, new[:3]):
            assert a.shape == b.shape and a.dtype == b.dtype
            np.testing.assert_array_equal(a, b)
        assert new[3].shape == new[4].shape == (base.nelements(), base.dim + 1)
        again = hmg.cell_extrema_where(dv, g, *args)                   # the same ints in a second run
        equal_ints(new[3], again[3])
        equal_ints(new[4], again[4])
        qs = q if args[0] is not None else X.element_values(grad, None, None)
        what = f"{name} level {level}" + ("" if args[0] is not None else " (no xi, no form)")
        check_against_statement(what, qs, elements, new[3], new[4])
        check_values_and_locator(what, g, level, dv.to_host(), args[0], args[1], new)
    assert ctx.counter(LCOUNT) == n0 + 4
    dv.close()


def test_level_1_has_one_element(ctx, shapes):
    base, implicit, g, v, xi, form = shapes("cube", 1)
    dv = hmg.DeviceMatrix(g, 1).from_host(v)
    qmax, qmin, _, wmax, wmin = hmg.cell_extrema_where(dv, g, xi, form)
    np.testing.assert_array_equal(qmax, qmin)
    equal_ints(wmax, wmin)
    np.testing.assert_array_equal(np.sort(wmax, axis=1), np.broadcast_to(np.arange(4, dtype=np.int32), wmax.shape))
    dv.close()


# ---- ties ----

@pytest.mark.parametrize("name,level,opt", FAMILIES)
def test_where_every_element_ties_the_lowest_code_wins(ctx, shapes, name, level, opt):
    """v = 0 and xi != 0: every element of a cell has the same operands, xi~ and Q~.  That alone does not give them the same bits:
    the six (two) evaluations of a node are one expression in six arrangements, and the compiler fuses their products into
    multiply-adds differently (measured on the perturbed cube: the elements of one permutation agree, those of two may differ in
    the last bit) -- which hmg_cell_extrema's bits rest on and this call must not change.  So the tie is made exact: on the
    unperturbed cube J, hence M = m Jinv B^-T and Q~ = M^T Q M for an integer Q, are integer matrices, and xi~ = M^-1 xi of an
    integer xi is a multiple of 1 / m; every product and sum of the form is then exact in double precision, whatever is fused.
    Then every element of a cell has the same bits, and both locations are the element of the lowest valid code."""
    base, implicit, g, _, _, _ = shapes(name, level)
    d = base.dim
    xi = np.array([1.0, -2.0, 3.0])[:d]
    Q = np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 4.0]])[:d, :d]
    form = Q[None] + (np.arange(base.nelements()) % 3)[:, None, None] * np.eye(d)[None]
    dv = hmg.DeviceMatrix(g, level)                                    # zero-filled
    want = lowest_code_element(g, level)
    with option(ctx, opt):
        n0 = ctx.counter(WCOUNT)
        qmax, qmin, counts, wmax, wmin = hmg.cell_extrema_where(dv, g, xi, form, [0.0])
        assert ctx.counter(WCOUNT) == n0 + (1 if opt else 0)
    np.testing.assert_array_equal(qmax, qmin)
    assert (counts[:, 0] == hmg.fine_elements(g, level)).all()
    equal_ints(wmax, np.broadcast_to(want, wmax.shape).astype(np.int32))
    equal_ints(wmin, wmax)
    dv.close()


@pytest.mark.parametrize("opt", [0, 2])
def test_a_tie_of_two_elements_in_different_waves(oracle, ctx, shapes, opt):
    """3D level 6 (512 threads: 8 waves; option 2: the slab kernel, whose 16 waves take the nodes in list order).  In two cells the same random values are planted on the
    3 x 3 x 3 lattice boxes around two interior nodes A and B, everything else 0, xi = 0: every element that touches box B is a
    translate of one that touches box A with the same operands, so the maximum is held by exactly two elements with the same
    bits, and the lower code must be reported.  Separation and position are asserted on the statement and the tables."""
    base, implicit, g, _, _, form = shapes("cube1", 6)
    level, m = 6, 32
    ref = implicit.reference.levels[level - 1]
    h2s = g.table_i32("hier2slot", level)
    ijk = g.table_i32("slot_ijk", level).reshape(-1, 3)[h2s]           # lattice position of every hierarchical node
    at = {tuple(p): h for h, p in enumerate(ijk.tolist())}
    codes = valid_codes(g, level)
    code_of = {tuple(sorted(r)): int(c) for r, c in zip(hmg.element_vertices(g, level, codes).tolist(), codes)}
    rng = np.random.default_rng(17)
    v = np.zeros((implicit.nf(level), base.nelements()), order="F")
    planted = {1: ((3, 2, 2), (9, 2, 14)), 4: ((2, 5, 3), (17, 6, 2))}
    box = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    for cell, (A, B) in planted.items():
        vals = rng.standard_normal(27)
        for P in (A, B):
            assert min(P) >= 2 and sum(P) + 6 <= m                     # the box and the ring of nodes around it lie in the cell
            for o, val in zip(box, vals):
                v[at[(P[0] + o[0], P[1] + o[1], P[2] + o[2])], cell] = val
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with option(ctx, opt):
        old = hmg.cell_extrema(dv, g, None, form)
        qmax, qmin, _, wmax, wmin = hmg.cell_extrema_where(dv, g, None, form)
    np.testing.assert_array_equal(qmax, old[0])
    np.testing.assert_array_equal(qmin, old[1])
    for cell in planted:
        XT = implicit.construct_full_grid(level)[cell][ref.elements, :]
        VT = v[:, cell][ref.elements]
        grad = np.linalg.solve(XT[:, 1:, :] - XT[:, :1, :], (VT[:, 1:] - VT[:, :1])[..., None])[..., 0]
        q = X.element_values(grad[None], None, form[cell:cell + 1])[0]
        top = np.argsort(q)[-3:][::-1]
        assert abs(q[top[0]] - q[top[1]]) <= 1e-12 * q[top[0]] and q[top[1]] - q[top[2]] > MARGIN * q[top[0]]
        cands = sorted(code_of[tuple(sorted(ref.elements[e].tolist()))] for e in top[:2])
        waves = [((c >> 3) % 512) // 64 for c in cands]                 # k_cell_extrema: thread slot mod 512 takes the slot
        print(f"option {opt}, cell {cell}: the maximum is held by codes {cands}, in waves {waves} of the LDS kernel")
        assert waves[0] != waves[1]
        want = hmg.element_vertices(g, level, [cands[0]])[0]
        equal_ints(wmax[cell], want)
        assert abs(qmax[cell] - q[top[0]]) <= TOL * q[top[0]]
    # the cells nothing was planted in: q = 0 everywhere, every element ties
    rest = [c for c in range(base.nelements()) if c not in planted]
    equal_ints(wmax[rest], np.broadcast_to(lowest_code_element(g, level), (len(rest), 4)).astype(np.int32))
    dv.close()


# ---- the window kernels ----

@pytest.mark.parametrize("name,level", [("cube1", 6), ("square", 2), ("square", 5), ("square", 8)])
def test_window_kernels_report_the_elements_of_the_lds_kernels(ctx, shapes, name, level):
    base, implicit, g, v, xi, form = shapes(name, level)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    res = []
    for value in (0, 2):
        with option(ctx, value):
            n0 = ctx.counter(WCOUNT)
            res.append(hmg.cell_extrema_where(dv, g, xi, form, [1.0, 2.0]) + hmg.cell_extrema_where(dv, g))
            assert ctx.counter(WCOUNT) == n0 + value
    for a, b in zip(*res):
        assert a.shape == b.shape and a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    dv.close()


@pytest.mark.parametrize("name,level", [("cube1", 7), ("square1", 9)])
def test_cells_larger_than_the_lds(ctx, shapes, name, level):
    base, implicit, g, v, xi, form, grad = shapes(name, level, grad=True)
    elements = implicit.reference.levels[level - 1].elements
    q = X.element_values(grad, xi, form)
    thr = X.gap_thresholds(q)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    with pytest.raises(hmg._lib.HmgError, match=f"hmg_cell_extrema_where: one cell of level {level} .*does not fit the LDS") as err:
        hmg.cell_extrema_where(dv, g)
    assert OPT in str(err.value)
    with option(ctx, 1):
        n0, l0 = ctx.counter(WCOUNT), ctx.counter(LCOUNT)
        old = hmg.cell_extrema(dv, g, xi, form, thr)
        new = hmg.cell_extrema_where(dv, g, xi, form, thr)
        a0 = ctx.counter("device_allocs")
        again = hmg.cell_extrema_where(dv, g, xi, form, thr)
        assert ctx.counter("device_allocs") == a0
        assert ctx.counter(WCOUNT) == n0 + 3 and ctx.counter(LCOUNT) == l0 + 2
    for a, b in zip(old, new[:3]):
        np.testing.assert_array_equal(a, b)
    equal_ints(new[3], again[3])
    equal_ints(new[4], again[4])
    check_against_statement(f"{name} level {level}", q, elements, new[3], new[4])
    check_values_and_locator(f"{name} level {level}", g, level, v, xi, form, new)
    dv.close()


# ---- independence of the launch ----

def test_more_cells_than_resident_workgroups_and_one_cell_alone(ctx, shapes):
    base, implicit, g, v, xi, form, grad = shapes("cube10", 2, grad=True)
    assert base.nelements() == 6000 > 16 * 256
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    thr = [0.5, 2.0]
    old = hmg.cell_extrema(dv, g, xi, form, thr)
    new = hmg.cell_extrema_where(dv, g, xi, form, thr)
    for a, b in zip(old, new[:3]):
        np.testing.assert_array_equal(a, b)
    check_against_statement("6000 cells level 2", X.element_values(grad, xi, form), implicit.reference.levels[1].elements,
                            new[3], new[4])
    dv.close()
    for cell in (0, 2999, 5999):
        g1 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes[base.elements[cell]], np.arange(1, 5)[None, :]), 2)
        d1 = hmg.DeviceMatrix(g1, 2).from_host(np.asfortranarray(v[:, cell:cell + 1]))
        one = hmg.cell_extrema_where(d1, g1, xi, form[cell:cell + 1], thr)
        for a, b in zip(one, new):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a[0], b[cell])
        d1.close()
        g1.close()


# ---- NaN and inf ----

@pytest.mark.parametrize("name,level,opt", [("cube", 3, 0), ("square", 5, 0), ("square", 5, 2), ("cube1", 6, 2)])
def test_nan_and_inf(ctx, shapes, name, level, opt):
    base, implicit, g, v, xi, form = shapes(name, level)
    ne, d = base.nelements(), base.dim
    cell = ne // 2
    others = np.arange(ne) != cell
    h2s = g.table_i32("hier2slot", level)
    ijk = g.table_i32("slot_ijk", level).reshape(-1, 3)[h2s]
    elements = implicit.reference.levels[level - 1].elements
    with option(ctx, opt):
        dv = hmg.DeviceMatrix(g, level).from_host(v)
        clean = hmg.cell_extrema_where(dv, g, xi, form)
        dv.close()
        bad = np.array(v, order="F")
        bad[v.shape[0] // 2, cell] = np.nan
        dv = hmg.DeviceMatrix(g, level).from_host(bad)
        got = hmg.cell_extrema_where(dv, g, xi, form)
        dv.close()
        assert np.isnan(got[0][cell]) and np.isnan(got[1][cell])
        assert (got[3][cell] == -1).all() and (got[4][cell] == -1).all()
        for a, b in zip(got, clean):
            np.testing.assert_array_equal(a[others], b[others])
        # the cell's corner at the lattice origin belongs to one fine element: a huge value there makes that element's q +inf
        corner = int(np.flatnonzero((ijk == 0).all(axis=1))[0])
        holds = np.flatnonzero((elements == corner).any(axis=1))
        assert holds.shape == (1,)
        bad = np.array(v, order="F")
        bad[corner, cell] = 2.0 ** 530
        dv = hmg.DeviceMatrix(g, level).from_host(bad)
        got = hmg.cell_extrema_where(dv, g, xi, form)
        dv.close()
        assert np.isposinf(got[0][cell]) and np.isfinite(got[1][cell])
        np.testing.assert_array_equal(np.sort(got[3][cell]), np.sort(elements[holds[0]]))
        for a, b in zip(got, clean):
            np.testing.assert_array_equal(a[others], b[others])
        np.testing.assert_array_equal(got[1], clean[1])                # the minimum and its element are elsewhere
        equal_ints(got[4], clean[4])


# ---- other grids and arguments ----

def test_shrunk_grid(oracle, ctx):
    O = oracle
    base = X.perturbed_cube(O, 3, 2)
    level = 3
    implicit = O.ImplicitFineGrid.create(base, level)
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), level)
    rng = np.random.default_rng(11)
    v = F.consistent_random(O, implicit, level, rng)
    xi, form = rng.standard_normal(3), T.random_spd(rng, 48, 3)
    dv = hmg.DeviceMatrix(g, level).from_host(v)
    full = hmg.cell_extrema_where(dv, g, xi, form, [1.0])
    g.shrink(47, base.nodes.shape[0])
    part = hmg.cell_extrema_where(dv, g, xi, form[:47], [1.0])
    for a, b in zip(full, part):
        assert b.shape[0] == 47 and a.dtype == b.dtype
        np.testing.assert_array_equal(b, a[:47])
    dv.close()
    g.close()


@pytest.mark.parametrize("name,level,opt", [("cube", 3, 0), ("square1", 9, 1)])
def test_partitioned_grid_is_indexed_by_local_cell(ctx, shapes, name, level, opt):
    base, implicit, g1, v, xi, form = shapes(name, level)
    ne = base.nelements()
    gbase = hmg.Mesh(base.nodes, base.elements + 1)
    owner = (np.arange(ne) % 2).astype(np.int32)
    with option(ctx, opt):
        d1 = hmg.DeviceMatrix(g1, level).from_host(v)
        whole = hmg.cell_extrema_where(d1, g1, xi, form, [1.0])
        d1.close()
        for rank in (0, 1):
            g = hdist.PartitionedGrid(ctx, gbase, level, owner, rank, 2)
            loc = g.local_cells
            dv = hmg.DeviceMatrix(g, level).from_host(np.asfortranarray(v[:, loc]))
            part = hmg.cell_extrema_where(dv, g, xi, form[loc], [1.0])
            for a, b in zip(part, whole):
                assert a.dtype == b.dtype
                np.testing.assert_array_equal(a, b[loc])
            dv.close()
            g.close()


def test_bad_arguments_are_refused(shapes, ctx):
    base, implicit, g, v, xi, form = shapes("cube", 2)
    dv = hmg.DeviceMatrix(g, 2).from_host(v)
    L = hmg._lib
    lib = L.load()
    out = np.zeros((g.ncells(), 3))
    where = np.full((g.ncells(), 2, 4), 7, dtype=np.int32)
    po, pw = out.ctypes.data_as(L.p_f64), where.ctypes.data_as(L.p_i32)
    n0 = ctx.counter(LCOUNT)
    assert lib.hmg_cell_extrema_where(g.h, dv.h, None, None, 0, None, po, None) != 0
    assert "hmg_cell_extrema_where: null where" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema_where(g.h, dv.h, None, None, 0, None, None, pw) != 0
    assert "hmg_cell_extrema_where: null output" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema_where(g.h, dv.h, None, None, 1, None, po, pw) != 0
    assert "hmg_cell_extrema_where: null thresholds" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema_where(g.h, None, None, None, 0, None, po, pw) != 0
    assert "hmg_cell_extrema_where: null vector" in lib.hmg_last_error().decode()
    gh = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: .*without a device context"):
        hmg.cell_extrema_where(dv, gh)
    gh.close()
    g2 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(base.nodes, base.elements + 1), 2)
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: .*another grid"):
        hmg.cell_extrema_where(dv, g2)
    g2.close()
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: 9 thresholds"):
        hmg.cell_extrema_where(dv, g, thresholds=np.arange(9.0))
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: threshold 1 is not finite"):
        hmg.cell_extrema_where(dv, g, thresholds=[1.0, np.nan])
    bad = form.copy()
    bad[5, 1, 1] = np.inf
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: the form of cell 5 is not finite"):
        hmg.cell_extrema_where(dv, g, form=bad)
    with pytest.raises(L.HmgError, match="hmg_cell_extrema_where: xi is not finite"):
        hmg.cell_extrema_where(dv, g, xi=[0.0, np.nan, 0.0])
    assert ctx.counter(LCOUNT) == n0 and (where == 7).all()            # nothing launched, nothing written
    # ... and the next call succeeds
    new = hmg.cell_extrema_where(dv, g, xi, form)
    for a, b in zip(hmg.cell_extrema(dv, g, xi, form), new[:3]):
        np.testing.assert_array_equal(a, b)
    assert ctx.counter(LCOUNT) == n0 + 1
    dv.close()


def test_allocations_settle(shapes, ctx):
    base, implicit, g, v, xi, form = shapes("cube", 4)
    dv = hmg.DeviceMatrix(g, 4).from_host(v)
    hmg.cell_extrema_where(dv, g, xi, form, [1.0, 2.0])
    n0, l0 = ctx.counter("device_allocs"), ctx.counter(LCOUNT)
    for _ in range(3):
        hmg.cell_extrema_where(dv, g, xi, form, [1.0, 2.0])
    assert ctx.counter("device_allocs") == n0
    assert ctx.counter(LCOUNT) == l0 + 3
    assert ctx.counter("cell_extrema_where_kernel_ns") > 0
    dv.close()


# ---- the Dirichlet driver ----

def test_driver_uniform_medium_reports_the_tie_rules_element(ctx):
    xi = np.array([1.0, 2.0])               # (integers on an integer mesh: every element's value is exact, see the ties above)
    kw = dict(ctx=ctx, sigma_grid=np.full((3, 3, 2), 3.0), extrema=True, thresholds=[0.5, 2.0], fields=True)
    plain = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, **kw)
    r = driver.dirichlet_homogenization(3, hmg.Tri64, 2, xi, locations=True, **kw)
    new = {"peak_location", "min_location", "hot_spots"}
    assert set(r) == set(plain) | new and not (set(plain) & new)
    for k in plain:                                                   # every other entry keeps its bits
        if k != "base":
            np.testing.assert_array_equal(np.asarray(plain[k]), np.asarray(r[k]))
    gh = hmg.ImplicitFineGrid(None, r["base"], 3)
    ne = gh.ncells()
    want = fields.element_centroids(gh, 3, np.arange(ne), np.broadcast_to(lowest_code_element(gh, 3), (ne, 3)))
    np.testing.assert_array_equal(r["peak_location"], want)
    np.testing.assert_array_equal(r["min_location"], want)
    order = np.lexsort((np.arange(ne), -r["peak_energy_density"]))[:10]
    np.testing.assert_array_equal(r["hot_spots"]["cell"], order)
    np.testing.assert_array_equal(r["hot_spots"]["point"], want[order])
    gh.close()


def test_driver_checkerboard_hot_spots(ctx):
    xi = np.array([0.6, 0.8])
    levels = 4
    r = driver.dirichlet_homogenization(4, hmg.Tri64, levels - 1, xi, ctx=ctx, seed=2, values=(1.0, 100.0), fields=True,
                                        extrema=True, locations=True)
    h = r["hot_spots"]
    ne = r["volumes"].shape[0]
    assert r["peak_location"].shape == r["min_location"].shape == (ne, 2)
    assert h["cell"].shape == (10,) and h["point"].shape == (10, 2)
    order = np.lexsort((np.arange(ne), -r["peak_energy_density"]))[:10]
    np.testing.assert_array_equal(h["cell"], order)
    np.testing.assert_array_equal(h["value"], r["peak_energy_density"][order])
    np.testing.assert_array_equal(h["point"], r["peak_location"][order])
    gh = hmg.ImplicitFineGrid(None, r["base"], levels)
    cell, _, w, _ = hmg.locate(gh, levels, h["point"])
    np.testing.assert_array_equal(cell, h["cell"])
    assert (w > 0.0).all()
    gh.close()
    err = np.abs(h["sampled"] - h["value"]).max() / r["peak_energy_density"].max()
    print(f"checkerboard of contrast 100: hot spots {h['cell'].tolist()}, peak / mean up to {h['value'][0] / r['energy_form']:.2f}; "
          f"sampled at the spot within {err:.2e} of the largest peak")
    assert err <= TOL
