"""GPU tests of the cell loop of the three LDS-resident per-cell kernels -- k_cell_pair_moments in its one- and two-vector forms
(hmg_cell_moments, hmg_cell_pair_moments; csrc/hmg_fields.hip) and k_cell_extrema (hmg_cell_extrema; csrc/hmg_extrema.hip) -- on
grids with MORE CELLS THAN WORKGROUPS, at every thread count.  Each kernel launches at most min(2048 / NT, 16) workgroups per CU
and a workgroup walks the cells blockIdx.x, blockIdx.x + gridDim.x, ...: on such a grid every workgroup overwrites its LDS image
and reuses its reduction slots for a second cell, which no smaller grid makes it do.

The grid is hypercube(dim, n), unperturbed: cell e is an exact translate of cell e % ncls of hypercube(dim, 1) (ncls = 6 in 3D,
2 in 2D; asserted on the host).  Column e is 2^k_e base[:, e % ncls] with k_e drawn per cell from -3..3: neighbouring turns of one
workgroup hold different data, and scaling by a power of two is exact, so that the large grid's results are the ONE-CUBE grid's
DEVICE results scaled, BIT FOR BIT (mean by s, Gram tensor, extrema by s^2, pair moment by s t; counts at thresholds t: the
one-cube counts at t / s^2).  The one-cube device results are held against the CPU statements of tests/_cell_moments_form.py,
_cell_pair_moments_form.py and _cell_extrema_form.py at the project's 1e-11 in the same test: the chain ends at the reference.
Where the cell's row reaches the kernel (extrema with xi and a form per cell) the comparison is with the statement itself.
n is the smallest with ncells > min(2048 / NT, 16) * CUs, an upper bound of the launch's grid whatever the LDS allows; asserted,
not skipped.  On 256 CUs: 3D levels 4, 5, 6 on n = 9, 7, 6 (4 374, 2 058, 1 296 cells), 2D levels 5, 6, 8 on n = 46, 33, 23 (4 232,
2 178, 1 058 cells); the largest vector is 71 MB.
The poison runs put a NaN into the columns of a seeded 2 % of the cells: those cells report NaN, every other cell the bits of the
clean run -- nothing leaks from one turn of a workgroup into the next."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
import _cell_extrema_form as X
import _cell_moments_form as F
import _cell_pair_moments_form as P
import _tensor_sigma_form as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
MARGIN = 1e-9
SHAPES = [(3, 4), (3, 5), (3, 6), (2, 5), (2, 6), (2, 8)]              # dim, level: 64, 256, 512 threads each
SCALES = 2.0 ** np.arange(-3, 4)
QUANT8 = (0.02, 0.10, 0.30, 0.50, 0.70, 0.90, 0.97, 0.995)
_cache = {}


def threads(nf):
    """the launch rule of both kernels (launch_dim)"""
    return 64 if nf <= 256 else 256 if nf <= 4096 else 512


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Shape:
    pass


@pytest.fixture(scope="module")
def shapes(oracle, ctx):
    """per (dim, level): the one-cube grid and the large grid on the device, the base columns, the scales, the large vectors
    (uploaded once, read only)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def get(dim, level):
        O = oracle
        if (dim, level) in _cache:
            return _cache[(dim, level)]
        s = Shape()
        s.dim, s.level = dim, level
        s.one = O.hypercube(dim, 1)
        s.ncls = s.one.nelements()
        s.implicit1 = O.ImplicitFineGrid.create(s.one, level)
        s.nf = s.implicit1.nf(level)
        s.bound = min(2048 // threads(s.nf), 16)                       # the launch's cap of workgroups per CU
        n = 1
        while s.ncls * n ** dim <= s.bound * cus:
            n += 1
        s.big = O.hypercube(dim, n)
        s.ne = s.big.nelements()
        assert s.ne > s.bound * cus                                    # more cells than workgroups, whatever the LDS allows
        s.cls = np.arange(s.ne) % s.ncls
        # cell e is a translate of cell e % ncls of the one cube, to the last bit
        Pb, Po = s.big.nodes[s.big.elements], s.one.nodes[s.one.elements]
        np.testing.assert_array_equal(Pb[:, 1:] - Pb[:, :1], (Po[:, 1:] - Po[:, :1])[s.cls])
        rng = np.random.default_rng(1000 * dim + level)
        s.base_v, s.base_w = (np.asfortranarray(rng.standard_normal((s.nf, s.ncls))) for _ in range(2))
        s.kv, s.kw = rng.integers(0, 7, s.ne), rng.integers(0, 7, s.ne)
        s.sv, s.sw = SCALES[s.kv], SCALES[s.kw]
        s.g1 = hmg.ImplicitFineGrid(ctx, hmg.Mesh(s.one.nodes, s.one.elements + 1), level)
        s.g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(s.big.nodes, s.big.elements + 1), level)
        assert s.g.ncells() == s.ne and s.g.nf(level) == s.nf
        s.v = np.asfortranarray(s.base_v[:, s.cls] * s.sv[None, :])
        s.w = np.asfortranarray(s.base_w[:, s.cls] * s.sw[None, :])
        s.d1v, s.d1w = hmg.DeviceMatrix(s.g1, level).from_host(s.base_v), hmg.DeviceMatrix(s.g1, level).from_host(s.base_w)
        s.dv, s.dw = hmg.DeviceMatrix(s.g, level).from_host(s.v), hmg.DeviceMatrix(s.g, level).from_host(s.w)
        lay = s.g.table_i32("layout", level)
        s.ncorner, s.nint, s.off_int = int(lay[2]), int(lay[7]), int(lay[10])
        assert s.ncorner == dim + 1 and s.nint > 0 and s.off_int + s.nint == s.nf
        h2s = s.g.table_i32("hier2slot", level)                        # (a host vector's rows are hierarchical, the device's slots)
        s.rows_vertex, s.rows_interior = np.flatnonzero(h2s < s.ncorner), np.flatnonzero(h2s >= s.off_int)
        assert s.rows_vertex.size == s.ncorner and s.rows_interior.size == s.nint
        # the statement's element values of the base columns (form and xi None), their thresholds
        s.grad1 = X.element_gradients(O, s.implicit1, level, s.base_v)
        s.q1 = X.element_values(s.grad1)
        for a in (s.base_v, s.base_w, s.v, s.w, s.grad1, s.q1):
            a.setflags(write=False)
        print(f"{dim}D level {level}: {s.nf} nodes, {threads(s.nf)} threads, hypercube({dim}, {n}): {s.ne} cells > "
              f"{s.bound} x {cus} CUs")
        _cache[(dim, level)] = s
        return s
    yield get
    for s in _cache.values():
        for o in (s.d1v, s.d1w, s.dv, s.dw, s.g1, s.g):
            o.close()
    _cache.clear()


def poison(s, rng, columns):
    """copies of `columns` with one NaN in the column of a seeded 2 % of the cells -- at a vertex slot in half of them, at a slot of
    the cell interior in the others -- each poisoned cell in ONE of the copies; returns the copies and the poisoned cells"""
    cells = np.sort(rng.choice(s.ne, max(4, s.ne // 50), replace=False))
    out = [np.array(c, order="F") for c in columns]
    for i, e in enumerate(cells):
        row = rng.choice(s.rows_vertex) if i % 2 == 0 else rng.choice(s.rows_interior)
        out[(i // 2) % len(out)][row, e] = np.nan
    return out, cells


def others_unchanged(s, cells, clean, dirty, what):
    keep = np.ones(s.ne, dtype=bool)
    keep[cells] = False
    for a, b in zip(clean, dirty):
        np.testing.assert_array_equal(a[keep], b[keep], err_msg=f"{what}: a cell next to a poisoned one changed")


@pytest.mark.parametrize("dim,level", SHAPES)
def test_moments(oracle, shapes, dim, level):
    s = shapes(dim, level)
    mean1, gram1 = hmg.cell_moments(s.d1v, s.g1)
    wm, wg = F.reference_form(oracle, s.implicit1, level, s.base_v)
    e1, e2 = np.abs(mean1 - wm).max() / np.abs(wm).max(), np.abs(gram1 - wg).max() / np.abs(wg).max()
    print(f"{dim}D level {level}: one cube against the statement, mean {e1:.2e} gram {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    mean, gram = hmg.cell_moments(s.dv, s.g)
    bad = int((mean != s.sv[:, None] * mean1[s.cls]).any(axis=1).sum()), \
        int((gram != (s.sv ** 2)[:, None, None] * gram1[s.cls]).any(axis=(1, 2)).sum())
    print(f"{dim}D level {level}: {bad[0]} / {bad[1]} of {s.ne} cells differ from the scaled one-cube mean / gram")
    np.testing.assert_array_equal(mean, s.sv[:, None] * mean1[s.cls])
    np.testing.assert_array_equal(gram, (s.sv ** 2)[:, None, None] * gram1[s.cls])
    # poison
    (pv,), cells = poison(s, np.random.default_rng(7), [s.v])
    dp = hmg.DeviceMatrix(s.g, level).from_host(pv)
    mean_p, gram_p = hmg.cell_moments(dp, s.g)
    dp.close()
    others_unchanged(s, cells, (mean, gram), (mean_p, gram_p), "moments")
    assert np.isnan(gram_p[cells]).all()


@pytest.mark.parametrize("dim,level", SHAPES)
def test_pair_moments(oracle, shapes, dim, level):
    s = shapes(dim, level)
    S1 = hmg.cell_pair_moments(s.d1v, s.d1w, s.g1)
    want = P.reference_form(oracle, s.implicit1, level, s.base_v, s.base_w)[2]
    sc = P.scale(F.reference_form(oracle, s.implicit1, level, s.base_v)[1], F.reference_form(oracle, s.implicit1, level, s.base_w)[1])
    e = np.abs(S1 - want).max() / sc
    print(f"{dim}D level {level}: one cube against the statement, pair {e:.2e}")
    assert e <= TOL
    S = hmg.cell_pair_moments(s.dv, s.dw, s.g)
    expect = (s.sv * s.sw)[:, None, None] * S1[s.cls]
    print(f"{dim}D level {level}: {int((S != expect).any(axis=(1, 2)).sum())} of {s.ne} cells differ from the scaled one-cube pair")
    np.testing.assert_array_equal(S, expect)
    # poison: v in some cells, w in others
    (pv, pw), cells = poison(s, np.random.default_rng(8), [s.v, s.w])
    assert np.isnan(pv).any() and np.isnan(pw).any() and not (np.isnan(pv).any(axis=0) & np.isnan(pw).any(axis=0)).any()
    dpv, dpw = hmg.DeviceMatrix(s.g, level).from_host(pv), hmg.DeviceMatrix(s.g, level).from_host(pw)
    S_p = hmg.cell_pair_moments(dpv, dpw, s.g)
    dpv.close()
    dpw.close()
    others_unchanged(s, cells, (S,), (S_p,), "pair moments")
    assert np.isnan(S_p[cells]).all()


def one_cube_extrema(s, thr):
    """the one-cube device run with thresholds thr, held against the statement; returns it"""
    if len(thr):
        mg = X.margin(s.q1, thr)
        print(f"{s.dim}D level {s.level}: no element within {mg:.2e} of a threshold (relative to the largest value)")
        assert mg > MARGIN                                             # (on the statement alone)
    wmax, wmin, wcounts = X.extrema(s.q1, thr)
    qmax1, qmin1, counts1 = hmg.cell_extrema(s.d1v, s.g1, None, None, thr)
    e1, e2 = np.abs(qmax1 - wmax).max() / wmax.max(), np.abs(qmin1 - wmin).max() / wmax.max()
    print(f"{s.dim}D level {s.level}: one cube against the statement, max {e1:.2e} min {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    np.testing.assert_array_equal(counts1, wcounts)
    return qmax1, qmin1, counts1


def scaled_counts(s, thr):
    """what the large grid's counts must be: per scale the one-cube DEVICE counts at thr / s^2"""
    want = np.zeros((s.ne, len(thr)), dtype=np.int64)
    for k, sc in enumerate(SCALES):
        c1 = hmg.cell_extrema(s.d1v, s.g1, None, None, np.asarray(thr) / sc ** 2)[2]
        sel = s.kv == k
        want[sel] = c1[s.cls[sel]]
    return want


NTHR = [(d, l, n) for d, l in SHAPES for n in ((0, 4, 8) if (d, l) in ((3, 4), (2, 5)) else (4,))]


@pytest.mark.parametrize("dim,level,nthr", NTHR)
def test_extrema(shapes, dim, level, nthr):
    s = shapes(dim, level)
    thr = np.zeros(0) if nthr == 0 else X.gap_thresholds(s.q1) if nthr == 4 else X.gap_thresholds(s.q1, quantiles=QUANT8)
    assert thr.shape == (nthr,)
    qmax1, qmin1, _ = one_cube_extrema(s, thr)
    qmax, qmin, counts = hmg.cell_extrema(s.dv, s.g, None, None, thr)
    assert counts.shape == (s.ne, nthr)
    s2 = s.sv ** 2
    print(f"{dim}D level {level}, {nthr} thresholds: {int((qmax != s2 * qmax1[s.cls]).sum())} / {int((qmin != s2 * qmin1[s.cls]).sum())}"
          f" of {s.ne} cells differ from the scaled one-cube maximum / minimum")
    np.testing.assert_array_equal(qmax, s2 * qmax1[s.cls])
    np.testing.assert_array_equal(qmin, s2 * qmin1[s.cls])
    if nthr:
        want = scaled_counts(s, thr)
        print(f"{dim}D level {level}, {nthr} thresholds: counts differ in {int((counts != want).sum())} of {counts.size}")
        np.testing.assert_array_equal(counts, want)
    if nthr != 4:
        return
    # poison: NaN extrema in the poisoned cells (the rule of include/hmg.h), counts that only lose elements
    (pv,), cells = poison(s, np.random.default_rng(9), [s.v])
    dp = hmg.DeviceMatrix(s.g, level).from_host(pv)
    qmax_p, qmin_p, counts_p = hmg.cell_extrema(dp, s.g, None, None, thr)
    dp.close()
    others_unchanged(s, cells, (qmax, qmin, counts), (qmax_p, qmin_p, counts_p), "extrema")
    assert np.isnan(qmax_p[cells]).all() and np.isnan(qmin_p[cells]).all()
    assert (counts_p[cells] <= counts[cells]).all() and (counts_p[cells] >= 0).all()


@pytest.mark.parametrize("dim,level", SHAPES)
def test_extrema_with_xi_and_a_form_per_cell(oracle, shapes, dim, level):
    """the cell's row (Q~, xi~) does reach the kernel: against the statement, on the ncls base cells at the 7 scales"""
    s = shapes(dim, level)
    rng = np.random.default_rng(50 + level)
    xi = rng.standard_normal(dim)
    form = T.random_spd(rng, s.ne, dim)
    grads = np.stack([X.element_gradients(oracle, s.implicit1, level, np.asfortranarray(s.base_v * sc)) for sc in SCALES])
    wmax, wmin = np.empty(s.ne), np.empty(s.ne)
    for e0 in range(0, s.ne, 64):                                      # (in pieces: the element values of all cells at once are 1 GB)
        sl = slice(e0, min(e0 + 64, s.ne))
        q = X.element_values(grads[s.kv[sl], s.cls[sl]], xi, form[sl])
        wmax[sl], wmin[sl] = q.max(axis=1), q.min(axis=1)
    scale = wmax.max()
    lo, hi = 0.5 * wmin.min(), 2.0 * wmax.max()
    assert 0.0 < lo < wmin.min() and np.isfinite(hi)
    qmax, qmin, counts = hmg.cell_extrema(s.dv, s.g, xi, form, [lo, hi])
    e1, e2 = np.abs(qmax - wmax).max() / scale, np.abs(qmin - wmin).max() / scale
    print(f"{dim}D level {level}: xi and a form per cell, max {e1:.2e} min {e2:.2e} of the largest maximum {scale:.3e}")
    assert e1 <= TOL and e2 <= TOL
    # a threshold below the minimum counts every fine element, one above the maximum none
    assert (counts[:, 0] == hmg.fine_elements(s.g, level)).all()
    assert (counts[:, 1] == 0).all()
