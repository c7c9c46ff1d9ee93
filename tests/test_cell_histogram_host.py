"""Host side of the per-cell histograms (include/hmg.h: hmg_histogram_nbins, hmg_histogram_edges, hmg_histogram_bin,
hmg_cell_histogram), without a GPU: the binning rule's host twin -- the text the kernel runs -- against the statement of
tests/_cell_histogram_form.py, the refusals that need no device, and the numpy layer on top (fields.py)."""
import ctypes

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import fields
import _cell_histogram_form as H


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("hmg_histogram_nbins", "hmg_histogram_edges", "hmg_histogram_bin", "hmg_cell_histogram"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["hmg_cell_histogram"] == (L.c_int, [L.vp, L.vp, L.p_f64, L.p_f64, L.c_int, L.c_int, L.c_int, L.p_i64])
    for f in (hmg.histogram_nbins, hmg.histogram_edges, hmg.histogram_bin, hmg.cell_histogram):
        assert callable(f)


@pytest.mark.parametrize("emin,emax,sub_bits", H.PARAMETER_SETS)
def test_rule_against_the_statement(emin, emax, sub_bits):
    E = H.edges(emin, emax, sub_bits)
    assert hmg.histogram_nbins(emin, emax, sub_bits) == H.nbins(emin, emax, sub_bits) == len(E) + 2
    got = hmg.histogram_edges(emin, emax, sub_bits)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, E)                              # exact doubles
    assert (np.diff(E) > 0).all() and E[0] == 2.0 ** emin and E[-1] == 2.0 ** emax
    q = H.value_set(E)
    want = H.bins(q, E)
    bins = hmg.histogram_bin(q, emin, emax, sub_bits)
    assert bins.dtype == np.int32 and bins.shape == q.shape
    bad = np.flatnonzero(bins != want)
    assert bad.size == 0, (q[bad[:5]], bins[bad[:5]], want[bad[:5]])
    # the value set reaches every kind of bin
    n = len(E) - 1
    assert {0, 1, n, n + 1, n + 2} <= set(np.unique(want).tolist())
    # ... and the shape of q is kept
    np.testing.assert_array_equal(hmg.histogram_bin(q[:12].reshape(3, 4), emin, emax, sub_bits), want[:12].reshape(3, 4))


def test_named_values():
    emin, emax, s = -6, 8, 3
    n = (emax - emin) << s
    q = np.array([0.0, -0.0, -1.0, -np.inf, 5e-324, 2.0 ** -7, 2.0 ** -6, np.nextafter(2.0 ** -6, 0.0), 1.0, 1.125, np.nextafter(1.125, 0.0),
                  np.nextafter(2.0 ** 8, 0.0), 2.0 ** 8, 1.7e308, np.inf, np.nan, -np.nan])
    want = [0, 0, 0, 0, 0, 0, 1, 0, 6 * 8 + 1, 6 * 8 + 2, 6 * 8 + 1, n, n + 1, n + 1, n + 1, n + 2, n + 2]
    assert hmg.histogram_bin(q, emin, emax, s).tolist() == want


@pytest.mark.parametrize("args,message", [
    ((0, 1, -1), "sub_bits = -1; 0 to 5 are served"),
    ((0, 1, 6), "sub_bits = 6; 0 to 5 are served"),
    ((-1023, 1, 0), "emin = -1023 is outside -1022 to 1023"),
    ((1024, 1025, 0), "emin = 1024 is outside -1022 to 1023"),
    ((0, 1024, 0), "emax = 1024 is outside -1022 to 1023"),
    ((0, -1023, 0), "emax = -1023 is outside -1022 to 1023"),
    ((3, 3, 0), "emin = 3 is not below emax = 3"),
    ((4, 3, 2), "emin = 4 is not below emax = 3"),
])
def test_parameters_outside_the_rule_are_refused(args, message):
    lib = L.load()
    assert lib.hmg_histogram_nbins(*args) == -1
    assert "hmg_histogram_nbins: " + message in lib.hmg_last_error().decode()
    with pytest.raises(L.HmgError, match="hmg_histogram_nbins: " + message):
        hmg.histogram_nbins(*args)
    e = np.zeros(5000)
    assert lib.hmg_histogram_edges(*args, e.ctypes.data_as(L.p_f64)) != 0
    assert "hmg_histogram_edges: " + message in lib.hmg_last_error().decode()
    q, b = np.ones(2), np.zeros(2, dtype=np.int32)
    assert lib.hmg_histogram_bin(2, q.ctypes.data_as(L.p_f64), *args, b.ctypes.data_as(L.p_i32)) != 0
    assert "hmg_histogram_bin: " + message in lib.hmg_last_error().decode()
    # the largest rule is served (the device call alone caps the regular bins at 1024: tests/test_gpu_cell_histogram.py)
    assert hmg.histogram_nbins(-1022, 1023, 5) == 2045 * 32 + 3


def test_null_arrays_are_refused():
    lib = L.load()
    assert lib.hmg_histogram_edges(0, 1, 0, None) != 0
    assert "hmg_histogram_edges: null edges" in lib.hmg_last_error().decode()
    b = np.zeros(2, dtype=np.int32)
    assert lib.hmg_histogram_bin(2, None, 0, 1, 0, b.ctypes.data_as(L.p_i32)) != 0
    assert "hmg_histogram_bin: null array" in lib.hmg_last_error().decode()
    assert lib.hmg_histogram_bin(-1, None, 0, 1, 0, None) != 0
    assert lib.hmg_histogram_bin(0, None, 0, 1, 0, None) == 0


def test_cell_histogram_on_a_host_only_grid_is_refused(oracle):
    base = oracle.hypercube(2, 1)
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), 3)
    lib = L.load()
    counts = np.zeros((g.ncells(), 11), dtype=np.int64)
    pc = counts.ctypes.data_as(L.p_i64)
    assert lib.hmg_cell_histogram(g.h, None, None, None, 0, 1, 3, pc) != 0
    msg = lib.hmg_last_error().decode()
    assert "hmg_cell_histogram" in msg and "created without a device context" in msg
    assert lib.hmg_cell_histogram(g.h, None, None, None, 0, 1, 3, None) != 0
    assert "hmg_cell_histogram: null counts" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_histogram(None, None, None, None, 0, 1, 3, pc) != 0 and lib.hmg_last_error().decode()
    g.close()


def test_fields_on_synthetic_counts():
    rng = np.random.default_rng(3)
    emin, emax, s = -3, 3, 2
    E = H.edges(emin, emax, s)
    ne, nel = 7, 64
    q = np.exp2(rng.uniform(-4.5, 4.5, (ne, nel)))
    q[2, :5] = 0.0
    q[4, 7] = -2.0
    counts = H.cell_counts(q, E)
    assert counts.shape == (ne, len(E) + 2) and (counts.sum(axis=1) == nel).all()
    vol = rng.random(ne) + 0.5
    # volumes: sum to the domain; labels split it
    v = fields.histogram_volume(counts, vol, nel)
    assert v.shape == (len(E) + 2,)
    np.testing.assert_allclose(v.sum(), vol.sum(), rtol=1e-14)
    np.testing.assert_allclose(v, (counts * (vol / nel)[:, None]).sum(axis=0), rtol=1e-14)
    labels = np.array([1, 2, 1, 1, 2, 3, 3])
    byl = fields.histogram_volume(counts, vol, nel, labels=labels)
    assert sorted(byl) == [1, 2, 3]
    for lab, row in byl.items():
        np.testing.assert_allclose(row.sum(), vol[labels == lab].sum(), rtol=1e-14)
    np.testing.assert_allclose(sum(byl.values()), v, rtol=1e-14)
    # tail: elements at or above each edge
    t = fields.histogram_tail(counts)
    assert t.shape == (ne, len(E)) and t.dtype == np.int64
    np.testing.assert_array_equal(t, (q[:, :, None] >= E[None, None, :]).sum(axis=1))
    np.testing.assert_array_equal(t, H.tail(counts))
    # quantile: the interval contains the volume-weighted quantile of the element values
    w = np.repeat(vol / nel, nel)
    order = np.argsort(q.ravel())
    qs, cw = q.ravel()[order], np.cumsum(w[order])
    for p in (0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0):
        lo, hi = fields.histogram_quantile(v, E, p)
        k = min(int(np.searchsorted(cw, p * cw[-1] * (1 - 1e-14), side="left")), qs.size - 1)
        assert lo <= qs[k] < hi, (p, lo, qs[k], hi)
        assert lo == -np.inf or lo in E
        assert hi == np.inf or hi in E
    assert fields.histogram_quantile(v[:-1], E, 0.5) == fields.histogram_quantile(v, E, 0.5)      # without the NaN bin
    # refusals
    bad = v.copy()
    bad[-1] = 1.0
    with pytest.raises(ValueError, match="NaN bin"):
        fields.histogram_quantile(bad, E, 0.5)
    with pytest.raises(ValueError):
        fields.histogram_quantile(v, E, 1.5)
    with pytest.raises(ValueError):
        fields.histogram_quantile(v[:5], E, 0.5)
    with pytest.raises(ValueError):
        fields.histogram_volume(counts, vol[:3], nel)
    with pytest.raises(ValueError):
        fields.histogram_volume(counts, vol, 0)
    with pytest.raises(ValueError):
        fields.histogram_volume(counts, vol, nel, labels=labels[:3])
