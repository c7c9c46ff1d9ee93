"""Host side of the per-cell pair moments (include/hmg.h: hmg_cell_pair_moments, hmg_cell_pair_moments_count), without a GPU: the
entry points exist and are bound, the count, the refusals a host-only grid can reach, and the numpy layer on top
(fields.pair_energy, fields.tensor_sensitivity) on hand-made arrays."""
import ctypes

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import driver, fields


def host_grid(oracle, dim, n=1, levels=2):
    base = oracle.hypercube(dim, n)
    return hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), levels)


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("hmg_cell_pair_moments", "hmg_cell_pair_moments_count"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["hmg_cell_pair_moments"] == (L.c_int, [L.vp, L.vp, L.vp, L.p_f64, L.p_f64, L.p_f64])
    assert L.SIGNATURES["hmg_cell_pair_moments_count"] == (L.c_int, [L.vp])
    assert callable(hmg.cell_pair_moments) and callable(driver.dirichlet_homogenization_tensor)


def test_count_is_3_in_2d_and_6_in_3d(oracle):
    lib = L.load()
    assert lib.hmg_cell_pair_moments_count(host_grid(oracle, 2).h) == 3
    assert lib.hmg_cell_pair_moments_count(host_grid(oracle, 3).h) == 6
    assert lib.hmg_cell_pair_moments_count(None) == -1
    assert lib.hmg_last_error().decode() == "null grid"


def test_refusals_that_need_no_device(oracle):
    lib = L.load()
    g = host_grid(oracle, 2)
    out = np.zeros((g.ncells(), 3))
    po = out.ctypes.data_as(L.p_f64)
    # a grid without a device context: refused before the vectors are looked at
    assert lib.hmg_cell_pair_moments(g.h, None, None, None, None, po) != 0
    assert "without a device context" in lib.hmg_last_error().decode()
    # null out, null grid
    assert lib.hmg_cell_pair_moments(g.h, None, None, None, None, None) != 0
    assert "null output" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_pair_moments(None, None, None, None, None, po) != 0
    assert "null grid" in lib.hmg_last_error().decode()
    with pytest.raises(L.HmgError, match="hmg_cell_pair_moments"):
        L.check(lib.hmg_cell_pair_moments(g.h, None, None, None, None, None))
    np.testing.assert_array_equal(out, 0.0)                          # nothing was written


def test_pair_energy_on_hand_made_arrays():
    rng = np.random.default_rng(0)
    ne, d = 5, 3
    S = rng.standard_normal((ne, d, d))
    S = S + np.swapaxes(S, 1, 2)
    sd = rng.random((ne, d)) + 1.0
    st = rng.standard_normal((ne, d, d))
    st = st + np.swapaxes(st, 1, 2)
    want_d = np.array([sum(sd[c, k] * S[c, k, k] for k in range(d)) for c in range(ne)])
    want_t = np.array([sum(st[c, k, l] * S[c, k, l] for k in range(d) for l in range(d)) for c in range(ne)])
    np.testing.assert_allclose(fields.pair_energy(sd, S), want_d, rtol=1e-14)
    np.testing.assert_allclose(fields.pair_energy(st, S), want_t, rtol=1e-13)
    # a diagonal cond and the full tensor with that diagonal agree; for S = G it is fields.energy
    full = np.zeros((ne, d, d))
    full[:, range(d), range(d)] = sd
    np.testing.assert_allclose(fields.pair_energy(full, S), fields.pair_energy(sd, S), rtol=1e-14)
    np.testing.assert_array_equal(fields.pair_energy(sd, S), fields.energy(sd, S))
    # a uniform medium and v = w = 0: S = |c| sym(e_0 e_1^T), so a diagonal sigma sees nothing and a full one its 01 entry
    vol = np.array([0.5, 1.5])
    S01 = vol[:, None, None] * np.array([[0.0, 0.5], [0.5, 0.0]])[None]
    np.testing.assert_array_equal(fields.pair_energy(np.full((2, 2), 3.0), S01), 0.0)
    np.testing.assert_allclose(fields.pair_energy(np.tile(np.array([[2.0, 0.25], [0.25, 4.0]]), (2, 1, 1)), S01), 0.25 * vol)
    for bad_cond, bad_pair in ((np.ones((4, d)), S), (np.ones((ne, d + 1)), S), (sd, S[:, :, :2]), (sd, S[0])):
        with pytest.raises(ValueError):
            fields.pair_energy(bad_cond, bad_pair)


def test_tensor_sensitivity_on_hand_made_arrays():
    rng = np.random.default_rng(1)
    d, ne = 2, 4
    pairs = rng.standard_normal((d, d, ne, d, d))
    full = fields.tensor_sensitivity(pairs)
    assert full.shape == (d, d, ne, d, d)
    np.testing.assert_array_equal(full, pairs)
    diag = fields.tensor_sensitivity(pairs, diagonal=True)
    assert diag.shape == (d, d, ne, d)
    for m in range(d):
        np.testing.assert_array_equal(diag[..., m], pairs[..., m, m])
    # Sigma_kl |Omega| = sum_c sigma_c : pairs[k, l, c] is linear in sigma at fixed pairs: the array is its derivative
    sig = rng.random((ne, d, d))
    dsig = np.zeros_like(sig)
    dsig[2, 0, 1] = 1.0
    for k in range(d):
        for l in range(d):
            delta = fields.pair_energy(sig + dsig, pairs[k, l]).sum() - fields.pair_energy(sig, pairs[k, l]).sum()
            np.testing.assert_allclose(delta, full[k, l, 2, 0, 1], rtol=1e-12)
    for bad in (pairs[0], rng.standard_normal((d, d, ne, d, 3)), rng.standard_normal((d, 3, ne, d, d))):
        with pytest.raises(ValueError):
            fields.tensor_sensitivity(bad)
