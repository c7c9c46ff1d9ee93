"""Host side of the per-cell gradient moments (include/hmg.h: hmg_cell_moments, hmg_cell_moments_count), without a GPU: the entry
points exist and are bound, the count, the refusals that need no device, and the numpy layer on top (fields.py,
vtk.export_cell_fields) on hand-made arrays."""
import ctypes
import os

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import fields, vtk


def host_grid(oracle, dim, n=1, levels=2):
    base = oracle.hypercube(dim, n)
    return hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), levels)


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("hmg_cell_moments", "hmg_cell_moments_count"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["hmg_cell_moments"] == (L.c_int, [L.vp, L.vp, L.p_f64, L.p_f64])
    assert callable(hmg.cell_moments)


def test_count_is_5_in_2d_and_9_in_3d(oracle):
    lib = L.load()
    assert lib.hmg_cell_moments_count(host_grid(oracle, 2).h) == 5
    assert lib.hmg_cell_moments_count(host_grid(oracle, 3).h) == 9


def test_refusals_that_need_no_device(oracle):
    lib = L.load()
    g = host_grid(oracle, 2)
    out = np.zeros((g.ncells(), 5))
    # a grid without a device context: refused before the vector is looked at
    rc = lib.hmg_cell_moments(g.h, None, None, out.ctypes.data_as(L.p_f64))
    assert rc != 0
    msg = lib.hmg_last_error().decode()
    assert msg and "without a device context" in msg
    # null out, null grid
    assert lib.hmg_cell_moments(g.h, None, None, None) != 0
    assert "null output" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_moments(None, None, None, out.ctypes.data_as(L.p_f64)) != 0 and lib.hmg_last_error().decode()
    assert lib.hmg_cell_moments_count(None) == -1
    with pytest.raises(L.HmgError):
        L.check(lib.hmg_cell_moments(g.h, None, None, None))


def two_phase_square():
    """the unit square [0, 2] x [0, 1] in four triangles: two of phase 0 (left), two of phase 1 (right)"""
    nodes = np.array([(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)], dtype=np.float64)
    cells = np.array([(1, 2, 4), (2, 4, 5), (2, 3, 5), (3, 5, 6)], dtype=np.int64)
    return hmg.Mesh(nodes, cells), np.array([0, 0, 1, 1])


def test_fields_on_hand_made_arrays():
    base, labels = two_phase_square()
    ne, d = 4, 2
    vol = fields.cell_volumes(base)
    np.testing.assert_allclose(vol, 0.5)
    xi = np.array([0.6, 0.8])
    # a uniform medium, v = 0: m_u = xi in every cell, G_u = |c| xi xi^T
    mean = np.tile(xi, (ne, 1))
    gram = vol[:, None, None] * np.outer(xi, xi)[None]
    sig_d = np.full((ne, d), 3.0)
    S = np.array([[2.0, 0.5], [0.5, 4.0]])
    sig_t = np.tile(S, (ne, 1, 1))
    np.testing.assert_allclose(fields.flux_row(base, sig_d, mean), 3.0 * xi, rtol=1e-15)
    np.testing.assert_allclose(fields.flux_row(base, sig_t, mean), S @ xi, rtol=1e-15)
    np.testing.assert_allclose(fields.flux_row(base, sig_t, mean, ncells=2), S @ xi, rtol=1e-15)
    np.testing.assert_allclose(fields.mean_flux(sig_d, mean), 3.0 * mean)
    np.testing.assert_allclose(fields.energy(sig_d, gram).sum() / vol.sum(), 3.0 * xi @ xi, rtol=1e-15)
    np.testing.assert_allclose(fields.energy(sig_t, gram).sum() / vol.sum(), xi @ S @ xi, rtol=1e-15)
    # two phases with different fields and unequal cell weights
    volw = np.array([0.5, 1.5, 1.0, 3.0])
    mean = np.array([(1.0, 0.0), (3.0, 4.0), (0.0, 2.0), (4.0, -2.0)])
    gram = np.arange(16, dtype=np.float64).reshape(4, 2, 2)
    pm = fields.phase_moments(labels, volw, mean, gram)
    assert set(pm) == {0, 1}
    np.testing.assert_allclose(pm[0]["volume"], 2.0)
    np.testing.assert_allclose(pm[0]["mean"], (0.5 * mean[0] + 1.5 * mean[1]) / 2.0)
    np.testing.assert_allclose(pm[1]["mean"], (1.0 * mean[2] + 3.0 * mean[3]) / 4.0)
    np.testing.assert_allclose(pm[1]["second"], (gram[2] + gram[3]) / 4.0)
    # sensitivities
    assert fields.sensitivity(gram) is not None and fields.sensitivity(gram).shape == (4, 2, 2)
    np.testing.assert_array_equal(fields.sensitivity(gram, diagonal=True), gram[:, [0, 1], [0, 1]])
    with pytest.raises(ValueError):
        fields.mean_flux(np.ones((3, 2)), mean)


def test_export_cell_fields_round_trips(tmp_path):
    base, labels = two_phase_square()
    rng = np.random.default_rng(0)
    mean = rng.standard_normal((4, 2))
    gram = rng.standard_normal((4, 2, 2))
    gram = gram + np.swapaxes(gram, 1, 2)
    en = rng.random(4)
    path = vtk.export_cell_fields(base, {"mean": mean, "gram": gram, "energy": en}, os.path.join(str(tmp_path), "cells"))
    assert path.endswith(".vtu")
    back = vtk.read_vtu(path)
    np.testing.assert_array_equal(back["connectivity"].reshape(-1, 3), base.elements - 1)
    np.testing.assert_array_equal(back["points"][:, :2], base.nodes)
    np.testing.assert_array_equal(back["cell_data"]["mean"], mean)
    np.testing.assert_array_equal(back["cell_data"]["energy"], en)
    np.testing.assert_array_equal(back["cell_data"]["gram"], gram[:, [0, 0, 1], [0, 1, 1]])
    # a prefix of the cells (a shrunk domain)
    back = vtk.read_vtu(vtk.export_cell_fields(base, {"energy": en[:2]}, os.path.join(str(tmp_path), "prefix")))
    assert back["connectivity"].size == 6
    with pytest.raises(ValueError):
        vtk.export_cell_fields(base, {"a": en, "b": en[:3]}, os.path.join(str(tmp_path), "bad"))
