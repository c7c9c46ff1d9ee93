"""CPU tests of the host side of tensor fields: driver.generate_polycrystal in 2D and 3D, driver.conductivity_per_element with a
grid of full tensors, and vtk.export_domain with tensors per cell."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver, vtk


@pytest.mark.parametrize("dim,n,principal", [(2, 7, (1.0, 9.0)), (3, 5, (1.0, 9.0, 100.0))])
def test_polycrystal_is_one_rotated_tensor_per_cube(dim, n, principal):
    S = driver.generate_polycrystal(dim, n, 3, principal)
    assert S.shape == (n,) * dim + (dim, dim) and S.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(S, np.swapaxes(S, -1, -2))              # exactly symmetric
    ev = np.linalg.eigvalsh(S.reshape(-1, dim, dim))
    # sigma = R diag(principal) R^T with R orthogonal: the eigenvalues are the principal conductivities (rounding of three
    # products and a symmetric eigensolve at condition 100)
    np.testing.assert_allclose(ev, np.broadcast_to(np.sort(principal), ev.shape), rtol=1e-12)
    flat = S.reshape(-1, dim * dim)
    assert np.unique(flat, axis=0).shape[0] == n ** dim                   # one orientation per cube
    np.testing.assert_array_equal(S, driver.generate_polycrystal(dim, n, 3, principal))      # seeded
    assert not np.array_equal(S, driver.generate_polycrystal(dim, n, 4, principal))
    with pytest.raises(ValueError):
        driver.generate_polycrystal(dim, n, 3, (1.0,) * (dim + 1))


def test_polycrystal_default_principal():
    for dim, want in ((2, (1.0, 9.0)), (3, (1.0, 9.0, 100.0))):
        ev = np.linalg.eigvalsh(driver.generate_polycrystal(dim, 2, 0).reshape(-1, dim, dim))
        np.testing.assert_allclose(ev, np.broadcast_to(want, ev.shape), rtol=1e-12)


def test_polycrystal_2d_angle_is_the_rotation_of_the_first_axis():
    """2D: sigma = R(t) diag(p) R(t)^T, t in [0, pi): sigma_11 = p1 c^2 + p2 s^2, sigma_12 = (p1 - p2) c s; the angle recovered
    from the entries rotates diag(p) back into sigma."""
    p = (1.0, 9.0)
    S = driver.generate_polycrystal(2, 9, 11, p).reshape(-1, 2, 2)
    t = 0.5 * np.arctan2(2.0 * S[:, 0, 1] / (p[0] - p[1]), (S[:, 0, 0] - S[:, 1, 1]) / (p[0] - p[1])) % np.pi
    c, s = np.cos(t), np.sin(t)
    np.testing.assert_allclose(S[:, 0, 0], p[0] * c * c + p[1] * s * s, rtol=1e-12)
    np.testing.assert_allclose(S[:, 0, 1], (p[0] - p[1]) * c * s, atol=1e-12)
    # uniform on [0, pi): 81 angles, all four quarters of the range are hit (a quarter stays empty with probability 4 (3/4)^81 < 1e-9)
    assert set(np.floor(t / (np.pi / 4)).astype(int)) == {0, 1, 2, 3}


def test_polycrystal_3d_rotations_are_uniform_in_the_mean():
    """A uniform rotation makes the mean tensor isotropic, trace / 3 times the identity.  With u, v two rows of R (uniform on the
    sphere, orthogonal): Var(sigma_11) = 4/45 (sum p^2 - sum_{j<k} p_j p_k) = 806.5 and Var(sigma_12) = 1/15 (the same bracket) =
    604.9 for p = (1, 9, 100); over 12^3 = 1728 cubes the means have standard deviations 0.68 and 0.59.  Bound: five of the larger."""
    p = np.array([1.0, 9.0, 100.0])
    S = driver.generate_polycrystal(3, 12, 1, p).reshape(-1, 3, 3)
    assert np.abs(S.mean(axis=0) - p.sum() / 3.0 * np.eye(3)).max() <= 5 * 0.684


@pytest.mark.parametrize("dim", [2, 3])
def test_conductivity_per_element_passes_tensor_grids_through(dim):
    n = 4
    tag = hmg.Tri64 if dim == 2 else hmg.Tet64
    mesh = driver.checkerboard_mesh(tag, n, origin=(-n / 2.0,) * dim, transposed_lookup=True)
    off = (n / 2.0 + 1.0,) * dim
    D = driver.generate_conductivity(dim, n, 2)
    T = np.zeros((n,) * dim + (dim, dim))
    T[..., np.arange(dim), np.arange(dim)] = D
    got = driver.conductivity_per_element(mesh, T, off)
    want = driver.conductivity_per_element(mesh, D, off)                   # the library's host code, diagonal grids
    assert got.shape == (mesh.elements.shape[0], dim, dim) and got.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got[:, np.arange(dim), np.arange(dim)], want)
    P = driver.generate_polycrystal(dim, n, 5)
    got = driver.conductivity_per_element(mesh, P, off)
    per_cube = (2 if dim == 2 else 6)
    rows, counts = np.unique(got.reshape(-1, dim * dim), axis=0, return_counts=True)
    assert rows.shape[0] == n ** dim and (counts == per_cube).all()        # every cube's tensor, on all of its simplices


@pytest.mark.parametrize("dim", [2, 3])
def test_export_domain_writes_the_tensor_components(dim, tmp_path):
    n = 2
    tag = hmg.Tri64 if dim == 2 else hmg.Tet64
    mesh = driver.checkerboard_mesh(tag, n, origin=(-1.0,) * dim, transposed_lookup=True)
    cond = driver.conductivity_per_element(mesh, driver.generate_polycrystal(dim, n, 8), (2.0,) * dim)
    out = vtk.read_vtu(vtk.export_domain(mesh, cond, str(tmp_path / "poly")))
    a = out["cell_data"]["a"]
    order = [(0, 0), (0, 1), (1, 1)] if dim == 2 else [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert a.shape == (mesh.elements.shape[0], len(order))
    for q, (i, j) in enumerate(order):
        np.testing.assert_array_equal(a[:, q], cond[:, i, j])
    # a diagonal field keeps the reference's layout
    diag = driver.conductivity_per_element(mesh, driver.generate_conductivity(dim, n, 8), (2.0,) * dim)
    out = vtk.read_vtu(vtk.export_domain(mesh, diag, str(tmp_path / "diag")))
    np.testing.assert_array_equal(out["cell_data"]["a"], diag)
