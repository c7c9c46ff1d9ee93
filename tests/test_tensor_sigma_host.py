"""CPU tests of hmg_grid_set_operator_tensor on host-only grids (no device): coefficient rows, level-1 matrix, refusals, the class
table.  The yardsticks are numpy restatements (tests/_tensor_sigma_form.py) and, for a uniformly rotated tensor, the diagonal
entry point itself on the rotated mesh."""
import numpy as np
import pytest
import scipy.sparse as sp

import homogenization_jl_amd as hmg
import _tensor_sigma_form as T


def host_grid(m, levels):
    return hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements + 1), levels)


def upload_hash(g):
    v = g.table_i32("upload_hash", 1).astype(np.uint32)
    return (int(v[1]) << 32) | int(v[0])


def mesh_of(O, dim):
    """3D: hypercube(3, 2) with perturbed interior nodes; 2D: n = 4"""
    if dim == 2:
        return O.hypercube(2, 4)
    m = O.hypercube(3, 2)
    inner = O.list_interior_nodes(m)
    m.nodes[inner] += 0.2 * (np.random.default_rng(5).random((len(inner), 3)) - 0.5)
    return m


def coarse_csr(g, n):
    return sp.csr_matrix((g.table_f64("coarse_val"), g.table_i32("coarse_colidx"), g.table_i32("coarse_rowptr")), shape=(n, n))


@pytest.mark.parametrize("dim", [3, 2])
def test_coefficient_table(oracle, dim):
    """(a) coef = |J| J^-1 sigma J^-T for random SPD tensors per cell.  An entry is |J| times a sum of nine products (four in 2D)
    of three factors: 1e-13 relative to the sum of the products' magnitudes (about 450 roundings' worth)."""
    O = oracle
    m = mesh_of(O, dim)
    sig = T.random_spd(np.random.default_rng(1), m.nelements(), dim)
    g = host_grid(m, 2)
    g.set_operator(sig, 0.5)
    got = g.table_f64("coef").reshape(-1, 8)
    want = T.coefficient_rows(O, m, sig)
    _, Jinv, det = O.cell_geometry(m)
    mag = np.zeros_like(want)
    pk = T.pack(np.einsum("eki,ekl,elj->eij", abs(Jinv), abs(sig), abs(Jinv))) * det[:, None]
    mag[:, :pk.shape[1]] = pk
    mag[:, pk.shape[1]] = det
    err = abs(got - want)
    print("coef: max error / magnitude =", (err[mag > 0] / mag[mag > 0]).max())
    assert (err <= 1e-13 * mag).all()
    assert np.count_nonzero(got[:, 1]) == m.nelements()                  # (the off-diagonal entries are there)


@pytest.mark.parametrize("dim", [3, 2])
def test_diagonal_field_takes_the_diagonal_entrys_bits(oracle, dim):
    """(b) zero off-diagonals: the coefficient table, the upload hash (class table included) and the level-1 tables of the
    diagonal entry point, bit for bit"""
    O = oracle
    m = mesh_of(O, dim)
    d = np.random.default_rng(2).choice([1.0, 9.0, 100.0], size=(m.nelements(), dim))
    sig = np.zeros((m.nelements(), dim, dim))
    for a in range(dim):
        sig[:, a, a] = d[:, a]
    tabs = []
    for field in (d, sig):
        g = host_grid(m, 3)
        g.set_operator(field, 0.35)
        g.coarse_setup()
        tabs.append((g.table_f64("coef"), g.table_i32("cell_class"), g.table_f64("coarse_val"), g.table_i32("coarse_colidx"),
                     g.table_i32("coarse_rowptr"), upload_hash(g)))
    for u, v in zip(*tabs):
        np.testing.assert_array_equal(u, v)
    assert tabs[0][0].view(np.uint64).tolist() == tabs[1][0].view(np.uint64).tolist()
    assert tabs[0][2].view(np.uint64).tolist() == tabs[1][2].view(np.uint64).tolist()


@pytest.mark.parametrize("dim", [2, 3])
def test_coarse_matrix(oracle, dim):
    """(c) the level-1 matrix against the textbook P1 matrix, at the tolerance of test_host_tables.py::test_coarse_matrix"""
    O = oracle
    m = O.hypercube(dim, 3)
    m.nodes = m.nodes + 0.2 * (np.random.default_rng(1).random(m.nodes.shape) - 0.5)
    sig = T.random_spd(np.random.default_rng(3), m.nelements(), dim, 1.0, 9.0)
    g = host_grid(m, 2)
    g.set_operator(sig, 0.35)
    g.coarse_setup()
    interior = O.list_interior_nodes(m)
    want = T.assemble_p1(O, m, sig, 0.35)[interior][:, interior]
    got = coarse_csr(g, want.shape[0])
    assert abs(got - want).max() <= 1e-13 * abs(want).max()
    # ... and it is not the matrix of the diagonal parts
    diag_only = sig * np.eye(dim)[None]
    assert abs(T.assemble_p1(O, m, diag_only, 0.35)[interior][:, interior] - want).max() > 1e-3 * abs(want).max()


@pytest.mark.parametrize("dim", [3, 2])
def test_refusals_name_the_cell_and_keep_the_operator(oracle, dim):
    """(d) indefinite, NaN and asymmetric tensors"""
    O = oracle
    m = mesh_of(O, dim)
    n = m.nelements()
    good = T.random_spd(np.random.default_rng(4), n, dim)
    g = host_grid(m, 2)
    g.set_operator(good, 0.5)
    coef = g.table_f64("coef").copy()
    cell = n - 3

    bad = good.copy()
    bad[cell] = np.eye(dim)
    bad[cell, 0, 1] = bad[cell, 1, 0] = 2.0                            # second leading minor 1 - 4 < 0
    with pytest.raises(hmg._lib.HmgError, match=rf"cell {cell}\b.*positive definite"):
        g.set_operator(bad, 0.5)
    bad = good.copy()
    bad[cell, dim - 1, dim - 1] = -abs(bad[cell, dim - 1, dim - 1])    # the last minor
    with pytest.raises(hmg._lib.HmgError, match=rf"cell {cell}\b.*positive definite"):
        g.set_operator(bad, 0.5)
    bad = good.copy()
    bad[cell, 0, 0] = np.nan
    with pytest.raises(hmg._lib.HmgError, match=rf"cell {cell}\b.*finite"):
        g.set_operator(bad, 0.5)
    bad = good.copy()
    bad[cell, dim - 1, dim - 1] = np.inf
    with pytest.raises(hmg._lib.HmgError, match=rf"cell {cell}\b.*finite"):
        g.set_operator(bad, 0.5)
    bad = good.copy()
    bad[cell, 0, 1] += 1e-9
    with pytest.raises(ValueError, match=rf"cell {cell}\b.*symmetric"):
        g.set_operator(bad, 0.5)
    with pytest.raises(ValueError, match=rf"cell {cell}\b.*symmetric"):
        hmg.L2PlusDivAGrad(g, 0.5, bad)
    with pytest.raises(ValueError, match="shape"):
        g.set_operator(good[:, :, :1], 0.5)

    np.testing.assert_array_equal(g.table_f64("coef"), coef)            # the previous operator is still in force
    g.coarse_setup()
    interior = O.list_interior_nodes(m)
    want = T.assemble_p1(O, m, good, 0.5)[interior][:, interior]
    assert abs(coarse_csr(g, want.shape[0]) - want).max() <= 1e-13 * abs(want).max()


@pytest.mark.parametrize("dim", [3, 2])
def test_uniform_rotation_is_the_diagonal_entry_on_the_rotated_mesh(oracle, dim):
    """(e) sigma = Q D Q^T on the plain mesh and diag D on the mesh x -> Q^T x: coefficient rows and level-1 matrix to 1e-12 of
    the largest entry (measured: 3e-15 with D = (1, 9, 100))"""
    O = oracle
    m = mesh_of(O, dim)
    Q = T.random_rotation(np.random.default_rng(6), dim)
    D = np.array([1.0, 9.0, 100.0])[:dim]
    S = (Q * D[None, :]) @ Q.T
    sig = np.broadcast_to(0.5 * (S + S.T), (m.nelements(), dim, dim))
    a = host_grid(m, 2)
    a.set_operator(sig, 0.7)
    a.coarse_setup()
    mr = T.rotated_mesh(O, m, Q)
    b = host_grid(mr, 2)
    b.set_operator(np.broadcast_to(D, (m.nelements(), dim)), 0.7)
    b.coarse_setup()
    ca, cb = a.table_f64("coef"), b.table_f64("coef")
    print("rotation: coef", abs(ca - cb).max() / abs(cb).max())
    assert abs(ca - cb).max() <= 1e-12 * abs(cb).max()
    n = len(O.list_interior_nodes(m))
    A, B = coarse_csr(a, n), coarse_csr(b, n)
    print("rotation: level-1 matrix", abs(A - B).max() / abs(B).max())
    assert abs(A - B).max() <= 1e-12 * abs(B).max()


def test_class_table_takes_a_row_per_cell(oracle):
    """(f) 6^3 cubes, 1 296 cells, one distinct tensor per cell: 1 296 classes (the library used to give up at 1 025 rows and
    export none); a {1, 9} field on the same mesh: 8 triples x 6 orientations, a few more by the sign of a
    zero"""
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(3, 6, origin=(-3.0, -3.0, -3.0)))
    n = m.nelements()
    assert n == 1296
    g = host_grid(m, 3)
    assert g.table_i32("cell_class").size == 0                           # no operator, no table
    sig = T.random_spd(np.random.default_rng(7), n, 3)
    g.set_operator(sig, 1.0)
    cls = g.table_i32("cell_class")
    assert cls.shape == (n,)
    assert np.unique(cls).size == n and cls.min() == 0 and cls.max() == n - 1
    rows = g.table_f64("coef").reshape(-1, 8)
    assert np.unique(rows, axis=0).shape[0] == n
    g.set_operator(np.random.default_rng(8).choice([1.0, 9.0], size=(n, 3)), 1.0)
    cls = g.table_i32("cell_class")
    rows = g.table_f64("coef").reshape(-1, 8)
    nbits = np.unique(np.ascontiguousarray(rows).view(np.uint64), axis=0).shape[0]    # (classes go by the BITS of the row)
    assert cls.shape == (n,) and np.unique(cls).size == nbits < 200
    first = {}
    for c, k in enumerate(cls):                                          # classes: the bits of the row, numbered by first use
        first.setdefault(int(k), rows[c])
        np.testing.assert_array_equal(rows[c], first[int(k)])
    assert hmg.ImplicitFineGrid(None, hmg.Mesh(O.hypercube(2, 4).nodes, O.hypercube(2, 4).elements + 1), 3).table_i32("cell_class").size == 0
