"""Premises of tests/test_gpu_coarse_solve.py, on host-only grids: every mesh used there reaches the path of the level-1
solve's kernels (csrc/hmg_kernels.hip: coarse_rows_product, k_coarse_direction, k_coarse_cheb, k_coarse_init, k_coarse_update)
that its case is named for.  The statement of the solve itself (tests/_coarse_form.py) is held against the oracle's V-cycle at
level 1 on the small meshes."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
import _coarse_form as C

# coarse_rows_product: a row's entries go to 16 lanes; `for (k = rp[j] + sub + 16; ...; k += 16)` runs once more per 16 entries
LANES = 16
# coarse_spmv_blocks: `if (b > 1024) b = 1024` blocks of 256 threads = 16 groups of 16 lanes, CR = 4 rows per group: one trip of
# `for (i0 = CR * (... >> 4); i0 < A.n; i0 += CR * (gridDim.x * blockDim.x >> 4))` covers
SPMV_CAP = 4 * 16 * 1024
# coarse_blocks: `if (b > 1024) b = 1024` blocks of 256 threads, one row per thread: one trip of
# `for (i = ...; i < A.n; i += gridDim.x * blockDim.x)` in k_coarse_init / k_coarse_update covers
VECTOR_CAP = 256 * 1024


def system(O, name, lam=0.7, seed=1):
    m = C.mesh(O, name)
    g = hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements + 1), 2)
    g.set_operator(C.two_valued(m, seed), lam)
    g.coarse_setup()
    A, interior = C.matrix(g)
    return m, g, A, interior


@pytest.mark.parametrize("name", [k for k in C.MESHES if k != "sq514"])
def test_matrix_of_every_small_mesh(oracle, name):
    O = oracle
    m, g, A, interior = system(O, name)
    n = interior.size
    assert n == C.UNKNOWNS[name]
    np.testing.assert_array_equal(interior, O.list_interior_nodes(m))
    if n == 0:
        return
    assert abs(A - A.T).max() <= 1e-14 * abs(A).max()
    assert A.diagonal().min() > 0.0
    rows = C.row_lengths(A)
    if name in C.LATTICES:
        assert rows.max() <= 15                                 # one trip of the lanes, never the extra-trip loop
    # the statement against the oracle's level-1 V-cycle (its own assembly and splu)
    sig = C.two_valued(m, 1)
    impl = O.ImplicitFineGrid.create(m, 2)
    st = [O.LevelState.create(m.nelements(), m.dim + 1)]
    b1 = np.random.default_rng(2).random(st[0].b.shape) - 0.5
    st[0].b[...] = b1
    O.vcycle(impl, O.make_base_level(m, sig, 0.7), None, st, 1)
    D = C.Direct(A, interior, m.elements, m.nnodes())
    assert C.relerr(D.solve(b1), st[0].x) <= 1e-12
    np.testing.assert_allclose(st[0].b, C.broadcast(m.elements, m.nnodes(), b1), rtol=1e-14, atol=1e-15)
    x = D.solve_interior(b1)
    assert D.residual(b1, x) <= 1e-13
    assert D.residual(b1, 1.001 * x) > 1e-4


def test_residues_of_the_row_groups():
    """four rows per group of 16 lanes: n = 0, n = 1, n < 4 and every residue of n mod 4 among the shapes of case 1"""
    shapes = ["sq1", "sq2", "sq3", "sq4", "cu2", "cu3", "cu4", "del2_18", "del2_19", "del2_20", "del2_21"]
    n = [C.UNKNOWNS[k] for k in shapes]
    assert 0 in n and 1 in n
    assert {v % 4 for v in n if v > 0} == {0, 1, 2, 3}
    assert {C.UNKNOWNS[k] % 4 for k in ("del2_18", "del2_19", "del2_20", "del2_21")} == {0, 1, 2, 3}
    assert C.UNKNOWNS["cu3"] % 4 == 0 and C.UNKNOWNS["cu4"] % 4 == 3


def test_long_rows(oracle):
    """one extra trip of the lanes on the Delaunay meshes, two on the fans (whose long row is the centre's)"""
    for name, least, most in (("del3_60", LANES, 2 * LANES), ("del3_120", LANES, 2 * LANES), ("fan2", 2 * LANES, 4 * LANES),
                              ("fan3", 2 * LANES, 3 * LANES)):
        m, g, A, interior = system(oracle, name)
        rows = C.row_lengths(A)
        assert least < rows.max() <= most, (name, rows.max())
        if name.startswith("fan"):
            ninner = C.MESHES[name][2]
            assert ninner >= 40
            np.testing.assert_array_equal(interior, np.arange(ninner + 1))         # the centre, the inner shell; the outer is constrained
            assert rows[0] == ninner + 1 and rows[1:].max() <= LANES
            e = m.nodes[m.elements[:, 1:]] - m.nodes[m.elements[:, :1]]
            vol = np.abs(np.linalg.det(e))
            assert vol.min() > 5e-3 * vol.max()                                     # no sliver: the cases are about indexing


def test_large_lattice_is_above_both_caps(oracle):
    m, g, A, interior = system(oracle, "sq514", lam=1.0e4)
    n = interior.size
    assert n == 513 * 513 == C.UNKNOWNS["sq514"] and n % 4 == 1
    assert SPMV_CAP == 65536 and VECTOR_CAP == 262144
    assert n > VECTOR_CAP > SPMV_CAP
    assert n < 2 * VECTOR_CAP                                   # (the vector kernels' second trip is a partial one)
    assert C.row_lengths(A).max() <= 15
    assert abs(A - A.T).max() <= 1e-14 * abs(A).max() and A.diagonal().min() > 0.0
    # the mass term dominates: strictly diagonally dominant rows, a short iteration
    off = np.asarray(abs(A).sum(axis=1)).ravel() - A.diagonal()
    assert (off < A.diagonal()).all()
