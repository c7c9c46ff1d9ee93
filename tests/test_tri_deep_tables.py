"""
CPU tests of 2D grids with 9 to 11 levels (cells larger than the LDS): host tables against the oracle's statement of the
reference rules, the level cap, the checksums of the tables of every shallower grid (unchanged by the deep levels), and the
register budget of the row-band kernels of hmg_apply_rows.hip (cross-compiled for gfx950, no GPU needed).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import homogenization_jl_amd as hmg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def host_grid(m, levels):
    return hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements + 1), levels)


def upload_hash(m, levels):
    v = host_grid(m, levels).table_i32("upload_hash", 1).astype(np.uint32)
    return (int(v[1]) << 32) | int(v[0])


@pytest.fixture(scope="module")
def deep(oracle):
    O = oracle
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, 2, origin=(-1.0, -1.0)))
    return m, host_grid(m, 11), O.refined_element(11, 2)


@pytest.mark.parametrize("lev", [9, 10, 11])
def test_deep_numbering_and_transfer_tables(deep, lev):
    m, g, ref = deep
    mm = 2 ** (lev - 1)
    nf = (mm + 1) * (mm + 2) // 2
    assert g.nf(lev) == nf == ref.levels[lev - 1].nnodes()
    h2s = g.table_i32("hier2slot", lev)
    ijk = g.table_i32("slot_ijk", lev).reshape(-1, 3)
    nfx, ld, ncorner, nedge, nface, nei, nfi, nint, off_edge, off_face, off_int = g.table_i32("layout", lev)[:11]
    assert (ncorner, nedge, nface, nei, off_edge, off_int) == (3, 3, 0, mm - 1, 3, 3 + 3 * (mm - 1))
    np.testing.assert_array_equal(np.sort(h2s), np.arange(nf))
    np.testing.assert_array_equal(ijk[h2s][:, :2], np.round(ref.levels[lev - 1].nodes * mm).astype(int))
    # the storage order the row-band kernels derive from (i,j): corners, edges j = 0 / i = 0 / i + j = m in lattice order, then
    # the interior row by row
    i, j = ijk[:, 0], ijk[:, 1]
    q = np.arange(1, mm)
    np.testing.assert_array_equal(ijk[:3, :2], [[0, 0], [mm, 0], [0, mm]])
    np.testing.assert_array_equal(np.c_[i, j][3:3 + nei], np.c_[q, 0 * q])
    np.testing.assert_array_equal(np.c_[i, j][3 + nei:3 + 2 * nei], np.c_[0 * q, q])
    np.testing.assert_array_equal(np.c_[i, j][3 + 2 * nei:off_int], np.c_[mm - q, q])
    ii, jj = i[off_int:], j[off_int:]
    assert np.all((ii > 0) & (jj > 0) & (ii + jj < mm))
    assert np.all(np.diff(jj * (mm + 1) + ii) > 0)
    nb = ref.numbering[lev - 1]
    np.testing.assert_array_equal(h2s[nb.nodes], np.arange(3))
    for e, lst in enumerate(nb.edges_interior):
        np.testing.assert_array_equal(np.sort(h2s[lst]), off_edge + e * nei + np.arange(len(lst)))
    # transfer tables: prolongation rows and restriction lists against the reference's interpolation operator
    rng = np.random.default_rng(lev)
    P = ref.interops[lev - 2]
    h2s_c = g.table_i32("hier2slot", lev - 1)
    pa, pb = g.table_i32("par_a", lev), g.table_i32("par_b", lev)
    assert pa.max() < g.nf(lev - 1) and pb.max() < g.nf(lev - 1)
    xc = rng.random(P.shape[1])
    xc_s = np.zeros_like(xc); xc_s[h2s_c] = xc
    yf_s = np.where(pa == pb, xc_s[pa], 0.5 * xc_s[pa] + 0.5 * xc_s[pb])
    np.testing.assert_allclose(yf_s[h2s], P @ xc, rtol=0, atol=1e-15)
    s2h_c = np.argsort(h2s_c)
    assert np.all(s2h_c[pa] <= s2h_c[pb])
    rptr, ridx = g.table_i32("rptr", lev), g.table_i32("ridx", lev)
    xf = rng.random(P.shape[0])
    xf_s = np.zeros_like(xf); xf_s[h2s] = xf
    assert np.all(np.diff(rptr) >= 1)
    first = xf_s[ridx[rptr[:-1]]]
    bc_s = first + 0.5 * (np.add.reduceat(xf_s[ridx], rptr[:-1]) - first)
    np.testing.assert_allclose(bc_s[h2s_c], P.T @ xf, rtol=0, atol=1e-13)


def test_deep_mesh_masks(oracle, deep):
    O = oracle
    m, g, _ = deep
    impl = O.ImplicitFineGrid.create(m, 2)
    cn, ce, _ = O.list_boundary_nodes_edges_faces(m)
    want = np.zeros(m.nelements(), dtype=np.int64)
    np.bitwise_or.at(want, ce.element, 1 << ce.local_id)
    np.bitwise_or.at(want, cn.element, 1 << (3 + cn.local_id))
    np.testing.assert_array_equal(g.table_i32("dmask"), want)
    inter = impl.interfaces
    dup = np.zeros(m.nelements(), dtype=np.int64)
    for smap, shift in ((inter.edges, 0), (inter.nodes, 3)):
        first = np.zeros(len(smap.element), dtype=bool)
        first[smap.offset[:-1]] = True
        np.bitwise_or.at(dup, smap.element[~first], 1 << (shift + smap.local_id[~first]))
    np.testing.assert_array_equal(g.table_i32("dupmask"), dup)
    np.testing.assert_array_equal(g.interior_nodes(), O.list_interior_nodes(m))


def test_nine_and_ten_levels_are_created(oracle):
    m = oracle.hypercube(2, 1)
    for levels in (9, 10):
        g = host_grid(m, levels)
        assert g.nf(levels) == (2 ** (levels - 1) + 1) * (2 ** (levels - 1) + 2) // 2
        assert upload_hash(m, levels) == upload_hash(m, levels)            # deterministic tables


def test_level_cap_names_the_cap(oracle):
    m = oracle.hypercube(2, 1)
    with pytest.raises(Exception, match="1..11"):
        host_grid(m, 12)
    with pytest.raises(Exception, match="1..7"):
        host_grid(oracle.hypercube(3, 1), 8)


# checksums of every table a device grid uploads, recorded before the 2D levels 9..11 existed: the tables of 3D grids and of 2D
# grids of up to 8 levels did not move
PINNED = {
    (2, 3, 1): 0x4114e34eec4382dd, (2, 3, 2): 0x0b7250cf89e78141, (2, 3, 3): 0x1ffc9ac2ac9d38c7, (2, 3, 4): 0x856c209cfd91a01b,
    (2, 3, 5): 0x002dd37b825619a9, (2, 3, 6): 0xe592a86dc9fd7ea5, (2, 3, 7): 0xf49e3a350827b100, (2, 3, 8): 0x340db813cc116a5a,
    (3, 2, 1): 0xe376ea96aee08008, (3, 2, 2): 0x3436a4954c2ed264, (3, 2, 3): 0xb54dbcb43b696e42, (3, 2, 4): 0x081b7b3f2df8a4f7,
    (3, 2, 5): 0x95bfd7fce15f4050, (3, 2, 6): 0xd07288998d01e006, (3, 2, 7): 0x0ccc883eabc160f5,
}


@pytest.mark.parametrize("dim,n,levels", sorted(PINNED))
def test_shallow_tables_unchanged(oracle, dim, n, levels):
    assert upload_hash(oracle.hypercube(dim, n), levels) == PINNED[(dim, n, levels)]


# k_apply_rows<FUSED, WD>: 1024-thread workgroups, two per CU (2 x 78 KB of LDS) -> 8 waves per SIMD -> at most 64 VGPRs, no scratch
ROWS_BUDGET = {"Lb0ELb0E": 64, "Lb1ELb0E": 64, "Lb1ELb1E": 64}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_row_kernels_fit_their_register_budget(tmp_path):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply_rows.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "r.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for mt in re.finditer(r"Function Name: _ZN3hmg\w*?(k_apply_rowsI\w+?EE|k_prolong_add_wideE|k_norm2_unique_wideE)"
                          r"\w*?NS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, re.S):
        found[mt.group(1)] = (int(mt.group(2)), int(mt.group(3)))
    for name, vgprs in ROWS_BUDGET.items():
        key = "k_apply_rowsI" + name + "E"
        assert key in found, f"instantiation {name} not compiled; have {sorted(found)}"
        assert found[key][0] <= vgprs and found[key][1] == 0, (name, found[key])
    for key in ("k_prolong_add_wideE", "k_norm2_unique_wideE"):
        assert key in found and found[key][1] == 0, (key, found)
