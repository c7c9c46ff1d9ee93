"""Host side of the per-cell extrema (include/hmg.h: hmg_cell_extrema, hmg_grid_fine_elements), without a GPU, on host-only
grids: the fine-element table of every level -- the lattice basis `elem_dirs` and the per-slot mask `elem_mask` -- rebuilt into
elements and compared with the oracle's element list; the element count; the refusals that need no device; the numpy layer on
top (fields.py)."""
import ctypes
import itertools

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib as L
from homogenization_jl_amd import fields

LEVELS = {2: 5, 3: 4}
_grids = {}


@pytest.fixture(scope="module")
def host(oracle):
    def get(dim):
        if dim not in _grids:
            base = oracle.hypercube(dim, 1)
            _grids[dim] = (hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), LEVELS[dim]),
                           oracle.ImplicitFineGrid.create(base, LEVELS[dim]))
        return _grids[dim]
    yield get
    for g, _ in _grids.values():
        g.close()
    _grids.clear()


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("hmg_cell_extrema", "hmg_grid_fine_elements"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["hmg_cell_extrema"] == (L.c_int, [L.vp, L.vp, L.p_f64, L.p_f64, L.c_int, L.p_f64, L.p_f64])
    assert L.SIGNATURES["hmg_grid_fine_elements"] == (L.c_i64, [L.vp, L.c_int])
    assert callable(hmg.cell_extrema) and callable(hmg.fine_elements)


@pytest.mark.parametrize("dim,level", [(2, 2), (2, 3), (2, 4), (2, 5), (3, 2), (3, 3), (3, 4)])
def test_elements_rebuilt_from_the_tables_are_the_oracles(host, dim, level):
    g, implicit = host(dim)
    ijk = g.table_i32("slot_ijk", level).reshape(-1, 3)
    dirs = g.table_i32("elem_dirs", level).reshape(dim, dim)
    mask = g.table_i32("elem_mask", level)
    h2s = g.table_i32("hier2slot", level)
    nf = ijk.shape[0]
    assert mask.shape == (nf,) and h2s.shape == (nf,)
    want_dirs = [(0, 0, 1), (0, 1, -1), (1, -1, 0)] if dim == 3 else [(0, 1), (1, -1)]
    assert dirs.tolist() == [list(d) for d in want_dirs]
    basis = np.zeros((dim, 3), dtype=np.int64)
    basis[:, :dim] = dirs
    slot_at = {tuple(p): s for s, p in enumerate(ijk.tolist())}
    perms = list(itertools.permutations(range(dim)))                  # lexicographic
    assert mask.min() >= 0 and mask.max() < (1 << len(perms))
    rebuilt = []
    for s in range(nf):
        for k, perm in enumerate(perms):
            if not (mask[s] >> k) & 1:
                continue
            cur, el = ijk[s].astype(np.int64), [s]
            for b in perm:
                cur = cur + basis[b]
                el.append(slot_at[tuple(cur.tolist())])               # (a KeyError: the simplex leaves the cell)
            rebuilt.append(tuple(sorted(el)))
    ref = implicit.reference.levels[level - 1]
    listed = sorted(tuple(sorted(int(h2s[i]) for i in t)) for t in ref.elements)
    assert sorted(rebuilt) == listed
    popcount = sum(bin(int(x)).count("1") for x in mask)
    assert popcount == hmg.fine_elements(g, level) == 2 ** (dim * (level - 1)) == len(listed)
    if dim == 3 and level == 2:
        assert len({k for s in range(nf) for k in range(6) if (mask[s] >> k) & 1}) == 5      # 5 of the 6 shapes occur


def test_fine_elements_and_bad_levels(host):
    lib = L.load()
    for dim in (2, 3):
        g, _ = host(dim)
        for level in range(1, LEVELS[dim] + 1):
            assert lib.hmg_grid_fine_elements(g.h, level) == 2 ** (dim * (level - 1))
        for bad in (0, -1, LEVELS[dim] + 1):
            assert lib.hmg_grid_fine_elements(g.h, bad) == -1
            with pytest.raises(ValueError):
                hmg.fine_elements(g, bad)
    assert lib.hmg_grid_fine_elements(None, 1) == -1


def test_refusals_that_need_no_device(host):
    lib = L.load()
    g, _ = host(2)
    out = np.zeros((g.ncells(), 2))
    po = out.ctypes.data_as(L.p_f64)
    assert lib.hmg_cell_extrema(g.h, None, None, None, 0, None, po) != 0
    msg = lib.hmg_last_error().decode()
    assert "hmg_cell_extrema" in msg and "without a device context" in msg
    assert lib.hmg_cell_extrema(g.h, None, None, None, 0, None, None) != 0
    assert "hmg_cell_extrema: null output" in lib.hmg_last_error().decode()
    assert lib.hmg_cell_extrema(None, None, None, None, 0, None, po) != 0 and lib.hmg_last_error().decode()


def test_fields_on_hand_made_arrays():
    rng = np.random.default_rng(1)
    ne, d = 5, 3
    A = rng.standard_normal((ne, d, d))
    sig = np.einsum("eki,eli->ekl", A, A) + np.eye(d)[None]
    g = rng.standard_normal((ne, d))
    Qe, Qf = fields.energy_form(sig), fields.flux_form(sig)
    np.testing.assert_array_equal(Qe, np.swapaxes(Qe, 1, 2))
    np.testing.assert_array_equal(Qf, np.swapaxes(Qf, 1, 2))
    np.testing.assert_allclose(np.einsum("ek,ekl,el->e", g, Qe, g), np.einsum("ek,ekl,el->e", g, sig, g), rtol=1e-14)
    flux = np.einsum("ekl,el->ek", sig, g)
    np.testing.assert_allclose(np.einsum("ek,ekl,el->e", g, Qf, g), (flux ** 2).sum(axis=1), rtol=1e-13)
    diag = rng.random((ne, d)) + 0.5
    np.testing.assert_allclose(fields.energy_form(diag)[:, [0, 1, 2], [0, 1, 2]], diag)
    np.testing.assert_allclose(fields.flux_form(diag)[:, [0, 1, 2], [0, 1, 2]], diag ** 2)
    counts = np.array([[8, 0], [4, 1], [0, 0], [8, 8], [2, 1]])
    vol = np.array([1.0, 2.0, 3.0, 0.5, 4.0])
    ev = fields.exceedance_volume(counts, vol, 8)
    np.testing.assert_allclose(ev, [[1.0, 0.0], [1.0, 0.25], [0.0, 0.0], [0.5, 0.5], [1.0, 0.5]])
    np.testing.assert_allclose(fields.concentration(np.array([2.0, 6.0]), 2.0), [1.0, 3.0])
    np.testing.assert_allclose(fields.concentration(np.array([2.0, 6.0]), np.array([1.0, 3.0])), [2.0, 2.0])
    with pytest.raises(ValueError):
        fields.exceedance_volume(counts, vol[:3], 8)
    with pytest.raises(ValueError):
        fields.energy_form(np.ones((3, 2, 3)))
