"""Host side of the per-cell extrema of cells larger than the LDS (csrc/hmg_extrema_window.hip), without a GPU, on host-only
grids of hypercube(3, 1) with 7 levels and hypercube(2, 1) with 11: the element mask of the levels only the window kernels serve
(3D level 7, 2D levels 9-11) -- built and checked against the element list at grid creation -- marks 2^(dim (level - 1)) elements,
and every slot of the cell interior has all of its 6 (2D: 2) simplices.  Then the closed form the row-band kernel finds a
lattice position's row with (rows_row_near), transcribed in float32: exact on every position of every 2D level, also with a square
root that is a few units in the last place off."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg

GRIDS = {3: 7, 2: 11}
_grids = {}


@pytest.fixture(scope="module")
def host(oracle):
    def get(dim):
        if dim not in _grids:
            base = oracle.hypercube(dim, 1)
            _grids[dim] = hmg.ImplicitFineGrid(None, hmg.Mesh(base.nodes, base.elements + 1), GRIDS[dim])
        return _grids[dim]
    yield get
    for g in _grids.values():
        g.close()
    _grids.clear()


@pytest.mark.parametrize("dim,level", [(3, 7), (2, 9), (2, 10), (2, 11)])
def test_element_mask_of_the_large_levels(host, dim, level):
    g = host(dim)
    mask = g.table_i32("elem_mask", level)
    lay = g.table_i32("layout", level)
    nf, off_int, nint = int(lay[0]), int(lay[10]), int(lay[7])
    m = 2 ** (level - 1)
    assert nf == ((m + 1) * (m + 2) * (m + 3) // 6 if dim == 3 else (m + 1) * (m + 2) // 2)
    assert mask.shape == (nf,) and off_int + nint == nf and nint > 0
    nperm = 6 if dim == 3 else 2
    assert (mask >= 0).all() and (mask < 2 ** nperm).all()
    popcount = sum(((mask >> k) & 1).astype(np.int64).sum() for k in range(nperm))
    assert popcount == 2 ** (dim * (level - 1)) == hmg.fine_elements(g, level)
    assert (mask[off_int:] == 2 ** nperm - 1).all()                  # the cell interior: every simplex at every slot
    assert (mask[:off_int] != 2 ** nperm - 1).any() and (mask == 0).any()   # ... the surface not (the face i + j + k = m: none)


def rows_ro(m, j):
    j = np.clip(j, 0, m + 1)
    return j * (m + 1) - ((j * (j - 1)) >> 1)


def rows_row_near(m, L, ulps=0):
    """csrc/hmg_extrema_window.hip, in numpy's float32; ulps: the square root moved by that many units in the last place"""
    f = np.float32
    b = f(2 * m + 3)
    root = np.sqrt(b * b - f(8.0) * L.astype(f))
    assert root.dtype == np.float32
    root = (root.view(np.int32) + np.int32(ulps)).view(f)
    j = ((b - root) * f(0.5)).astype(np.int64)
    j = np.clip(j, 0, m)
    for _ in range(2):
        j = j - ((j > 0) & (rows_ro(m, j) > L))
    for _ in range(2):
        j = j + ((j < m) & (rows_ro(m, j + 1) <= L))
    return j


@pytest.mark.parametrize("level", range(2, 12))
def test_row_of_a_lattice_position_in_closed_form(level):
    m = 2 ** (level - 1)
    want = np.repeat(np.arange(m + 1), m + 1 - np.arange(m + 1))     # row j holds m + 1 - j positions
    L = np.arange(want.size, dtype=np.int64)
    assert want.size == rows_ro(m, m + 1)
    for ulps in (0, -4, 4):
        np.testing.assert_array_equal(rows_row_near(m, L, ulps), want)
