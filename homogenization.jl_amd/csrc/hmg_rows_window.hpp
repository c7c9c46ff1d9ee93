// Row bands of a 2D cell larger than the LDS: the window geometry that k_apply_rows (hmg_apply_rows.hip) and
// k_cell_pair_moments_rows (hmg_fields_window.hip) share.  The lattice image is L(i,j) = RO(j) + i, row j holds m+1-j nodes; a
// band evaluates rows [j0, j1) from a window that holds rows [j0-1, j1] and a zero guard.  Closed forms: no per-level tables.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

constexpr int RW_NT = 1024;          // threads per workgroup: two resident per CU (<= 64 VGPRs, 2 x 78 KB of LDS)
constexpr int RW_WIN = 9600;         // window doubles: rows [j0-1, j1] + guard
constexpr int RW_GUARD = 8;          // zero entries behind the window (the last evaluated row reads one past it)
constexpr int RW_MV = 3;             // values per thread of the window move (two rows of <= 1025 nodes)

__host__ __device__ __forceinline__ int rows_ro(int m, int j)   // RO(j) = lattice nodes in rows < j (j clamped to [0, m+1])
{
    j = j < 0 ? 0 : j > m + 1 ? m + 1 : j;
    return j * (m + 1) - ((j * (j - 1)) >> 1);
}

// last row (exclusive) of the band that starts at row j0: the window [j0-1, j1] plus the guard fits RW_WIN
__host__ __device__ __forceinline__ int rows_band_end(int m, int j0)
{
    const int lo = rows_ro(m, j0 - 1);
    int j1 = j0 + 1;
    while (j1 <= m && rows_ro(m, j1 + 2) - lo + RW_GUARD <= RW_WIN) ++j1;
    return j1;
}

// row of lattice position L (0 <= L < nf): RO(j) <= L < RO(j+1)
__device__ __forceinline__ int rows_row_of(int m, int L)
{
    const float b = (float)(2 * m + 3);
    int j = (int)((b - __builtin_sqrtf(b * b - 8.0f * (float)L)) * 0.5f);
    j = j < 0 ? 0 : j > m ? m : j;
    while (j > 0 && rows_ro(m, j) > L) --j;
    while (j < m && rows_ro(m, j + 1) <= L) ++j;
    return j;
}

}  // namespace hmg
