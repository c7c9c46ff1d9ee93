// Row bands of a 2D cell larger than the LDS: the window geometry that k_apply_rows (hmg_apply_rows.hip) and the rows walk of the
// per-cell results (hmg_cell_window.hpp) share.  The lattice image is L(i,j) = RO(j) + i, row j holds m+1-j nodes; a
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

// Row of lattice position L (0 <= L < nf), as rows_row_of, without its loops.  RO(j) <= L is j^2 - b j + 2 L >= 0, b = 2 m + 3, so
// the row is the floor of the smaller root (b - sqrt(b^2 - 8 L)) / 2.  b^2 <= 4 206 601 and 8 L are integers below 2^24 and their
// difference is at least 9: exact in float; the root, the difference from b and the halving each round once, an absolute error
// below 1e-3: the truncated estimate is at most one row off, and two steps either way correct it with one to spare.  (The loops
// of rows_row_of, inlined four times into the load phase next to k_cell_extrema_rows' counters, cost it 40 scalar registers and spills.)
__device__ __forceinline__ int rows_row_near(int m, int L)
{
    const float b = (float)(2 * m + 3);
    int j = (int)((b - __builtin_sqrtf(b * b - 8.0f * (float)L)) * 0.5f);
    j = j < 0 ? 0 : j > m ? m : j;
    j -= (j > 0 && rows_ro(m, j) > L) ? 1 : 0;
    j -= (j > 0 && rows_ro(m, j) > L) ? 1 : 0;
    j += (j < m && rows_ro(m, j + 1) <= L) ? 1 : 0;
    j += (j < m && rows_ro(m, j + 1) <= L) ? 1 : 0;
    return j;
}
// ... and the node's storage slot: i is clamped into the row, so that the slot lies inside the column whatever j is
__device__ __forceinline__ int rows_slot_at(int m, int L, int j, int nei, int off_int)
{
    const int i = min(max(L - rows_ro(m, j), 0), m - j);
    int cls;
    return rows_slot(m, i, j, nei, off_int, cls);
}

}  // namespace hmg
