// Per-cell extrema and exceedance counts of a quadratic form of the fine-element gradients of a level vector (include/hmg.h:
// hmg_cell_extrema): what the host module (hmg_extrema.cpp) and the kernels (hmg_extrema.hip, hmg_extrema_window.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// The fine elements of a cell are the Kuhn simplices {p, p + pi1, p + pi1 + pi2, p + s} of the lattice basis a, b, c (2D: a, b),
// s = a + b + c, p the lexicographically lowest vertex.  The kernel reaches the 7 (2D: 3) nodes above p through these taps of
// stencil_eval_v's numbering; build_element_tables (hmg_extrema.cpp) derives the taps from the stencil's direction list and
// refuses a grid where they differ.
constexpr int EX_TAP_A = 11, EX_TAP_B = 8, EX_TAP_C = 4, EX_TAP_AB = 5, EX_TAP_AC = 13, EX_TAP_BC = 10, EX_TAP_S = 1;   // 3D
constexpr int EX2_TAP_A = 5, EX2_TAP_B = 4, EX2_TAP_S = 1;                                                             // 2D
constexpr int EX_MAX_THRESHOLDS = 8;
// hmg_cell_extrema_where: an element's code is slot(p) * 8 + k, k its bit of the element mask; a thread that saw no element holds
constexpr int EX_NO_CODE = 0x7fffffff;

struct ExtremaThresholds {
    double t[EX_MAX_THRESHOLDS];
};

// numbers per cell in the folded row: Q~ = M^T Q M (order 11, 12, 13, 22, 23, 33; 2D: 11, 12, 22), then xi~ = M^-1 xi
inline int cell_extrema_nrow(int dim) { return dim * (dim + 1) / 2 + dim; }

// LDS of one workgroup: the lattice image with its guard, per wave a maximum, a minimum and the counters
size_t cell_extrema_lds_bytes(const LevelDev &lv);
// ... of the located form (codes given): per wave two codes more
size_t cell_extrema_where_lds_bytes(const LevelDev &lv);
// the levels served: those whose cell fits the LDS with the image (3D up to 6, 2D up to 8)
bool cell_extrema_ok(const LevelDev &lv);
// out[c][0] = max, out[c][1] = min of q over the fine elements of cell c, out[c][2 + j] = number of elements with q > thr.t[j],
// j < nthr, for the first ncells columns of v (column stride lv.ld).  elem_mask: one byte per slot (ElementTables::mask);
// rows: cell_extrema_nrow(dim) numbers per cell.  The same bits in every run and for every grid size.
// codes = nullptr: the kernels of hmg_cell_extrema.  codes given (device, 2 ints per cell): the located instantiations of the
// same bodies -- out has the same bits, and codes[c][0], codes[c][1] name the elements that hold the maximum and the minimum as
// slot(p) * 8 + k (p the element's lowest vertex, k its bit of the mask), among equal values (==) the lowest code; -1, -1 where
// the cell's extrema are NaN.  The same ints in every run, for every grid size and from either kernel family.
void launch_cell_extrema(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask,
                         const double *rows, const ExtremaThresholds &thr, int nthr, double *out, int *codes = nullptr);

// Cells larger than the LDS (hmg_extrema_window.hip): the same results in the same rows from a rolling window of the LDS -- slabs of
// k-planes in 3D (st: the level's SlabTables, the lists of k_apply_slab), bands of lattice rows in 2D (closed forms, st unused).
// Both kernel families evaluate a node with one function (hmg_extrema_device.hpp): the same bits on a level both serve.
// can the window kernels address this level?  3D: levels with slab tables; 2D: m >= 2
bool cell_extrema_window_ok(const LevelDev &lv, const SlabTables &st);
// out[c][0 .. 2 + nthr) for the first ncells columns; throws on a level it cannot address, on nthr outside 0 .. 8, on null bases and
// on more than 2^31 - 1 cells before any launch; the same bits in every run and for every number of cells
void launch_cell_extrema_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                const uint8_t *elem_mask, const double *rows, const ExtremaThresholds &thr, int nthr, double *out,
                                int *codes = nullptr);

}  // namespace hmg
