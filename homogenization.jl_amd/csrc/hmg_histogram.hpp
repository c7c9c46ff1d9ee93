// Per-cell histograms of a quadratic form of the fine-element gradients of a level vector (include/hmg.h: hmg_cell_histogram):
// what the host module (hmg_histogram.cpp) and the kernel (hmg_histogram.hip) share.  The binning rule itself is
// hmg_histogram_device.hpp.
#pragma once

#include "hmg_device.hpp"
#include "hmg_histogram_device.hpp"

namespace hmg {

// How a workgroup brings its counts into the LDS histogram (the context option "cell_histogram_variant"; the counts are the same
// integers from each, DESIGN section 4 has what each costs):
//   HIST_PLAIN  one LDS add per existing element
//   HIST_NODE   the 6 (2D: 2) elements of a node are combined in registers first: one add per distinct bin of the node (the
//               default: the flattest of the three -- a field that is constant over a cell costs what a random one costs)
//   HIST_WAVE   ... and per element slot the bin of the wave's first active lane is summed across the wave and added once by one
//               lane; lanes with another bin add for themselves
constexpr int HIST_PLAIN = 0, HIST_NODE = 1, HIST_WAVE = 2, HIST_VARIANTS = 3;
constexpr int HIST_DEFAULT = HIST_NODE;

// LDS of one workgroup: the lattice image with its guard, behind it nbins counters
size_t cell_histogram_lds_bytes(const LevelDev &lv, int nbins);
// the levels served: those whose cell fits the LDS together with the largest histogram (3D up to 6, 2D up to 8)
bool cell_histogram_ok(const LevelDev &lv);
// out[c * nbins + b], nbins = rule.nreg + 3: the number of fine elements of cell c whose value falls into bin b, for the first
// ncells columns of v (column stride lv.ld).  elem_mask and rows are those of launch_cell_extrema, and so are the values, bit for
// bit.  Integer counts, no global atomics: the same ints in every run, for every grid size and from every variant.
void launch_cell_histogram(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask,
                           const double *rows, const HistogramRule &rule, int variant, int *out);

// Cells larger than the LDS (hmg_histogram_window.hip): the same rows from a rolling window of the LDS, with the walk every window
// kernel of the per-cell results shares (hmg_cell_window.hpp) -- slabs of k-planes in 3D (st: the level's SlabTables), bands of
// lattice rows in 2D (closed forms, st unused).  LDS: [window | nbins counters].  A node is evaluated and counted with the functions
// k_cell_histogram calls, in its HIST_NODE form alone (the variant has no say here): the same ints on a level both serve.
// can the window kernels address this level?  the walk's layout checks, and the window fits the LDS together with HIST_MAX_BINS
// counters (3D: one workgroup per CU; 2D: two)
bool cell_histogram_window_ok(const LevelDev &lv, const SlabTables &st);
// out[c * nbins + b] for the first ncells columns; throws on a level it cannot address, on bin parameters outside the rule, on null
// bases and on more than 2^31 - 1 cells before any launch; the same ints in every run and for every number of cells
void launch_cell_histogram_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                  const uint8_t *elem_mask, const double *rows, const HistogramRule &rule, int *out);

// Sums of the per-cell rows over groups of cells (hmg_cell_histogram_groups; k_histogram_groups of hmg_histogram.hip):
//   counts[g * nbins + b] = sum of rows[c * nbins + b] over the cells c of group g, in int64;
//   volume[g * nbins + b] = sum of w[c] * rows[c * nbins + b] in FP64, the cells taken in the order of the list (the host gives
//   ascending cell ids), from 0.0, product and sum rounded separately (no fused multiply-add) -- volume and w both null or both given.
// group_ptr[ngroups + 1], group_cells[group_ptr[ngroups]]: a CSR of cells per group.  One thread per (group, bin): loads coalesced
// across bins, no atomics; the same bits for every launch shape and in every run.
void launch_histogram_groups(const Launch &L, int nbins, int ngroups, const int *rows, const int *group_ptr, const int *group_cells,
                             const double *w, long long *counts, double *volume);

}  // namespace hmg
