// Per-cell gradient moments of a level vector (include/hmg.h: hmg_cell_moments) and of a pair of them (hmg_cell_pair_moments):
// what the host module (hmg_fields.cpp) and the kernels (hmg_fields.hip, hmg_fields_pair.hip, hmg_fields_window.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// Reference sums per cell: the quadratic forms of the stiffness terms of the class table, then the linear forms of dphi.
//   raw[c][t]      = sum_i v_i (T_t v_c)_i,  t = 0 .. nterm - 2   (term order 11, 12, 13, 22, 23, 33; 2D: 11, 12, 22; an
//                    off-diagonal term of the class table is A^(a,b) + A^(b,a), so its form is 2 q_ab)
//   raw[c][nq + a] = sum_i dphi[3 i + a] v_i,  a = 0 .. dim - 1
inline int cell_moments_nraw(int dim) { return dim * (dim + 1) / 2 + dim; }

// LDS of one workgroup: the class table without its mass term, the lattice image with its guard, one row of partial sums per wave
size_t cell_moments_lds_bytes(const LevelDev &lv);
// does one cell of this level fit the LDS of a compute unit, with the tables the kernel needs?
bool cell_moments_ok(const LevelDev &lv);
// raw[c][0 .. nraw) for the first ncells columns of v (column stride lv.ld); deterministic: the same bits in every run
void launch_cell_moments(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, double *raw);

// The bilinear counterpart for two vectors v, w of one level (w may be v):
//   raw[c][t]            = sum_i v_i (T_t w_c)_i,  t = 0 .. nterm - 2   (the same term order; an off-diagonal term is 2 sym q_ab)
//   raw[c][nq + a]       = sum_i dphi[3 i + a] v_i
//   raw[c][nq + dim + a] = sum_i dphi[3 i + a] w_i,  a = 0 .. dim - 1
inline int cell_pair_moments_nraw(int dim) { return dim * (dim + 1) / 2 + 2 * dim; }

// LDS of one workgroup: as above (one image: w's), with the wider rows of partial sums -- a verdict of its own
size_t cell_pair_moments_lds_bytes(const LevelDev &lv);
bool cell_pair_moments_ok(const LevelDev &lv);
// raw[c][0 .. nraw) for the first ncells columns of v and w (column stride lv.ld); deterministic: the same bits in every run
void launch_cell_pair_moments(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const double *w, double *raw);

// Cells larger than the LDS (hmg_fields_window.hip): the same raw sums, in the pair layout, from a rolling window of the LDS -- slabs
// of k-planes in 3D (st: the level's SlabTables, the lists of k_apply_slab), bands of lattice rows in 2D (closed forms, st unused).
// v == w (the same pointer) reads the column once; the single-vector sums are the first nq + dim of every row.
// can the window kernels address this level?  3D: levels with slab tables; 2D: m >= 2
bool cell_moments_window_ok(const LevelDev &lv, const SlabTables &st);
// raw[c][0 .. nraw) of the pair layout for the first ncells columns; throws on a level it cannot address and on null bases before
// any launch; deterministic: the same bits in every run and for every number of cells
void launch_cell_pair_moments_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                     const double *w, double *raw);

}  // namespace hmg
