// Per-cell gradient moments of a level vector (include/hmg.h: hmg_cell_moments) and of a pair of them (hmg_cell_pair_moments):
// what the host module (hmg_fields.cpp) and the kernels (hmg_fields.hip, hmg_fields_window.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// Reference sums per cell of two vectors v, w of one level: the bilinear forms of the stiffness terms of the class table, then the
// linear forms of dphi.  same: w is v (the same pointer) -- the forms are quadratic and the second set of linear forms is left out.
//   raw[c][t]            = sum_i v_i (T_t w_c)_i,  t = 0 .. nterm - 2   (term order 11, 12, 13, 22, 23, 33; 2D: 11, 12, 22; an
//                          off-diagonal term of the class table is A^(a,b) + A^(b,a), so its form is 2 sym q_ab)
//   raw[c][nq + a]       = sum_i dphi[3 i + a] v_i,  a = 0 .. dim - 1
//   raw[c][nq + dim + a] = sum_i dphi[3 i + a] w_i   (two vectors only)
inline int cell_moments_nraw(int dim, bool same) { return dim * (dim + 1) / 2 + (same ? 1 : 2) * dim; }

// LDS of one workgroup: the class table without its mass term, the lattice image of w with its guard, one row of partial sums per
// wave -- the row width makes the verdict of two vectors one of its own
size_t cell_moments_lds_bytes(const LevelDev &lv, bool same);
// does one cell of this level fit the LDS of a compute unit, with the tables the kernel needs?
bool cell_moments_ok(const LevelDev &lv, bool same);
// raw[c][0 .. nraw) for the first ncells columns of v and w (column stride lv.ld); v == w reads the column once; deterministic: the
// same bits in every run
void launch_cell_pair_moments(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const double *w, double *raw);

// Cells larger than the LDS (hmg_fields_window.hip): the same raw sums in the same rows from a rolling window of the LDS -- slabs
// of k-planes in 3D (st: the level's SlabTables, the lists of k_apply_slab), bands of lattice rows in 2D (closed forms, st unused).
// can the window kernels address this level?  3D: levels with slab tables; 2D: m >= 2
bool cell_moments_window_ok(const LevelDev &lv, const SlabTables &st);
// raw[c][0 .. nraw) for the first ncells columns; throws on a level it cannot address and on null bases before any launch;
// deterministic: the same bits in every run and for every number of cells
void launch_cell_pair_moments_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                     const double *w, double *raw);

}  // namespace hmg
