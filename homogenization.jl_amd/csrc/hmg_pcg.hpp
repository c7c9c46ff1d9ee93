// Jacobi-preconditioned CG smoother (hmg_grid_set_smoother(grid, 1)): what its host side (smooth_pcg() in hmg_smooth.cpp)
// and its kernels (hmg_pcg.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// The assembled diagonal is summed in fixed point, limb by limb (see hmg_pcg.hip): for limb = diag_limbs() - 1 down to 0
//   launch_operator_diag(.., limb, t);  interface sum of t;  launch_diag_accum(.., t, d, limb)
// t[slot, cell] = limb `limb` of floor(2^96 w), w = the cell-local diagonal of lambda M + K_sigma = sum_t scale_t(cell) *
// ctab[class(slot)][centre tap][t]
int diag_limbs();
void launch_operator_diag(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double lambda, int limb, double *t);
// d = t * 2^(32 limb - 96) for the top limb, d += ... below it
void launch_diag_accum(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const double *t, double *d, int limb);
// d (interface-summed diagonal) -> dinv: 0 on the entities flagged in the Dirichlet mask, 1 / d elsewhere
void launch_dinv_finish(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double *d);
// p = dinv o r; scal[s_out] = r . p
void launch_pcg_start(const Launch &L, double *p, const double *r, const double *dinv, int64_t n, int s_out);
// r -= alpha q; scal[s_out] = r . (dinv o r)
void launch_pcg_rupdate(const Launch &L, double *r, const double *q, const double *dinv, int64_t n, Ratio alpha, int s_out);
// x += alpha p; p = dinv o r + beta p
void launch_pcg_xp(const Launch &L, double *x, double *p, const double *r, const double *dinv, int64_t n, Ratio alpha, Ratio beta);

}  // namespace hmg
