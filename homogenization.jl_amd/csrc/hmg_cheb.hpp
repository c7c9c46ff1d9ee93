// Chebyshev-Jacobi smoother (hmg_grid_set_smoother_chebyshev): what its host side (smooth_cheb() and ensure_smoother_diag() in
// hmg_smooth.cpp) and its kernels (hmg_cheb.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// The rounding factor on a formed bound (the level-1 preconditioner's, hmg_coarse.cpp); an explicit bound is used as given.
constexpr double CHEB_SAFETY = 1.02;
// lambda_lo = lambda_hi / ratio where the caller names none (the ratio with the fewest V-cycles over the
// cases of its table)
constexpr double CHEB_DEFAULT_RATIO = 30.0;

// The coefficients of one smoothing, all known before its first launch (no reduction enters):
//   theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma1 = theta / delta, rho_0 = 1 / sigma1, rho_{k+1} = 1 / (2 sigma1 - rho_k)
//   d_0 = c0 dinv o r, c0 = 1 / theta;   d_{k+1} = c1[k] d_k + c2[k] dinv o r_{k+1}, c1[k] = rho_{k+1} rho_k, c2[k] = 2 rho_{k+1} / delta
struct ChebCoef {
    double theta, delta, sigma1, c0, rho;
    ChebCoef(double lo, double hi)
        : theta(0.5 * (hi + lo)), delta(0.5 * (hi - lo)), sigma1(theta / delta), c0(1.0 / theta), rho(1.0 / sigma1) {}
    void next(double &c1, double &c2)
    {
        const double rho1 = 1.0 / (2.0 * sigma1 - rho);
        c1 = rho1 * rho;
        c2 = 2.0 * rho1 / delta;
        rho = rho1;
    }
};

// s[slot, cell] = sum over the taps of | sum_t ctab[class(slot)][tap][t] * scale_t(cell) |: the absolute row sum of the cell's own
// lambda M + K_sigma at that slot (the products of launch_operator_diag, over all taps instead of the centre one); 0 in the padding
void launch_operator_rowabs(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double lambda, double *s);
// scal[slot] = max over the n entries of dinv[e] * s[e] (0 for n = 0; NaN if a term is NaN): block partials, then a fixed-order fold
void launch_cheb_max(const Launch &L, const double *dinv, const double *s, int64_t n, int slot);
// d = c0 * (dinv o r)
void launch_cheb_start(const Launch &L, double *d, const double *r, const double *dinv, int64_t n, double c0);
// x += d;  r -= Ad;  d = c1 d + c2 (dinv o r)
void launch_cheb_step(const Launch &L, double *x, double *d, double *r, const double *Ad, const double *dinv, int64_t n, double c1,
                      double c2);
// x += d;  with Ad: r -= Ad as well
void launch_cheb_tail(const Launch &L, double *x, const double *d, double *r, const double *Ad, int64_t n);

}  // namespace hmg
