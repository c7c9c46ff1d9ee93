// Flexible CG with one retained direction, preconditioned by the V-cycle (include/hmg.h: hmg_fcg_*): what its host module
// (hmg_fcg.cpp) and its kernels (hmg_fcg.hip) share.
#pragma once

#include "hmg_device.hpp"

namespace hmg {

// The method's own scalars (device doubles, owned by the hmg_fcg object).  They outlive the V-cycle inside a step, so none of
// them lives in the context's scalar bank, whose slots the smoother and the level-1 solve overwrite.
enum { F_ALPHA = 0, F_BETA = 1, F_PQ = 2, F_PR = 3, F_COUNT = 4 };
// The bank serves as the landing place of a step's reductions only, because that is where the grid's scalar_sum hook sums
// over the ranks: the last three slots, which no kernel of the smoother or of the level-1 solve touches (hmg_device.hpp).  Nothing
// is kept there from one call to the next.
enum { FB_ZQ = 13, FB_PQ = 14, FB_PR = 15 };

struct FcgLaunch {
    hipStream_t stream;
    double *part;      // block partials: 2 per block of 512 entries
    double *fold;      // 2 x 256 folded partials
    double *fs;        // F_COUNT own scalars
    double *bank;      // the context's scalar bank (16 doubles)
};

int64_t fcg_blocks(int64_t n);                       // blocks of a streaming launch over n doubles
// bank[FB_ZQ] = z.q
void launch_fcg_dot_zq(const FcgLaunch &F, const double *z, const double *q, int64_t n);
// ... with z's last two or three CG updates still pending (option lazy_x; hmg_objects.hpp: PendingX): z with the updates u is formed,
// stored and used; u: saved_updates() of the record, its ratios read from the saved block u.scal as launch_cg_x_save left them
void launch_fcg_dot_zq_x(const FcgLaunch &F, double *z, const XUpdates &u, const double *q, int64_t n);
// first != 0: p = z, fs[F_BETA] = 0;  else beta = -bank[FB_ZQ] / fs[F_PQ], p = z + beta p, fs[F_BETA] = beta
void launch_fcg_direction(const FcgLaunch &F, double *p, const double *z, int64_t n, int first);
// bank[FB_PQ] = p.q, bank[FB_PR] = p.R
void launch_fcg_dots_pq_pr(const FcgLaunch &F, const double *p, const double *q, const double *R, int64_t n);
// alpha = bank[FB_PR] / bank[FB_PQ]; x += alpha p; R -= alpha q; fs[F_ALPHA, F_PQ, F_PR] = alpha, p.q, p.R
void launch_fcg_update(const FcgLaunch &F, double *x, double *R, const double *p, const double *q, int64_t n);

}  // namespace hmg
