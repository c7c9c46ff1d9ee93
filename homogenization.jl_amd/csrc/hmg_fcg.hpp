// Flexible CG with one retained direction, preconditioned by the V-cycle (include/hmg.h: hmg_fcg_*): what its host module
// (hmg_fcg.cpp), its kernels (hmg_fcg.hip) and the hooks it needs inside hmg_capi.cpp share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct hmg_ctx;
struct hmg_grid;
struct hmg_vec;

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
// first != 0: p = z, fs[F_BETA] = 0;  else beta = -bank[FB_ZQ] / fs[F_PQ], p = z + beta p, fs[F_BETA] = beta
void launch_fcg_direction(const FcgLaunch &F, double *p, const double *z, int64_t n, int first);
// bank[FB_PQ] = p.q, bank[FB_PR] = p.R
void launch_fcg_dots_pq_pr(const FcgLaunch &F, const double *p, const double *q, const double *R, int64_t n);
// alpha = bank[FB_PR] / bank[FB_PQ]; x += alpha p; R -= alpha q; fs[F_ALPHA, F_PQ, F_PR] = alpha, p.q, p.R
void launch_fcg_update(const FcgLaunch &F, double *x, double *R, const double *p, const double *q, int64_t n);

// ---- hooks into hmg_capi.cpp (they throw std::runtime_error) ---------------------------------------------------------
hmg_ctx *fcg_hook_ctx(hmg_grid *g);
// v is a level vector of this grid and level that holds the grid's current cells; returns its device pointer
double *fcg_hook_vec(const hmg_grid *g, int level, const hmg_vec *v, const char *name);
int64_t fcg_hook_len(const hmg_grid *g, int level);          // ld * current cells
// counts the operators this grid has had: hmg_grid_set_operator, hmg_grid_set_lambda and hmg_grid_shrink each add one
uint64_t fcg_hook_epoch(const hmg_grid *g);
// hmg_vcycle on a zero initial guess: where the smoother's form lets the top level be entered with a zero that is never written
// (zero_entry_ok) it is, otherwise x is filled first -- the same bits either way
void fcg_hook_vcycle_zero(hmg_grid *g, int top_level, int steps, int steps_coarse, hmg_vec **states);
// sum over the ranks of bank[slot .. slot + count) through the grid's scalar_sum hook (nothing on an unpartitioned grid)
void fcg_hook_scalar_sum(hmg_grid *g, int slot, int count);
// device memory of count doubles, zero-filled on the context's stream (counted by "device_allocs"); throws if it is not there
double *fcg_hook_alloc(hmg_ctx *c, size_t count);
void fcg_hook_free(hmg_ctx *c, double *p);
void fcg_hook_account(hmg_ctx *c, int64_t fcg_bytes_delta);   // hmg_ctx_counter "fcg_bytes"

}  // namespace hmg
