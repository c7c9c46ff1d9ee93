// Device helpers the per-cell moment kernels share (hmg_fields.hip: k_cell_pair_moments; hmg_fields_window.hip: its slab and
// row-band forms).
#pragma once

#include "hmg_stencil.hpp"

namespace hmg {

template <int DIM>
__device__ __forceinline__ void read_taps(const double *xs, int L, int len, int A, int B, int hi, bool clamp, double *tap)
{
    // tap numbering of stencil_eval_v; clamp: surface nodes, whose zero-weight taps may leave the image on either side
    auto at = [&](int off) {
        int q = L + off;
        if (clamp) q = min(max(q, 0), hi);
        return lds_ld(xs + q);
    };
    tap[0] = lds_ld(xs + L);
    tap[1] = at(1);
    tap[2] = at(-1);
    tap[3] = at(len - 1);
    tap[4] = at(-len);
    tap[5] = at(len);
    tap[6] = at(-len - 1);
    if (DIM == 3) {
        tap[7] = at(A - len);
        tap[8] = at(len + 1 - B);
        tap[9] = at(A - 1);
        tap[10] = at(1 - B);
        tap[11] = at(A);
        tap[12] = at(-B);
        tap[13] = at(A + 1 - len);
        tap[14] = at(len - B);
    }
}

// one cell's sums: lanes by data-parallel moves, waves in ascending order by one thread per sum; red is [NT / 64][NR], wave the
// caller's tid >> 6 (in a scalar register or not, as its own loops want it)
template <int NR, int NT>
__device__ __forceinline__ void fold_cell(const double (&acc)[NR], int wave, double *red, double *__restrict__ out)
{
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double ws = wave_sum63(acc[r]);
        if (lane == 63) red[wave * NR + r] = ws;
    }
    __syncthreads();
    if (tid < NR) {
        double sum = 0.0;
        for (int k = 0; k < NT / 64; ++k) sum += red[k * NR + tid];
        out[tid] = sum;
    }
}

}  // namespace hmg
