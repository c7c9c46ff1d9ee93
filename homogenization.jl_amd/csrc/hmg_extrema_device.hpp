// Device helpers the per-cell extrema kernels share (hmg_extrema.hip: k_cell_extrema; hmg_extrema_window.hip: its slab and
// row-band forms): the cell's row, the evaluation of one node -- eight (2D: four) reads, six (two) values, the mask, the updates
// of maximum, minimum, NaN trackers and counters -- and the fold of a cell.  Maxima, minima and integer counts do not depend on
// any order, and both kernel families evaluate a node with this one function: on a level both serve they give the same bits.
#pragma once

#include "hmg_extrema.hpp"
#include "hmg_stencil.hpp"

#include <type_traits>

namespace hmg {

// maximum / minimum / integer sum over the wave by data-parallel moves (the pattern of wave_sum63): the result arrives in lane 63.
// Lanes a move does not reach keep `old`: the lane's own value for the extrema, 0 for the sum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_other(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
// the larger (MAX) or smaller of a and b; a NaN on either side is the result
template <bool MAX>
__device__ __forceinline__ double ext_pick(double a, double b)
{
    return ((MAX ? b > a : b < a) || b != b) ? b : a;
}
template <bool MAX>
__device__ __forceinline__ double wave_ext63(double v)
{
    auto pick = [](double a, double b) { return ext_pick<MAX>(a, b); };
    v = pick(v, dpp_other<0x111, 0xf>(v));     // row_shr:1
    v = pick(v, dpp_other<0x112, 0xf>(v));     // row_shr:2
    v = pick(v, dpp_other<0x114, 0xf>(v));     // row_shr:4
    v = pick(v, dpp_other<0x118, 0xf>(v));     // row_shr:8
    v = pick(v, dpp_other<0x142, 0xa>(v));     // row_bcast:15
    v = pick(v, dpp_other<0x143, 0xc>(v));     // row_bcast:31
    return v;
}
// The located forms (hmg_cell_extrema_where): next to a value travels the code slot * 8 + k of the element it was seen on.  The
// value is picked exactly as above, whatever the codes are -- the located kernels give the bits of the others --, and the code
// goes with it: the other side's where its value wins or is a NaN, the lower of the two where the values are equal (==).
template <bool MAX>
__device__ __forceinline__ int ext_pick_code(double a, int ca, double b, int cb)
{
    return ((MAX ? b > a : b < a) || b != b || (b == a && cb < ca)) ? cb : ca;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_otheri(int c)
{
    return __builtin_amdgcn_update_dpp(c, c, CTRL, ROW_MASK, 0xf, false);
}
// (a lane a move does not reach meets itself: its value and its code stay)
template <bool MAX, int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_pick_where(double &v, int &c)
{
    const double ov = dpp_other<CTRL, ROW_MASK>(v);
    const int oc = dpp_otheri<CTRL, ROW_MASK>(c);
    c = ext_pick_code<MAX>(v, c, ov, oc);
    v = ext_pick<MAX>(v, ov);
}
template <bool MAX>
__device__ __forceinline__ void wave_ext63_where(double &v, int &c)
{
    dpp_pick_where<MAX, 0x111, 0xf>(v, c);     // row_shr:1
    dpp_pick_where<MAX, 0x112, 0xf>(v, c);     // row_shr:2
    dpp_pick_where<MAX, 0x114, 0xf>(v, c);     // row_shr:4
    dpp_pick_where<MAX, 0x118, 0xf>(v, c);     // row_shr:8
    dpp_pick_where<MAX, 0x142, 0xa>(v, c);     // row_bcast:15
    dpp_pick_where<MAX, 0x143, 0xc>(v, c);     // row_bcast:31
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_addi(int v)
{
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_isum63(int v)
{
    v = dpp_addi<0x111, 0xf>(v);
    v = dpp_addi<0x112, 0xf>(v);
    v = dpp_addi<0x114, 0xf>(v);
    v = dpp_addi<0x118, 0xf>(v);
    v = dpp_addi<0x142, 0xa>(v);
    v = dpp_addi<0x143, 0xc>(v);
    return v;
}

// what a thread keeps of the elements it has seen
struct ExtremaAcc {
    double mx, mn;
    // the largest high word, signed and unsigned, of the values of this thread's existing elements: above +inf's a positive NaN,
    // above -inf's a negative one (a value is the result of arithmetic: its NaN is quiet, with a bit in the high word)
    int hs;
    unsigned hu;
    int cnt[EX_MAX_THRESHOLDS];
    __device__ __forceinline__ void reset()
    {
        mx = -__builtin_huge_val();
        mn = __builtin_huge_val();
        hs = 0;
        hu = 0;
#pragma unroll
        for (int j = 0; j < EX_MAX_THRESHOLDS; ++j) cnt[j] = 0;
    }
};
// ... and, in the located kernels, the codes of the elements that hold mx and mn: the lowest code among equal values
struct ExtremaWhere {
    int cmx, cmn;
    __device__ __forceinline__ void reset() { cmx = cmn = EX_NO_CODE; }
};
struct ExtremaNoWhere {};

// the cell's row: Q~ (off-diagonal entries doubled here, once per cell) and xi~, the same in every lane
template <int DIM>
__device__ __forceinline__ void extrema_row(const double *__restrict__ row, double *Q, double *X)
{
    constexpr int NQ = DIM == 3 ? 6 : 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q) Q[q] = row[q];
#pragma unroll
    for (int a = 0; a < DIM; ++a) X[a] = row[NQ + a];
    if (DIM == 3) {
        Q[1] *= 2.0;
        Q[2] *= 2.0;
        Q[4] *= 2.0;
    } else
        Q[1] *= 2.0;
}

// One node: xs is the base of a lattice image (or of a window of one: image - first lattice position held), L the node's lattice
// position, len / A / B its row length and plane offsets (decode32 and its kin), mk its byte of the element mask.  The centre and
// the 7 (2D: 3) nodes above it are read with every address clamped into [lo, hi], which the caller guarantees to be readable LDS;
// an element that does not exist reads some word in there and takes no part.
// The located form (W = ExtremaWhere) is told the node's slot and keeps the codes slot * 8 + k; the values are the same ones.
template <int DIM, class W = ExtremaNoWhere>
__device__ __forceinline__ void extrema_node(const double *xs, int L, int len, int A, int B, int lo, int hi, unsigned mk,
                                             const double *Q, const double *X, const ExtremaThresholds &thr, int nthr, ExtremaAcc &a,
                                             int slot = 0, W *w = nullptr)
{
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    constexpr int NEL = DIM == 3 ? 6 : 2, NTHR = EX_MAX_THRESHOLDS;
    const double inf = __builtin_huge_val();
    auto at = [&](int off) { return lds_ld(xs + min(max(L + off, lo), hi)); };
    double q[NEL];
    const double u0 = lds_ld(xs + L);
    if constexpr (DIM == 3) {
        // taps 11, 8, 4, 5, 13, 10, 1 of stencil_eval_v (hmg_extrema.hpp)
        const double ua = at(A), ub = at(len + 1 - B), uc = at(-len), uab = at(len), uac = at(A + 1 - len), ubc = at(1 - B),
                     us = at(1);
        auto form = [&](double ga, double gb, double gc) {
            ga += X[0];
            gb += X[1];
            gc += X[2];
            return ga * (Q[0] * ga + Q[1] * gb + Q[2] * gc) + gb * (Q[3] * gb + Q[4] * gc) + gc * (Q[5] * gc);
        };
        q[0] = form(ua - u0, uab - ua, us - uab);      // a, b, c
        q[1] = form(ua - u0, us - uac, uac - ua);      // a, c, b
        q[2] = form(uab - ub, ub - u0, us - uab);      // b, a, c
        q[3] = form(us - ubc, ub - u0, ubc - ub);      // b, c, a
        q[4] = form(uac - uc, us - uac, uc - u0);      // c, a, b
        q[5] = form(us - ubc, ubc - uc, uc - u0);      // c, b, a
    } else {
        // taps 5, 4, 1
        const double ua = at(len), ub = at(-len), us = at(1);
        auto form = [&](double ga, double gb) {
            ga += X[0];
            gb += X[1];
            return ga * (Q[0] * ga + Q[1] * gb) + gb * (Q[2] * gb);
        };
        q[0] = form(ua - u0, us - ua);                 // a, b
        q[1] = form(us - ub, ub - u0);                 // b, a
    }
    if constexpr (WHERE) {
        // The values are complete here, as in the other form: what the located form does with them below must not reach back into
        // how the compiler fuses the products above into multiply-adds (it did: other last bits than hmg_cell_extrema's).
#pragma unroll
        for (int k = 0; k < NEL; ++k) asm volatile("" : "+v"(q[k]));
    }
    double qh[NEL];                       // for the maximum and the counts: -inf where the element does not exist
#pragma unroll
    for (int k = 0; k < NEL; ++k) {
        const bool on = (mk >> k) & 1u;
        qh[k] = on ? q[k] : -inf;
        const double ql = on ? q[k] : inf;
        a.hs = max(a.hs, __double2hiint(qh[k]));
        a.hu = max(a.hu, (unsigned)__double2hiint(qh[k]));
        if constexpr (WHERE) {
            // (an element that does not exist names no place, not even while mx is still -inf.  Folding `on` into the code instead
            // -- the largest int where the element is missing -- costs the 3D kernels of hmg_extrema.hip a scalar spill)
            const int code = slot * 8 + k;
            w->cmx = on && (q[k] > a.mx || (q[k] == a.mx && code < w->cmx)) ? code : w->cmx;
            w->cmn = on && (q[k] < a.mn || (q[k] == a.mn && code < w->cmn)) ? code : w->cmn;
        }
        a.mx = qh[k] > a.mx ? qh[k] : a.mx;
        a.mn = ql < a.mn ? ql : a.mn;
    }
#pragma unroll
    for (int j = 0; j < NTHR; ++j)
        if (j < nthr) {                   // (the same in every lane: a scalar branch)
#pragma unroll
            for (int k = 0; k < NEL; ++k) a.cnt[j] += qh[k] > thr.t[j] ? 1 : 0;
        }
}

// The values of one node alone, for a kernel that does something else with them (hmg_histogram.hip): extrema_node's reads and
// expressions, and behind them the fence of its located form, so that what the caller does with the values cannot reach back into
// how the products are fused -- the bits of hmg_cell_extrema.  q[k] of an element whose bit of the mask is clear is some number.
template <int DIM>
__device__ __forceinline__ void extrema_values(const double *xs, int L, int len, int A, int B, int lo, int hi, const double *Q,
                                               const double *X, double *q)
{
    constexpr int NEL = DIM == 3 ? 6 : 2;
    auto at = [&](int off) { return lds_ld(xs + min(max(L + off, lo), hi)); };
    const double u0 = lds_ld(xs + L);
    if constexpr (DIM == 3) {
        const double ua = at(A), ub = at(len + 1 - B), uc = at(-len), uab = at(len), uac = at(A + 1 - len), ubc = at(1 - B),
                     us = at(1);
        auto form = [&](double ga, double gb, double gc) {
            ga += X[0];
            gb += X[1];
            gc += X[2];
            return ga * (Q[0] * ga + Q[1] * gb + Q[2] * gc) + gb * (Q[3] * gb + Q[4] * gc) + gc * (Q[5] * gc);
        };
        q[0] = form(ua - u0, uab - ua, us - uab);      // a, b, c
        q[1] = form(ua - u0, us - uac, uac - ua);      // a, c, b
        q[2] = form(uab - ub, ub - u0, us - uab);      // b, a, c
        q[3] = form(us - ubc, ub - u0, ubc - ub);      // b, c, a
        q[4] = form(uac - uc, us - uac, uc - u0);      // c, a, b
        q[5] = form(us - ubc, ubc - uc, uc - u0);      // c, b, a
    } else {
        const double ua = at(len), ub = at(-len), us = at(1);
        auto form = [&](double ga, double gb) {
            ga += X[0];
            gb += X[1];
            return ga * (Q[0] * ga + Q[1] * gb) + gb * (Q[2] * gb);
        };
        q[0] = form(ua - u0, us - ua);                 // a, b
        q[1] = form(us - ub, ub - u0);                 // b, a
    }
#pragma unroll
    for (int k = 0; k < NEL; ++k) asm volatile("" : "+v"(q[k]));
}

// One cell's results: lanes by data-parallel moves, waves through LDS (red: [NW][2] maximum, minimum; redc: [NW][8]), one thread
// per output, out[cell][0 .. 2 + nthr).  The barrier inside also says that every wave is done with the cell's image.
// (out and cell apart: the row's address formed here, behind the loops, keeps k_cell_extrema<3, *> free of scalar spills)
// The located form carries the codes with the values through both folds (redw: [NW][2] ints) and writes codes[cell][0 .. 2): the
// elements of maximum and minimum, -1 where the cell's extrema are NaN.
template <int NW, class W = ExtremaNoWhere>
__device__ __forceinline__ void extrema_fold(ExtremaAcc &a, int nthr, int wave, double *red, int *redc, double *__restrict__ out,
                                             int64_t cell, W *w = nullptr, int *redw = nullptr, int *__restrict__ codes = nullptr)
{
    constexpr int NTHR = EX_MAX_THRESHOLDS;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    const int tid = threadIdx.x, lane = tid & 63;
    if (a.hs > 0x7ff00000 || a.hu > 0xfff00000u) a.mx = a.mn = __builtin_nan("");
    if constexpr (WHERE) {
        wave_ext63_where<true>(a.mx, w->cmx);
        wave_ext63_where<false>(a.mn, w->cmn);
    } else {
        a.mx = wave_ext63<true>(a.mx);
        a.mn = wave_ext63<false>(a.mn);
    }
#pragma unroll
    for (int j = 0; j < NTHR; ++j)
        if (j < nthr) a.cnt[j] = wave_isum63(a.cnt[j]);
    if (lane == 63) {
        red[2 * wave] = a.mx;
        red[2 * wave + 1] = a.mn;
        if constexpr (WHERE) {
            redw[2 * wave] = w->cmx;
            redw[2 * wave + 1] = w->cmn;
        }
#pragma unroll
        for (int j = 0; j < NTHR; ++j) redc[wave * NTHR + j] = a.cnt[j];
    }
    __syncthreads();
    if (tid < 2 + nthr) {
        double r;
        if (tid == 0) {
            r = red[0];
            for (int k = 1; k < NW; ++k) r = ext_pick<true>(r, red[2 * k]);
        } else if (tid == 1) {
            r = red[1];
            for (int k = 1; k < NW; ++k) r = ext_pick<false>(r, red[2 * k + 1]);
        } else {
            int s = 0;
            for (int k = 0; k < NW; ++k) s += redc[k * NTHR + tid - 2];
            r = (double)s;
        }
        out[cell * (2 + nthr) + tid] = r;
    }
    if constexpr (WHERE) {
        if (tid < 2) {                    // the waves' (value, code) pairs once more, in the order of the values' fold above
            double r = red[tid];
            int c = redw[tid];
            for (int k = 1; k < NW; ++k) {
                const double o = red[2 * k + tid];
                const int oc = redw[2 * k + tid];
                c = tid == 0 ? ext_pick_code<true>(r, c, o, oc) : ext_pick_code<false>(r, c, o, oc);
                r = tid == 0 ? ext_pick<true>(r, o) : ext_pick<false>(r, o);
            }
            codes[cell * 2 + tid] = r != r ? -1 : c;
        }
    }
}

}  // namespace hmg
