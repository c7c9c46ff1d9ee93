// The binning rule of the per-cell histograms (include/hmg.h: hmg_histogram_bin, hmg_cell_histogram): ONE text for the host twin
// of hmg_histogram.cpp and for the kernels of hmg_histogram.hip and hmg_histogram_window.hip.
//
// Bins are floating-point buckets: emin < emax (-1022 <= emin, emax <= 1023) and s = sub_bits in 0 .. 5 give
//   nreg = (emax - emin) 2^s regular bins with the edges E_i = 2^(emin + i div 2^s) (1 + (i mod 2^s) / 2^s),
//   i = 0 .. nreg -- every edge an exact double --, and nbins = nreg + 3:
//   bin 0            everything below 2^emin: zeros of either sign, negatives, -inf, denormals
//   bin b, 1..nreg   [E_(b-1), E_b)
//   bin nreg + 1     q >= 2^emax, +inf included
//   bin nreg + 2     a NaN of either sign
// that is bin(q) = searchsorted(E, q, side = "right") for every q that is no NaN.
//
// Positive doubles order like their bit patterns, and the top 12 + s bits of a positive double are its octave and its sub-bin: the
// key is hi >> (20 - s), the bin the key minus the key of 2^emin, clamped.  Integer arithmetic on the high word alone (the low
// word only tells an infinity from a NaN whose payload sits there): no logarithm, no floating-point compare, no rounding that
// could differ between host and device.
// The rule holds for every such emin, emax and s; the kernel keeps a cell's histogram in LDS and serves nreg <= 1024
// (hmg_cell_histogram says so where it refuses more), the host twin serves them all.
#pragma once
#include "hmg_device.hpp"

#ifndef HMG_HD
#define HMG_HD __host__ __device__ __forceinline__
#endif

namespace hmg {

constexpr int HIST_MAX_SUB_BITS = 5;
constexpr int HIST_MAX_REGULAR = 1024;                     // regular bins the kernel serves at most
constexpr int HIST_MAX_BINS = HIST_MAX_REGULAR + 3;
constexpr int HIST_MAX_GROUPS = 65535;                     // groups of hmg_cell_histogram_groups: the second dimension of its launch

// the rule as the kernel takes it
struct HistogramRule {
    int shift;      // 20 - sub_bits
    int key0;       // key of 2^emin: (emin + 1023) << sub_bits
    int nreg;       // regular bins; nbins = nreg + 3
};

// parameters inside the rule?  0: yes; 1 emin, 2 emax, 3 their order, 4 sub_bits
HMG_HD int histogram_rule_check(int emin, int emax, int sub_bits)
{
    if (sub_bits < 0 || sub_bits > HIST_MAX_SUB_BITS) return 4;
    if (emin < -1022 || emin > 1023) return 1;
    if (emax < -1022 || emax > 1023) return 2;
    if (emin >= emax) return 3;
    return 0;
}

HMG_HD HistogramRule histogram_rule(int emin, int emax, int sub_bits)
{
    HistogramRule r;
    r.shift = 20 - sub_bits;
    r.key0 = (emin + 1023) << sub_bits;
    r.nreg = (emax - emin) << sub_bits;
    return r;
}

// the bin of the double with the high word hi and the low word lo
HMG_HD int histogram_bin(uint32_t hi, uint32_t lo, const HistogramRule &r)
{
    const uint32_t mag = hi & 0x7fffffffu;
    if (mag > 0x7ff00000u || (mag == 0x7ff00000u && lo != 0u)) return r.nreg + 2;      // NaN, quiet or signalling
    if (hi >> 31) return 0;                                                            // negatives, -0, -inf
    const int k = (int)(hi >> r.shift) - r.key0 + 1;                                   // (hi < 2^31: the key fits an int)
    return k < 0 ? 0 : (k > r.nreg + 1 ? r.nreg + 1 : k);
}

// edge i of the rule, i = 0 .. nreg: built from its bits, exact
HMG_HD uint64_t histogram_edge_bits(int i, int emin, int sub_bits)
{
    const uint64_t key = (uint64_t)(((int64_t)(emin + 1023) << sub_bits) + i);
    return key << (52 - sub_bits);
}

// ---- what the kernels alone share (hmg_histogram.hip: k_cell_histogram; hmg_histogram_window.hip: its slab and row-band forms) ----

// one workgroup-scope integer add to the LDS histogram
__device__ __forceinline__ void lds_count(int *hist, int bin, int n)
{
    (void)__hip_atomic_fetch_add(hist + bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the bins of a node's NEL values q and what each has to add: 1 where the element's bit of the mask mk is set, else 0
template <int NEL>
__device__ __forceinline__ void histogram_node_bins(const double *q, unsigned mk, const HistogramRule &rule, int *bin, int *cnt)
{
#pragma unroll
    for (int k = 0; k < NEL; ++k) {
        bin[k] = histogram_bin((uint32_t)__double2hiint(q[k]), (uint32_t)__double2loint(q[k]), rule);
        cnt[k] = (int)((mk >> k) & 1u);
    }
}

// the node's elements with one bin become one count: the first of them takes the others' (an element folded into an earlier one
// has 0 left and takes nothing: whatever shares its bin went the same way)
template <int NEL>
__device__ __forceinline__ void histogram_node_combine(const int *bin, int *cnt)
{
#pragma unroll
    for (int k = 0; k < NEL; ++k)
#pragma unroll
        for (int j = k + 1; j < NEL; ++j) {
            const int take = (bin[j] == bin[k] && cnt[k] > 0) ? cnt[j] : 0;
            cnt[k] += take;
            cnt[j] -= take;
        }
}

// the HIST_NODE form (hmg_histogram.hpp) of a node: combined in registers, one LDS add per distinct bin
template <int NEL>
__device__ __forceinline__ void histogram_node_add(int *hist, const int *bin, int *cnt)
{
    histogram_node_combine<NEL>(bin, cnt);
#pragma unroll
    for (int k = 0; k < NEL; ++k)
        if (cnt[k] > 0) lds_count(hist, bin[k], cnt[k]);
}

}  // namespace hmg
