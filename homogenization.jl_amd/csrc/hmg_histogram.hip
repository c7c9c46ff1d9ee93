// HIP kernel for AMD CDNA4 (gfx950, wave64).
//
// k_cell_histogram: per coarse cell the histogram, over the cell's fine elements T, of the quadratic form of hmg_cell_extrema
//   q_T = (xi~ + g~_T) . Q~_c (xi~ + g~_T)
// in the floating-point buckets of hmg_histogram_device.hpp (include/hmg.h: hmg_cell_histogram; rows and element mask are the
// host's, those of hmg_cell_extrema).  The walk is k_cell_extrema's (hmg_extrema.hip): a workgroup takes cells blockIdx.x,
// blockIdx.x + gridDim.x, ...; per cell the column goes into the LDS lattice image through lpos (zero guard behind the image);
// every thread takes the slots tid, tid + NT, ..., decodes pos32 and forms the 6 (2D: 2) values of the node with extrema_values
// (hmg_extrema_device.hpp) -- the expressions of extrema_node behind its fence: the bits of hmg_cell_extrema.  Every value whose
// bit of the mask is set is binned -- integer arithmetic on its high word -- and counted; an element that does not exist is
// counted nowhere.
// The histogram sits in LDS behind the image: nbins 32-bit counters, zero when a cell's walk begins, written with LDS integer
// adds, and behind the barrier that ends the walk flushed as one coalesced row out[cell * nbins ..] by the threads that zero it
// again.  No global atomics and no floating-point sums: the counts do not depend on any order -- the same ints in every run, for
// every launch shape and from every variant below.
//
// The same-bin hazard.  A smooth field puts all 64 lanes of a wave, and all elements of a node, into one or two bins, and LDS
// adds to one address serialise.  VAR says what is done about it (hmg_histogram.hpp; DESIGN section 4 has the measurements):
// HIST_PLAIN nothing; HIST_NODE, the default, combines the elements of a node in registers (15 integer compares in 3D) and adds
// once per distinct bin; HIST_WAVE then takes, per element slot, the bin of the first lane that has something to add, sums the
// counts of all lanes with that bin by data-parallel moves and lets one lane add the sum -- a field that is constant across the
// wave costs one add per 64 nodes instead of 384 --, and lanes with another bin add for themselves.  Measured (profiles/
// cell_histogram.txt, level 6): the plain form pays a factor 2.4 on a cell-wise constant field, the node form nothing, and the
// wave form's moves cost more on every field than the adds they save.
// The slot loop has the same trip count in every lane (slots past nf have an empty mask) so that the moves across the wave see
// every lane.
#include "hmg_histogram.hpp"
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_stencil.hpp"

#include <algorithm>

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;

template <int DIM, int NT, int VAR>
__global__ void __launch_bounds__(NT)
k_cell_histogram(LevelDev lv, const double *v, int64_t ncells, int g1, const uint8_t *__restrict__ elem_mask,
                 const double *__restrict__ rows, HistogramRule rule, int *__restrict__ out)
{
    constexpr int NQ = DIM == 3 ? 6 : 3, NROW = NQ + DIM, NEL = DIM == 3 ? 6 : 2;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nf = lv.nf, m = lv.m, nbins = rule.nreg + 3;
    double *xs = smem;                                   // lattice image of v, g1 zeros behind it
    int *hist = (int *)(xs + ((nf + g1 + 1) & ~1));      // [nbins]
    for (int q = tid; q < g1; q += NT) xs[nf + q] = 0.0;
    for (int b = tid; b < nbins; b += NT) hist[b] = 0;
    const int hi = nf + g1 - 1;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const double *vc = v + cell * lv.ld;
        for (int t = tid; t < nf; t += NT) xs[lv.lpos[t]] = vc[t];
        double Q[NQ], X[DIM];
        extrema_row<DIM>(rows + cell * NROW, Q, X);
        __syncthreads();                                 // image complete (first cell: guard and zeroed counters too)
        for (int t0 = 0; t0 < nf; t0 += NT) {
            const int t = t0 + tid;
            const unsigned mk = t < nf ? elem_mask[t] : 0u;
            // no element has its lowest vertex here (the faces i = m - j - k, ..., slots past the last)
            if constexpr (VAR == HIST_WAVE) {
                if (__builtin_amdgcn_ballot_w64(mk != 0u) == 0) continue;       // (the whole wave: a scalar branch)
            } else {
                if (mk == 0u) continue;
            }
            int L, len, A, B, cls;
            decode32<DIM>(lv.pos32[min(t, nf - 1)], m, L, len, A, B, cls);
            double q[NEL];
            extrema_values<DIM>(xs, L, len, A, B, 0, hi, Q, X, q);
            int bin[NEL], cnt[NEL];
            histogram_node_bins<NEL>(q, mk, rule, bin, cnt);
            if constexpr (VAR == HIST_PLAIN) {
#pragma unroll
                for (int k = 0; k < NEL; ++k)
                    if (cnt[k]) lds_count(hist, bin[k], 1);
            } else if constexpr (VAR == HIST_NODE) {
                histogram_node_add<NEL>(hist, bin, cnt);         // (hmg_histogram_device.hpp: the text the window kernels run)
            } else {
                histogram_node_combine<NEL>(bin, cnt);
#pragma unroll
                for (int k = 0; k < NEL; ++k) {
                    const bool act = cnt[k] > 0;
                    const uint64_t who = __builtin_amdgcn_ballot_w64(act);
                    if (who == 0) continue;                                  // (scalar)
                    const int b0 = __builtin_amdgcn_readlane(bin[k], (int)__builtin_ctzll(who));
                    const bool same = act && bin[k] == b0;
                    const int sum = wave_isum63(same ? cnt[k] : 0);          // lane 63: all of the wave's counts for b0
                    if (lane == 63) lds_count(hist, b0, sum);
                    if (act && !same) lds_count(hist, bin[k], cnt[k]);
                }
            }
        }
        __syncthreads();                                 // every wave is done with the image and with the counters
        int *row = out + cell * nbins;
        for (int b = tid; b < nbins; b += NT) {          // (a counter is read, and zeroed for the next cell, by one and the same thread)
            row[b] = hist[b];
            hist[b] = 0;
        }
    }
}

template <int DIM, int NT, int VAR>
void launch(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
            const HistogramRule &rule, int *out)
{
    const size_t lds = cell_histogram_lds_bytes(lv, rule.nreg + 3);
    if (lds > 48 * 1024)
        HMG_HIP_CHECK(hipFuncSetAttribute((const void *)k_cell_histogram<DIM, NT, VAR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many workgroups as are resident at once; each walks its share of the cells
    int64_t per_cu = std::min<int64_t>((int64_t)(LDS_PER_CU / lds), 2048 / NT);
    per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu, 16));
    const int64_t grid = std::min<int64_t>(ncells, per_cu * std::max(L.num_cu, 1));
    hipLaunchKernelGGL((k_cell_histogram<DIM, NT, VAR>), dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, v, ncells, lv.lds_g1,
                       elem_mask, rows, rule, out);
    check_launch();
}

// the choice by nf is launch_dim's of hmg_extrema.hip
template <int DIM, int VAR>
void launch_dim(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
                const HistogramRule &rule, int *out)
{
    if (lv.nf <= 256)
        launch<DIM, 64, VAR>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else if (lv.nf <= 4096)
        launch<DIM, 256, VAR>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else
        launch<DIM, 512, VAR>(L, lv, ncells, v, elem_mask, rows, rule, out);
}

template <int VAR>
void launch_var(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
                const HistogramRule &rule, int *out)
{
    if (lv.dim == 3)
        launch_dim<3, VAR>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else
        launch_dim<2, VAR>(L, lv, ncells, v, elem_mask, rows, rule, out);
}

constexpr int HG_NT = 256;           // threads per workgroup of k_histogram_groups: bins blockIdx.x * 256 ..
constexpr int HG_AHEAD = 8;          // rows in flight per thread

// Group sums of the per-cell rows (hmg_histogram.hpp: launch_histogram_groups).  blockIdx.y is the group, a thread takes one bin and
// walks the group's cells in the order of the list: the loads of a trip are 256 consecutive ints of one row.  HG_AHEAD rows are
// requested before the first of them is added; the additions themselves run in list order, one cell after the other -- the order is
// the interface's, whatever the launch shape.  int64 for the counts (a group may hold more than 2^31 elements); for the volume the
// product and the sum are rounded separately (mul_rn, add_rn below: never contracted into a multiply-add).
// A product and a sum that each round once, to nearest.  (This toolchain's __dmul_rn / __dadd_rn are a plain `x * y` and `x + y`
// compiled under the default contraction: inlined next to each other they come out as one v_fma_f64 -- seen in the ISA and in the
// last bits.  Here the contraction is off where the operations are written.)
__device__ __forceinline__ double mul_rn(double x, double y)
{
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ double add_rn(double x, double y)
{
#pragma clang fp contract(off)
    return x + y;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(HG_NT)
k_histogram_groups(int nbins, const int *__restrict__ rows, const int *__restrict__ group_ptr, const int *__restrict__ group_cells,
                   const double *__restrict__ w, long long *__restrict__ counts, double *__restrict__ volume)
{
    const int b = blockIdx.x * HG_NT + threadIdx.x, grp = blockIdx.y;
    if (b >= nbins) return;
    const int p0 = group_ptr[grp], p1 = group_ptr[grp + 1];
    long long n = 0;
    double vol = 0.0;
    for (int p = p0; p < p1; p += HG_AHEAD) {
        int c[HG_AHEAD], r[HG_AHEAD];
        double wc[HG_AHEAD];
#pragma unroll
        for (int a = 0; a < HG_AHEAD; ++a) c[a] = group_cells[min(p + a, p1 - 1)];   // (a trip is completed with copies of the last cell)
#pragma unroll
        for (int a = 0; a < HG_AHEAD; ++a) {
            r[a] = rows[(int64_t)c[a] * nbins + b];
            if constexpr (WEIGHTED) wc[a] = w[c[a]];
        }
#pragma unroll
        for (int a = 0; a < HG_AHEAD; ++a)
            if (p + a < p1) {
                n += r[a];
                if constexpr (WEIGHTED) vol = add_rn(vol, mul_rn(wc[a], (double)r[a]));
            }
    }
    counts[(int64_t)grp * nbins + b] = n;
    if constexpr (WEIGHTED) volume[(int64_t)grp * nbins + b] = vol;
}

}  // namespace

void launch_histogram_groups(const Launch &L, int nbins, int ngroups, const int *rows, const int *group_ptr, const int *group_cells,
                             const double *w, long long *counts, double *volume)
{
    if (nbins < 1 || nbins > HIST_MAX_BINS) throw std::runtime_error("histogram groups: number of bins out of range");
    if (ngroups < 1 || ngroups > HIST_MAX_GROUPS) throw std::runtime_error("histogram groups: 1 to 65535 groups");
    if ((w == nullptr) != (volume == nullptr)) throw std::runtime_error("histogram groups: weights and volume go together");
    if (!rows || !group_ptr || !group_cells || !counts) throw std::runtime_error("histogram groups: null device pointer");
    const dim3 grid((unsigned)((nbins + HG_NT - 1) / HG_NT), (unsigned)ngroups);
    if (w)
        hipLaunchKernelGGL(k_histogram_groups<true>, grid, dim3(HG_NT), 0, L.stream, nbins, rows, group_ptr, group_cells, w, counts, volume);
    else
        hipLaunchKernelGGL(k_histogram_groups<false>, grid, dim3(HG_NT), 0, L.stream, nbins, rows, group_ptr, group_cells, w, counts, volume);
    check_launch();
}

size_t cell_histogram_lds_bytes(const LevelDev &lv, int nbins)
{
    const size_t img = ((size_t)lv.nf + lv.lds_g1 + 1) & ~(size_t)1;
    return sizeof(double) * img + sizeof(int) * (((size_t)nbins + 1) & ~(size_t)1);
}

bool cell_histogram_ok(const LevelDev &lv) { return cell_extrema_ok(lv) && cell_histogram_lds_bytes(lv, HIST_MAX_BINS) <= LDS_PER_CU; }

void launch_cell_histogram(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask,
                           const double *rows, const HistogramRule &rule, int variant, int *out)
{
    if (!cell_histogram_ok(lv)) throw std::runtime_error("cell histogram: one cell of this level does not fit the LDS");
    if (rule.nreg < 1 || rule.nreg > HIST_MAX_REGULAR || rule.shift < 20 - HIST_MAX_SUB_BITS || rule.shift > 20 || rule.key0 < 0)
        throw std::runtime_error("cell histogram: bin parameters outside the rule");
    if (!v || !elem_mask || !rows || !out) throw std::runtime_error("cell histogram: null device pointer");
    if (ncells <= 0) return;
    if (variant == HIST_PLAIN)
        launch_var<HIST_PLAIN>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else if (variant == HIST_NODE)
        launch_var<HIST_NODE>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else if (variant == HIST_WAVE)
        launch_var<HIST_WAVE>(L, lv, ncells, v, elem_mask, rows, rule, out);
    else
        throw std::runtime_error("cell histogram: no such variant");
}

}  // namespace hmg
