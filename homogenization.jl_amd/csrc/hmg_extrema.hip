// HIP kernel for AMD CDNA4 (gfx950, wave64).
//
// k_cell_extrema: per coarse cell the maximum and the minimum, over the cell's fine elements T, of a quadratic form of the P1
// gradient of u = xi . x + v, and the number of elements on which it exceeds each of up to 8 thresholds (include/hmg.h:
// hmg_cell_extrema; the fold of the cell's geometry, form and xi into one row per cell is the host's, hmg_extrema.cpp):
//   q_T = (xi~ + g~_T) . Q~_c (xi~ + g~_T)
// The refined cell is the Kuhn triangulation of its lattice: with the basis a, b, c (2D: a, b) and s = a + b + c every element is
// {p, p + pi1, p + pi1 + pi2, p + s} for a permutation pi of the basis, and the successive differences of u along that path ARE
// the components of g~ (the gradient in the basis' dual coordinates): no per-element matrix.  Bit k of elem_mask[slot] says that
// the simplex of permutation k (lexicographic order) with its lowest vertex at the slot exists.
// One 8 B/DOF read of the column and one byte of mask per slot; 16 + 8 nthr bytes written per cell.  No operator, no lambda, no
// mask of constraints: the vector as stored.
//
// A workgroup walks cells blockIdx.x, blockIdx.x + gridDim.x, ...  Per cell the column goes into the LDS lattice image through
// lpos (zero guard behind the image); every thread takes the slots tid, tid + NT, ..., decodes pos32, reads the centre and the
// 7 (2D: 3) nodes above it -- every address clamped into the image and its guard, so that an element that does not exist reads
// some node of the image instead of leaving it -- and evaluates the 6 (2D: 2) forms; those whose bit is clear take no part.
// Maxima, minima and integer counts do not depend on any order: the same bits in every run and for every grid size.
// NaN: a comparison never picks one, so every thread notes whether some EXISTING element of its slots had a NaN q_T (integer
// maxima of the values' high words: 6 full-rate operations per slot, half the cost of 6 double-precision compares) and turns its
// maximum and minimum into NaN behind the slot loop; the picks of the folds across lanes and waves take a NaN and keep one.
// A cell's maximum and minimum are NaN exactly when one of its elements' values is; an infinite value is a value like any other;
// the counts compare, and a NaN compares false.
#include "hmg_extrema.hpp"
#include "hmg_stencil.hpp"

#include <algorithm>

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;

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

template <int DIM, int NT>
__global__ void __launch_bounds__(NT)
k_cell_extrema(LevelDev lv, const double *v, int64_t ncells, int g1, const uint8_t *__restrict__ elem_mask,
               const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    constexpr int NQ = DIM == 3 ? 6 : 3, NROW = NQ + DIM, NEL = DIM == 3 ? 6 : 2, NW = NT / 64;
    constexpr int NTHR = EX_MAX_THRESHOLDS;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nf = lv.nf, m = lv.m;
    double *xs = smem;                            // lattice image of v, g1 zeros behind it
    double *red = xs + ((nf + g1 + 1) & ~1);      // [NW][2]: maximum, minimum
    int *redc = (int *)(red + 2 * NW);            // [NW][NTHR]
    for (int q = tid; q < g1; q += NT) xs[nf + q] = 0.0;
    const int hi = nf + g1 - 1;
    const double inf = __builtin_huge_val();
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const double *vc = v + cell * lv.ld;
        for (int t = tid; t < nf; t += NT) xs[lv.lpos[t]] = vc[t];
        // the cell's row: Q~ (off-diagonal entries doubled here, once per cell) and xi~, the same in every lane
        const double *row = rows + cell * NROW;
        double Q[NQ], X[DIM];
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
        __syncthreads();                          // image (first cell: guard too) complete; red[] of the last cell read
        double mx = -inf, mn = inf;
        // the largest high word, signed and unsigned, of the values of this thread's existing elements: above +inf's a positive NaN,
        // above -inf's a negative one (a value is the result of arithmetic: its NaN is quiet, with a bit in the high word)
        int hs = 0;
        unsigned hu = 0;
        int cnt[NTHR];
#pragma unroll
        for (int j = 0; j < NTHR; ++j) cnt[j] = 0;
        for (int t = tid; t < nf; t += NT) {
            const unsigned mk = elem_mask[t];
            if (mk == 0) continue;                // no element has its lowest vertex here (the faces i = m - j - k, ...)
            int L, len, A, B, cls;
            decode32<DIM>(lv.pos32[t], m, L, len, A, B, cls);
            auto at = [&](int off) { return lds_ld(xs + min(max(L + off, 0), hi)); };
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
            double qh[NEL];                       // for the maximum and the counts: -inf where the element does not exist
#pragma unroll
            for (int k = 0; k < NEL; ++k) {
                const bool on = (mk >> k) & 1u;
                qh[k] = on ? q[k] : -inf;
                const double ql = on ? q[k] : inf;
                hs = max(hs, __double2hiint(qh[k]));
                hu = max(hu, (unsigned)__double2hiint(qh[k]));
                mx = qh[k] > mx ? qh[k] : mx;
                mn = ql < mn ? ql : mn;
            }
#pragma unroll
            for (int j = 0; j < NTHR; ++j)
                if (j < nthr) {                   // (the same in every lane: a scalar branch)
#pragma unroll
                    for (int k = 0; k < NEL; ++k) cnt[j] += qh[k] > thr.t[j] ? 1 : 0;
                }
        }
        // lanes by data-parallel moves, waves through LDS, one thread per output
        if (hs > 0x7ff00000 || hu > 0xfff00000u) mx = mn = __builtin_nan("");
        mx = wave_ext63<true>(mx);
        mn = wave_ext63<false>(mn);
#pragma unroll
        for (int j = 0; j < NTHR; ++j)
            if (j < nthr) cnt[j] = wave_isum63(cnt[j]);
        if (lane == 63) {
            red[2 * wave] = mx;
            red[2 * wave + 1] = mn;
#pragma unroll
            for (int j = 0; j < NTHR; ++j) redc[wave * NTHR + j] = cnt[j];
        }
        __syncthreads();                          // every wave is done with the image: the next cell's may be written
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
    }
}

template <int DIM, int NT>
void launch(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
            const ExtremaThresholds &thr, int nthr, double *out)
{
    auto kern = k_cell_extrema<DIM, NT>;
    const size_t lds = cell_extrema_lds_bytes(lv);
    if (lds > 48 * 1024) HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many workgroups as are resident at once; each walks its share of the cells
    int64_t per_cu = std::min<int64_t>((int64_t)(LDS_PER_CU / lds), 2048 / NT);
    per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu, 16));
    const int64_t grid = std::min<int64_t>(ncells, per_cu * std::max(L.num_cu, 1));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, v, ncells, lv.lds_g1, elem_mask, rows, thr, nthr, out);
    check_launch();
}

template <int DIM>
void launch_dim(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
                const ExtremaThresholds &thr, int nthr, double *out)
{
    if (lv.nf <= 256)
        launch<DIM, 64>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out);
    else if (lv.nf <= 4096)
        launch<DIM, 256>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out);
    else
        launch<DIM, 512>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out);
}

}  // namespace

size_t cell_extrema_lds_bytes(const LevelDev &lv)
{
    const size_t img = ((size_t)lv.nf + lv.lds_g1 + 1) & ~(size_t)1;
    return sizeof(double) * (img + (size_t)8 * 2) + sizeof(int) * (size_t)8 * EX_MAX_THRESHOLDS;   // (8 waves at most)
}

bool cell_extrema_ok(const LevelDev &lv)
{
    if (lv.dim != 2 && lv.dim != 3) return false;
    if (!lv.pos32 || !lv.lpos) return false;
    if (lv.lds_g0 != 0 || lv.lds_g1 < 0) return false;
    if (lv.dim == 3 ? lv.m > 63 : lv.m > 255) return false;        // the packed addressing words hold this level's values
    return lv.nf <= 0xffff && cell_extrema_lds_bytes(lv) <= LDS_PER_CU;
}

void launch_cell_extrema(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask,
                         const double *rows, const ExtremaThresholds &thr, int nthr, double *out)
{
    if (!cell_extrema_ok(lv)) throw std::runtime_error("cell extrema: one cell of this level does not fit the LDS");
    if (nthr < 0 || nthr > EX_MAX_THRESHOLDS) throw std::runtime_error("cell extrema: 0 to 8 thresholds");
    if (!v || !elem_mask || !rows || !out) throw std::runtime_error("cell extrema: null device pointer");
    if (ncells <= 0) return;
    if (lv.dim == 3)
        launch_dim<3>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out);
    else
        launch_dim<2>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out);
}

}  // namespace hmg
