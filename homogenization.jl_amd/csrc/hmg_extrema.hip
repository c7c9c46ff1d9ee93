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
// The evaluation of a node and the fold of a cell are extrema_node / extrema_fold of hmg_extrema_device.hpp, which the window
// kernels of cells larger than the LDS (hmg_extrema_window.hip) call too: the same bits on a level both serve.
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_stencil.hpp"

#include <algorithm>

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;

// The body of both kernels below.  W = ExtremaWhere is the located form (hmg_cell_extrema_where): the codes slot * 8 + k of the
// elements that hold maximum and minimum ride along in two registers and go to codes[cell][0 .. 2); every value is formed and
// picked as in the other form, which this parameter leaves as it was, instruction for instruction.
template <int DIM, int NT, class W>
__device__ __forceinline__ void cell_extrema_body(const LevelDev &lv, const double *v, int64_t ncells, int g1,
                                                  const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                                                  const ExtremaThresholds &thr, int nthr, double *__restrict__ out,
                                                  int *__restrict__ codes)
{
    constexpr int NQ = DIM == 3 ? 6 : 3, NROW = NQ + DIM, NW = NT / 64;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nf = lv.nf, m = lv.m;
    double *xs = smem;                            // lattice image of v, g1 zeros behind it
    double *red = xs + ((nf + g1 + 1) & ~1);      // [NW][2]: maximum, minimum
    int *redc = (int *)(red + 2 * NW);            // [NW][EX_MAX_THRESHOLDS]
    int *redw = redc + 8 * EX_MAX_THRESHOLDS;     // located form: [NW][2] codes, behind the counters of 8 waves
    for (int q = tid; q < g1; q += NT) xs[nf + q] = 0.0;
    const int hi = nf + g1 - 1;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const double *vc = v + cell * lv.ld;
        for (int t = tid; t < nf; t += NT) xs[lv.lpos[t]] = vc[t];
        double Q[NQ], X[DIM];
        extrema_row<DIM>(rows + cell * NROW, Q, X);
        __syncthreads();                          // image (first cell: guard too) complete; red[] of the last cell read
        ExtremaAcc acc;
        acc.reset();
        W wh;
        if constexpr (WHERE) wh.reset();
        for (int t = tid; t < nf; t += NT) {
            const unsigned mk = elem_mask[t];
            if (mk == 0) continue;                // no element has its lowest vertex here (the faces i = m - j - k, ...)
            int L, len, A, B, cls;
            decode32<DIM>(lv.pos32[t], m, L, len, A, B, cls);
            if constexpr (WHERE)
                extrema_node<DIM>(xs, L, len, A, B, 0, hi, mk, Q, X, thr, nthr, acc, t, &wh);
            else
                extrema_node<DIM>(xs, L, len, A, B, 0, hi, mk, Q, X, thr, nthr, acc);
        }
        // (its barrier: every wave is done with the image, the next cell's may be written)
        if constexpr (WHERE)
            extrema_fold<NW>(acc, nthr, wave, red, redc, out, cell, &wh, redw, codes);
        else
            extrema_fold<NW>(acc, nthr, wave, red, redc, out, cell);
    }
}

template <int DIM, int NT>
__global__ void __launch_bounds__(NT)
k_cell_extrema(LevelDev lv, const double *v, int64_t ncells, int g1, const uint8_t *__restrict__ elem_mask,
               const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    cell_extrema_body<DIM, NT, ExtremaNoWhere>(lv, v, ncells, g1, elem_mask, rows, thr, nthr, out, nullptr);
}

template <int DIM, int NT>
__global__ void __launch_bounds__(NT)
k_cell_extrema_where(LevelDev lv, const double *v, int64_t ncells, int g1, const uint8_t *__restrict__ elem_mask,
                     const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out,
                     int *__restrict__ codes)
{
    cell_extrema_body<DIM, NT, ExtremaWhere>(lv, v, ncells, g1, elem_mask, rows, thr, nthr, out, codes);
}

template <int DIM, int NT>
void launch(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
            const ExtremaThresholds &thr, int nthr, double *out, int *codes)
{
    const size_t lds = codes ? cell_extrema_where_lds_bytes(lv) : cell_extrema_lds_bytes(lv);
    const void *kern = codes ? (const void *)k_cell_extrema_where<DIM, NT> : (const void *)k_cell_extrema<DIM, NT>;
    if (lds > 48 * 1024) HMG_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many workgroups as are resident at once; each walks its share of the cells
    int64_t per_cu = std::min<int64_t>((int64_t)(LDS_PER_CU / lds), 2048 / NT);
    per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu, 16));
    const int64_t grid = std::min<int64_t>(ncells, per_cu * std::max(L.num_cu, 1));
    if (codes)
        hipLaunchKernelGGL((k_cell_extrema_where<DIM, NT>), dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, v, ncells, lv.lds_g1,
                           elem_mask, rows, thr, nthr, out, codes);
    else
        hipLaunchKernelGGL((k_cell_extrema<DIM, NT>), dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, v, ncells, lv.lds_g1,
                           elem_mask, rows, thr, nthr, out);
    check_launch();
}

template <int DIM>
void launch_dim(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask, const double *rows,
                const ExtremaThresholds &thr, int nthr, double *out, int *codes)
{
    if (lv.nf <= 256)
        launch<DIM, 64>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out, codes);
    else if (lv.nf <= 4096)
        launch<DIM, 256>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out, codes);
    else
        launch<DIM, 512>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out, codes);
}

}  // namespace

size_t cell_extrema_lds_bytes(const LevelDev &lv)
{
    const size_t img = ((size_t)lv.nf + lv.lds_g1 + 1) & ~(size_t)1;
    return sizeof(double) * (img + (size_t)8 * 2) + sizeof(int) * (size_t)8 * EX_MAX_THRESHOLDS;   // (8 waves at most)
}

// ... of the located form: per wave two codes more
size_t cell_extrema_where_lds_bytes(const LevelDev &lv) { return cell_extrema_lds_bytes(lv) + sizeof(int) * (size_t)8 * 2; }

bool cell_extrema_ok(const LevelDev &lv)
{
    if (lv.dim != 2 && lv.dim != 3) return false;
    if (!lv.pos32 || !lv.lpos) return false;
    if (lv.lds_g0 != 0 || lv.lds_g1 < 0) return false;
    if (lv.dim == 3 ? lv.m > 63 : lv.m > 255) return false;        // the packed addressing words hold this level's values
    return lv.nf <= 0xffff && cell_extrema_lds_bytes(lv) <= LDS_PER_CU;
}

void launch_cell_extrema(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const uint8_t *elem_mask,
                         const double *rows, const ExtremaThresholds &thr, int nthr, double *out, int *codes)
{
    if (!cell_extrema_ok(lv) || (codes && cell_extrema_where_lds_bytes(lv) > LDS_PER_CU))
        throw std::runtime_error("cell extrema: one cell of this level does not fit the LDS");
    if (nthr < 0 || nthr > EX_MAX_THRESHOLDS) throw std::runtime_error("cell extrema: 0 to 8 thresholds");
    if (!v || !elem_mask || !rows || !out) throw std::runtime_error("cell extrema: null device pointer");
    if (ncells <= 0) return;
    if (lv.dim == 3)
        launch_dim<3>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out, codes);
    else
        launch_dim<2>(L, lv, ncells, v, elem_mask, rows, thr, nthr, out, codes);
}

}  // namespace hmg
