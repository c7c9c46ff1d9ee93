// HIP kernel for AMD CDNA4 (gfx950, wave64).
//
// k_cell_pair_moments: per coarse cell the reference sums behind the symmetrised cross moment of the gradients of two level vectors
// v, w of one level, and -- SAME: w is v -- behind the mean gradient and the Gram tensor of the gradient of one (include/hmg.h:
// hmg_cell_pair_moments, hmg_cell_moments; the transform to physical moments is the host's, hmg_fields.cpp):
//   raw[c][t]            = sum_i v_i (T_t w_c)_i     the stiffness terms of the class table one by one, before any coefficient row
//                                                    (T_t is symmetric: the tapped vector is w, the multiplying one v)
//   raw[c][nq + a]       = sum_i dphi[3 i + a] v_i   the table behind hmg_rhs_axi_grad (zero on the cell interior: skipped by the
//   raw[c][nq + dim + a] = sum_i dphi[3 i + a] w_i   interior waves); the second set only where w is another vector
// SAME: one 8 B/DOF read of the column, 72 B (2D: 40 B) written per cell; two vectors: 16 B/DOF, 96 B (2D: 56 B).  No mass term, no
// lambda, no coefficient row, no weight cache, no Dirichlet mask: the moments are of the vectors as stored.
//
// A workgroup walks cells blockIdx.x, blockIdx.x + gridDim.x, ...  Per cell ONLY w goes into the LDS lattice image through lpos,
// as in k_apply (zero guard behind the image, zero-weight taps below it clamped to 0); every thread takes the slots tid,
// tid + NT, ..., decodes pos32, reads the 15 (2D: 7) taps of w once and adds v_s * sum_dir ctab[cls][dir][t] * tap_dir to its sum
// of term t.  v_s is the centre tap where w is v; otherwise it is read straight from the column (coalesced: no second image),
// after the barrier that completes the image, from global memory that nothing writes.
// A wave whose 64 slots are all of one entity class -- entity-major storage: all but the waves that straddle two entities
// -- takes that class row by scalar loads; the other waves read their lanes' rows from an LDS copy of the table.
// Reduction: lanes by data-parallel moves, waves in ascending order by one thread per sum -- a fixed order, the same bits in
// every run and for every grid size.
#include "hmg_fields.hpp"
#include "hmg_fields_device.hpp"

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;

template <int DIM, int NT, bool SAME>
__global__ void __launch_bounds__(NT)
k_cell_pair_moments(LevelDev lv, const double *v, const double *w, int64_t ncells, int g1, double *__restrict__ raw)
{
    constexpr int NDIR = DIM == 3 ? 15 : 7;
    constexpr int NTERM = DIM == 3 ? 7 : 4;
    constexpr int NQ = NTERM - 1, NR = NQ + (SAME ? 1 : 2) * DIM;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nf = lv.nf, m = lv.m;
    const int ncw = (lv.ncls * NDIR * NQ + 1) & ~1;
    double *cs = smem;                         // [ncls][NDIR][NQ]: the class table without its mass term
    double *xs = smem + ncw;                   // lattice image of w, g1 zeros behind it
    double *red = xs + ((nf + g1 + 1) & ~1);   // [NT / 64][NR]
    for (int q = tid; q < lv.ncls * NDIR * NQ; q += NT) cs[q] = lv.ctab[(size_t)(q / NQ) * NTERM + q % NQ];
    for (int q = tid; q < g1; q += NT) xs[nf + q] = 0.0;
    const int hi = nf + g1 - 1;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const double *vc = v + cell * lv.ld, *wc = w + cell * lv.ld;
        for (int t = tid; t < nf; t += NT) xs[lv.lpos[t]] = wc[t];
        __syncthreads();                       // image (first cell: table and guard too) complete; red[] of the last cell read
        double acc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] = 0.0;
        for (int t0 = wave * 64; t0 < nf; t0 += NT) {
            const int t = t0 + lane;
            const bool act = t < nf;
            int L = 0, len = 0, A = 0, B = 0, cls = 0;
            double vs = 0.0;                   // the multiplying operand at this slot
            if (act) {
                if constexpr (!SAME) vs = vc[t];   // (requested ahead of the taps)
                decode32<DIM>(lv.pos32[t], m, L, len, A, B, cls);
            }
            double tap[NDIR], s[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q] = 0.0;
            // entity-major storage: the 64 consecutive slots of a wave are mostly of ONE entity class (a level-6 face has 465 interior
            // nodes, the cell interior 4495) -- such a wave takes the class row by scalar loads
            const int cls0 = __builtin_amdgcn_readfirstlane(cls);
            if (__builtin_amdgcn_ballot_w64(act && cls == cls0) == ~0ull) {
                read_taps<DIM>(xs, L, len, A, B, hi, cls0 != 0, tap);
                if constexpr (SAME) vs = tap[0];
                if (cls0 != 0) {               // (dphi is zero on the cell interior; in front of the products, see below)
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        const double dp = lv.dphi[3 * t + a];
                        acc[NQ + a] += dp * vs;
                        if constexpr (!SAME) acc[NQ + DIM + a] += dp * tap[0];
                    }
                }
                // (the row's 90 terms do not fit the scalar registers: an opaque pointer keeps the backend from hoisting their loads out
                //  of the slot loop into vector registers -- they are fetched through the scalar cache where they are used)
                auto *c0 = HMG_KP(double, lv.ctab) + cls0 * (NDIR * NTERM);
                asm volatile("" : "+s"(c0));
#pragma unroll
                for (int d = 0; d < NDIR; ++d)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s[q] += c0[d * NTERM + q] * tap[d];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
            } else if (act) {
                double dp[DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) dp[a] = lv.dphi[3 * t + a];
                read_taps<DIM>(xs, L, len, A, B, hi, cls != 0, tap);
                if constexpr (SAME) vs = tap[0];
                const double *cr = cs + cls * (NDIR * NQ);
#pragma unroll
                for (int d = 0; d < NDIR; ++d) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s[q] += lds_ld(cr + d * NQ + q) * tap[d];
                    // (ordered LDS reads and a scheduling fence: without them the backend requests the lane's whole row, 90 terms, ahead of the first product
                    //  -- 250 registers, one workgroup per CU)
                    __builtin_amdgcn_sched_barrier(0);
                }
                // (each branch adds to its own sums, and no branch follows the products: the backend sinks them behind the next join
                //  and keeps the row's 90 terms alive until there.  dphi is zero on the few interior slots that come this way.)
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    acc[NQ + a] += dp[a] * vs;
                    if constexpr (!SAME) acc[NQ + DIM + a] += dp[a] * tap[0];
                }
            }
        }
        fold_cell<NR, NT>(acc, wave, red, raw + cell * NR);   // (its barrier: every wave is done with the image)
    }
}

template <int DIM, int NT, bool SAME>
void launch(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const double *w, double *raw)
{
    auto kern = k_cell_pair_moments<DIM, NT, SAME>;
    const size_t lds = cell_moments_lds_bytes(lv, SAME);
    if (lds > 48 * 1024) HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many workgroups as are resident at once; each walks its share of the cells
    int64_t per_cu = std::min<int64_t>((int64_t)(LDS_PER_CU / lds), 2048 / NT);
    per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu, 16));
    const int64_t grid = std::min<int64_t>(ncells, per_cu * std::max(L.num_cu, 1));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, v, w, ncells, lv.lds_g1, raw);
    check_launch();
}

template <int DIM, bool SAME>
void launch_dim(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const double *w, double *raw)
{
    if (lv.nf <= 256)
        launch<DIM, 64, SAME>(L, lv, ncells, v, w, raw);
    else if (lv.nf <= 4096)
        launch<DIM, 256, SAME>(L, lv, ncells, v, w, raw);
    else
        launch<DIM, 512, SAME>(L, lv, ncells, v, w, raw);
}

}  // namespace

size_t cell_moments_lds_bytes(const LevelDev &lv, bool same)
{
    const int nq = lv.nterm - 1;
    const size_t ncw = ((size_t)lv.ncls * lv.ndir * nq + 1) & ~(size_t)1;
    const size_t img = ((size_t)lv.nf + lv.lds_g1 + 1) & ~(size_t)1;
    return sizeof(double) * (ncw + img + (size_t)8 * (nq + (same ? 1 : 2) * lv.dim));   // (8 waves at most)
}

bool cell_moments_ok(const LevelDev &lv, bool same)
{
    if (lv.dim != 2 && lv.dim != 3) return false;
    if (!lv.pos32 || !lv.lpos || !lv.ctab || !lv.dphi) return false;
    if (lv.nterm != (lv.dim == 3 ? 7 : 4) || lv.ndir != (lv.dim == 3 ? 15 : 7)) return false;
    if (lv.lds_g0 != 0 || lv.lds_g1 < 0) return false;
    if (lv.dim == 3 ? lv.m > 63 : lv.m > 255) return false;        // the packed addressing words hold this level's values
    return lv.nf <= 0xffff && cell_moments_lds_bytes(lv, same) <= LDS_PER_CU;
}

void launch_cell_pair_moments(const Launch &L, const LevelDev &lv, int64_t ncells, const double *v, const double *w, double *raw)
{
    const bool same = v == w;
    if (!cell_moments_ok(lv, same))
        throw std::runtime_error(same ? "cell moments: one cell of this level does not fit the LDS"
                                      : "cell pair moments: one cell of this level does not fit the LDS");
    if (ncells <= 0) return;
    if (lv.dim == 3)
        same ? launch_dim<3, true>(L, lv, ncells, v, w, raw) : launch_dim<3, false>(L, lv, ncells, v, w, raw);
    else
        same ? launch_dim<2, true>(L, lv, ncells, v, w, raw) : launch_dim<2, false>(L, lv, ncells, v, w, raw);
}

}  // namespace hmg
