// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell pair moments of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the raw sums of k_cell_pair_moments
// (hmg_fields.hip, hmg_fields.hpp) in the same row layout,
//   raw[c][t]            = sum_i v_i (T_t w_c)_i,   raw[c][nq + a] = sum_i dphi[3 i + a] v_i,   raw[c][nq + dim + a] = sum_i dphi[3 i + a] w_i
// (the last set only where w is another vector), formed while the cell walks through a ROLLING window of the LDS, as the operator
// applies of those levels do:
//   k_cell_pair_moments_slab (3D) follows k_apply_slab (hmg_apply.hip): slabs of k-planes from SlabTables -- the window holds
//     planes [k0-1, k1], planes k0-1 and k0 move to its front LDS -> LDS, the new planes come from HBM through ld_word, the nodes
//     of planes [k0, k1) are taken from cp_word / cp_slot, surface entries first (decode32w), then the cell interior (decode_lattice);
//   k_cell_pair_moments_rows (2D) follows k_apply_rows (hmg_apply_rows.hip): bands of lattice rows in closed form (rows_band_end,
//     rows_row_of, rows_slot), two rows moved in registers, no per-level tables.
// One workgroup per cell.  Only w goes into the window; v is read at the evaluated node's storage slot, or, where both columns are
// the same (SAME: one handle given twice, the single-vector entry point), taken from the centre tap -- 8 B/DOF instead of 16.  Per
// node the 15 (7) taps are read once; the addressing is that of stencil_eval_c / stencil_eval_v with the window's base img - lo:
// a zero-weight tap below the image is clamped to 0 (that can happen in the first slab / band only, where lo = 0), the upper end
// is the window's zero guard, and what lies behind the moved planes is zeroed before the loads.  The interior class row comes by
// scalar loads (3D: 90 terms, 2D: 21; an opaque pointer keeps them inside the loop and out of vector registers); a surface
// node takes its row per lane from an LDS copy of the class table without its mass term.  The sums stay in registers across the
// slabs / bands and are folded ONCE per cell -- lanes by data-parallel moves, waves in ascending order: the same bits in every
// run, whatever the number of cells.  No global store before that fold.
// LDS: 3D window (<= 70 KB) + table (10.8 KB) + partial sums (1.5 KB): one 1024-thread workgroup per CU, which the register need
// asks for anyway (12 sums + 15 taps + 6 products = 66 VGPRs of doubles: not a 64-VGPR kernel; one workgroup leaves 128).  2D:
// window 76.8 KB + table and sums 2 KB, 60 VGPRs: two workgroups per CU, as k_apply_rows (no occupancy bound in __launch_bounds__:
// it caps the scalar registers at 80 and the kernel spilled them; tests/test_cell_moments_kernel_resources.py holds the 64).
#include "hmg_fields.hpp"
#include "hmg_fields_device.hpp"
#include "hmg_rows_window.hpp"

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr int SW_NT = 1024;          // threads per workgroup of the slab form
constexpr int SW_MV = 5;             // values per thread of its window move (two planes of level 7: 4225 nodes)
constexpr int SW_HB = 4;             // loads in flight per thread in its load phase

// The taps of one node in the tap numbering of stencil_eval_v, from a window whose base is xs = img - lo.  clamp (surface nodes):
// the taps stencil_eval_c clamps -- the ones that may leave the image below -- are clamped to lattice position 0.
template <int DIM>
__device__ __forceinline__ void window_taps(const double *xs, int L, int len, int A, int B, bool clamp, double *tap)
{
    auto low = [&](int off) {
        int q = L + off;
        if (clamp) q = max(q, 0);
        return lds_ld(xs + q);
    };
    const double *p = xs + L;
    tap[0] = lds_ld(p);
    tap[1] = lds_ld(p + 1);
    tap[2] = low(-1);
    tap[3] = lds_ld(p + len - 1);
    tap[4] = low(-len);
    tap[5] = lds_ld(p + len);
    tap[6] = low(-len - 1);
    if (DIM == 3) {
        tap[7] = lds_ld(p + A - len);
        tap[8] = low(len + 1 - B);
        tap[9] = lds_ld(p + A - 1);
        tap[10] = low(1 - B);
        tap[11] = lds_ld(p + A);
        tap[12] = low(-B);
        tap[13] = lds_ld(p + A + 1 - len);
        tap[14] = low(len - B);
    }
}

template <bool SAME>
__global__ void __launch_bounds__(SW_NT)
k_cell_pair_moments_slab(LevelDev lv, const double *v, const double *w, SlabTables st, double *__restrict__ raw)
{
    constexpr int DIM = 3, NDIR = 15, NTERM = 7, NQ = NTERM - 1, NR = NQ + (SAME ? 1 : 2) * DIM, NT = SW_NT, HB = SW_HB, MV = SW_MV;
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int m = lv.m;
    const int ncw = (lv.ncls * NDIR * NQ + 1) & ~1;
    double *cs = smem;                        // [ncls][NDIR][NQ]: the class table without its mass term
    double *red = cs + ncw;                   // [NT / 64][NR]
    double *img = red + (NT / 64) * NR;       // st.lds_nodes doubles: [planes k0-1 .. k1 | zero guard]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld, *wc = w + cell * lv.ld;
    for (int q = tid; q < lv.ncls * NDIR * NQ; q += NT) cs[q] = lv.ctab[(size_t)(q / NQ) * NTERM + q % NQ];
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    auto plane_off = [&](int k) {   // PO(k) = number of lattice nodes in planes < k
        if (k <= 0) return 0;
        if (k > m + 1) k = m + 1;
        const long long n1 = m + 1, n2 = m + 1 - k;
        return (int)((n1 * (n1 + 1) * (n1 + 2) - n2 * (n2 + 1) * (n2 + 2)) / 6);
    };
    int lo_prev = 0;
    for (int sl = 0; sl < st.nslab; ++sl) {
        const int *hd = st.head + 8 * sl;                           // k0, ld_off, ld_cnt, cp_off, cp_cnt, cp_surf
        const int k0 = hd[0], ld_off = hd[1], ld_cnt = hd[2], cp_off = hd[3], cp_cnt = hd[4], cp_surf = hd[5];
        const int lo = plane_off(k0 - 1);                           // lattice range held in LDS: [lo, PO(k1 + 1))
        double *xs = img - lo;                                      // xs[L] valid inside that range (+ zero guard)
        // the words of the first batch of loads are requested before the window is rearranged; a batch is completed with copies of
        // the list's last entry, so that every load of the phase is unconditional and inside the list
        auto ld_at = [&](int e) { return st.ld_word[ld_off + max(min(e, ld_cnt - 1), 0)]; };
        uint32_t wd0[HB];
#pragma unroll
        for (int q = 0; q < HB; ++q) wd0[q] = ld_at(q * NT + tid);
        if (sl > 0) {
            __syncthreads();                                        // previous slab fully consumed
            // planes k0-1 and k0 move to the front of the window: every thread takes its share into registers, one barrier, then
            // writes (the ranges may overlap; the launcher checks that two planes are at most MV * NT nodes)
            const int cnt = plane_off(k0 + 1) - lo, src = lo - lo_prev;
            double mv[MV];
#pragma unroll
            for (int c = 0; c < MV; ++c) {
                const int q = c * NT + tid;
                mv[c] = q < cnt ? img[src + q] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < MV; ++c) {
                const int q = c * NT + tid;
                if (q < cnt) img[q] = mv[c];
            }
        }
        for (int q = (sl > 0 ? plane_off(k0 + 1) - lo : 0) + tid; q < st.lds_nodes; q += NT) img[q] = 0.0;   // stale data + guard
        __syncthreads();
        // planes new in the window: HBM -> LDS, every slot of w once
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            uint32_t wd[HB];
            double xv[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) wd[q] = q0 == 0 ? wd0[q] : ld_at(q0 + q * NT + tid);
#pragma unroll
            for (int q = 0; q < HB; ++q) xv[q] = wc[wd[q] >> 16];
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (q0 + q * NT + tid < ld_cnt) xs[wd[q] & 0xffffu] = xv[q];
        }
        // evaluated planes, surface entities first: addressing word and slot fetched two iterations ahead of use
        const int ib = cp_off + cp_surf;                            // start of the interior part of the list
        uint32_t p0 = st.cp_word[cp_off + tid], p1 = st.cp_word[cp_off + tid + NT];
        int s0 = (int)st.cp_slot[cp_off + tid], s1 = (int)st.cp_slot[cp_off + tid + NT];
        uint32_t q0 = st.cp_word[ib + tid], q1 = st.cp_word[ib + tid + NT];
        int t0 = (int)st.cp_slot[ib + tid], t1 = (int)st.cp_slot[ib + tid + NT];
        __syncthreads();
        const int nit_s = (cp_surf + NT - 1) / NT;
        for (int it = 0; it < nit_s; ++it) {
            const int e = it * NT + tid;
            const uint32_t pw = p0;
            const int t = s0;
            p0 = p1;
            s0 = s1;
            p1 = st.cp_word[cp_off + e + 2 * NT];
            s1 = (int)st.cp_slot[cp_off + e + 2 * NT];
            // (the lists are padded with valid slots: the loads of an entry behind the list's end are unconditional, their values unused)
            double vs = 0.0, dp[DIM];
            if (!SAME) vs = vc[t];                                  // the other operand at this slot: requested ahead of the taps
#pragma unroll
            for (int a = 0; a < DIM; ++a) dp[a] = lv.dphi[3 * t + a];
            if (e < cp_surf) {
                int L, len, A, B, cls, k;
                decode32w(pw, m, L, len, A, B, cls, k);
                double tap[NDIR], s[NQ];
                window_taps<DIM>(xs, L, len, A, B, true, tap);
                if (SAME) vs = tap[0];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = 0.0;
                const double *cr = cs + cls * (NDIR * NQ);
#pragma unroll
                for (int d = 0; d < NDIR; ++d) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s[q] += lds_ld(cr + d * NQ + q) * tap[d];
                    // (ordered LDS reads and a scheduling fence keep the lane's row from being requested whole ahead of the first product)
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    acc[NQ + a] += dp[a] * vs;
                    if constexpr (!SAME) acc[NQ + DIM + a] += dp[a] * tap[0];
                }
            }
        }
        const int n_int = cp_cnt - cp_surf;
        const int nit_i = (n_int + NT - 1) / NT;
        for (int it = 0; it < nit_i; ++it) {                        // cell interior: one class row for all nodes, dphi is zero
            const int e = it * NT + tid;
            const uint32_t pw = q0;
            const int t = t0;
            q0 = q1;
            t0 = t1;
            q1 = st.cp_word[ib + e + 2 * NT];
            t1 = (int)st.cp_slot[ib + e + 2 * NT];
            double vs = 0.0;
            if (!SAME) vs = vc[t];
            if (e < n_int) {
                int L, len, A, B;
                decode_lattice(pw, m, L, len, A, B);
                double tap[NDIR], s[NQ];
                window_taps<DIM>(xs, L, len, A, B, false, tap);
                if (SAME) vs = tap[0];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = 0.0;
                // (an opaque pointer keeps the backend from hoisting the row's 90 scalar loads out of the loop into vector registers)
                auto *c0 = HMG_KP(double, lv.ctab);
                asm volatile("" : "+s"(c0));
#pragma unroll
                for (int d = 0; d < NDIR; ++d)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s[q] += c0[d * NTERM + q] * tap[d];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
            }
        }
        lo_prev = lo;
    }
    fold_cell<NR, NT>(acc, tid >> 6, red, raw + cell * NR);
}

template <bool SAME>
__global__ void __launch_bounds__(RW_NT)
k_cell_pair_moments_rows(LevelDev lv, const double *v, const double *w, double *__restrict__ raw)
{
    constexpr int DIM = 2, NDIR = 7, NTERM = 4, NQ = NTERM - 1, NR = NQ + (SAME ? 1 : 2) * DIM, NT = RW_NT, HB = 4;
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int m = lv.m, nei = lv.nei, off_int = lv.off_int;
    const int ncw = (lv.ncls * NDIR * NQ + 1) & ~1;
    double *cs = smem;                        // [ncls][NDIR][NQ]: the class table without its mass term
    double *red = cs + ncw;                   // [NT / 64][NR]
    double *img = red + (NT / 64) * NR;       // RW_WIN doubles: [rows j0-1 .. j1 | zero guard]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld, *wc = w + cell * lv.ld;
    for (int q = tid; q < lv.ncls * NDIR * NQ; q += NT) cs[q] = lv.ctab[(size_t)(q / NQ) * NTERM + q % NQ];
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;

    int lo_prev = 0;
    for (int j0 = 0, j1 = 0; j0 <= m; j0 = j1) {
        j1 = rows_band_end(m, j0);
        const int lo = rows_ro(m, j0 - 1);                          // lattice range held in LDS: [lo, hi) + guard
        const int hi = rows_ro(m, j1 + 1);
        double *xs = img - lo;                                      // xs[L] valid inside that range
        int ld_first = 0;                                           // first lattice position that comes from HBM
        if (j0 > 0) {
            __syncthreads();                                        // previous band fully consumed
            // rows j0-1 and j0 move to the front of the window: into registers, one barrier, then written (the ranges may overlap)
            const int cnt = rows_ro(m, j0 + 1) - lo, src = lo - lo_prev;
            double mv[RW_MV];
#pragma unroll
            for (int c = 0; c < RW_MV; ++c) {
                const int q = c * NT + tid;
                mv[c] = q < cnt ? img[src + q] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < RW_MV; ++c) {
                const int q = c * NT + tid;
                if (q < cnt) img[q] = mv[c];
            }
            ld_first = rows_ro(m, j0 + 1);
        }
        for (int q = hi - lo + tid; q < hi - lo + RW_GUARD; q += NT) img[q] = 0.0;   // guard behind the window
        // rows new in the window: HBM -> LDS, every slot of w once; batches of HB slots per thread
        const int ld_cnt = hi - ld_first;
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            int tt[HB];
            double xv[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                // (a batch is completed with copies of the band's last position: every load is unconditional and inside the column)
                const int L = ld_first + min(q0 + q * NT + tid, ld_cnt - 1), j = rows_row_of(m, L), i = L - rows_ro(m, j);
                int cls;
                tt[q] = rows_slot(m, i, j, nei, off_int, cls);
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) xv[q] = wc[tt[q]];
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (q0 + q * NT + tid < ld_cnt) img[ld_first - lo + q0 + q * NT + tid] = xv[q];
        }
        __syncthreads();
        // rows [j0, j1)
        const int e0 = rows_ro(m, j0), ecnt = rows_ro(m, j1) - e0;
        for (int q0 = 0; q0 < ecnt; q0 += NT) {
            const int e = q0 + tid;
            if (e < ecnt) {
                const int L = e0 + e, j = rows_row_of(m, L), i = L - rows_ro(m, j), len = m + 1 - j;
                int cls;
                const int t = rows_slot(m, i, j, nei, off_int, cls);
                double vs = 0.0;
                if (!SAME) vs = vc[t];                              // the other operand at this slot: requested ahead of the taps
                double tap[NDIR], s[NQ];
                window_taps<DIM>(xs, L, len, 0, 0, cls != 0, tap);
                if (SAME) vs = tap[0];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = 0.0;
                if (cls == 0) {                                     // (dphi is zero on the cell interior)
                    // the interior class row by scalar loads (kept in SGPRs across the bands, its 21 terms spilled scalar registers; the
                    // opaque pointer keeps the backend from hoisting the loads out of the loop)
                    auto *c0 = HMG_KP(double, lv.ctab);
                    asm volatile("" : "+s"(c0));
#pragma unroll
                    for (int d = 0; d < NDIR; ++d)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) s[q] += c0[d * NTERM + q] * tap[d];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
                } else {
                    double dp[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) dp[a] = lv.dphi[3 * t + a];
                    const double *cr = cs + cls * (NDIR * NQ);
#pragma unroll
                    for (int d = 0; d < NDIR; ++d)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) s[q] += lds_ld(cr + d * NQ + q) * tap[d];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] += vs * s[q];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        acc[NQ + a] += dp[a] * vs;
                        if constexpr (!SAME) acc[NQ + DIM + a] += dp[a] * tap[0];
                    }
                }
            }
        }
        lo_prev = lo;
    }
    fold_cell<NR, NT>(acc, tid >> 6, red, raw + cell * NR);
}

size_t slab_lds_bytes(const LevelDev &lv, const SlabTables &st)
{
    const size_t ncw = ((size_t)lv.ncls * 15 * 6 + 1) & ~(size_t)1;
    return sizeof(double) * (ncw + (size_t)(SW_NT / 64) * 12 + (size_t)st.lds_nodes);
}

size_t rows_lds_bytes(const LevelDev &lv)
{
    const size_t ncw = ((size_t)lv.ncls * 7 * 3 + 1) & ~(size_t)1;
    return sizeof(double) * (ncw + (size_t)(RW_NT / 64) * 7 + (size_t)RW_WIN);
}

bool slab_ok(const LevelDev &lv, const SlabTables &st)
{
    if (lv.ncls != 15 || lv.ndir != 15 || lv.nterm != 7 || lv.lds_g0 != 0) return false;
    if (!st.head || !st.ld_word || !st.cp_word || !st.cp_slot || st.nslab < 1 || st.lds_nodes <= 0) return false;
    // the packed words (L and the slot in 16 bits each, i, j, k in 7 bits each) hold this level's values; two planes fit the move
    if (lv.m < 1 || lv.m > 127 || lv.nf > 0x10000 || (lv.m + 1) * (lv.m + 1) > SW_MV * SW_NT) return false;
    return slab_lds_bytes(lv, st) <= LDS_PER_CU;
}

bool rows_ok(const LevelDev &lv)
{
    if (lv.ncls != 7 || lv.ndir != 7 || lv.nterm != 4 || lv.ncorner != 3 || lv.nedge != 3 || lv.nface != 0) return false;
    if (lv.m < 2 || lv.m > 1024 || lv.nei != lv.m - 1 || lv.off_int != 3 + 3 * lv.nei || lv.nf != rows_ro(lv.m, lv.m + 1)) return false;
    // the window of the widest band (rows 0..2 at least) plus the guard fits, and so does the move of two rows
    if (rows_ro(lv.m, 3) + RW_GUARD > RW_WIN || 2 * (lv.m + 1) > RW_MV * RW_NT) return false;
    return 2 * rows_lds_bytes(lv) <= LDS_PER_CU;
}

template <class K, class... Args>
void launch_cells(K kern, size_t lds, const Launch &L, int64_t ncells, Args... args)
{
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ncells), dim3(1024), lds, L.stream, args...);
    check_launch();
}

}  // namespace

bool cell_moments_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!lv.ctab || !lv.dphi || lv.nf <= 0 || lv.ld < lv.nf) return false;
    return lv.dim == 3 ? slab_ok(lv, st) : lv.dim == 2 ? rows_ok(lv) : false;
}

void launch_cell_pair_moments_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                     const double *w, double *raw)
{
    if (lv.dim != 2 && lv.dim != 3) throw std::runtime_error("cell moments (window): not a 2D or 3D level");
    if (!cell_moments_window_ok(lv, st))
        throw std::runtime_error(lv.dim == 3 ? "cell moments (slabs): level layout out of range, no slab tables, or a slab does not fit the window"
                                             : "cell moments (row bands): level layout out of range, or a band of rows does not fit the window");
    if (!v || !w) throw std::runtime_error("cell moments (window): null input vector");
    if (!raw) throw std::runtime_error("cell moments (window): null output array");
    if (ncells <= 0) return;
    if (ncells > 0x7fffffffLL) throw std::runtime_error("cell moments (window): too many cells for one launch");
    static_assert(SW_NT == 1024 && RW_NT == 1024, "launch_cells launches 1024 threads");
    const bool same = v == w;
    if (lv.dim == 3) {
        const size_t lds = slab_lds_bytes(lv, st);
        if (same)
            launch_cells(k_cell_pair_moments_slab<true>, lds, L, ncells, lv, v, w, st, raw);
        else
            launch_cells(k_cell_pair_moments_slab<false>, lds, L, ncells, lv, v, w, st, raw);
    } else {
        const size_t lds = rows_lds_bytes(lv);
        if (same)
            launch_cells(k_cell_pair_moments_rows<true>, lds, L, ncells, lv, v, w, raw);
        else
            launch_cells(k_cell_pair_moments_rows<false>, lds, L, ncells, lv, v, w, raw);
    }
}

}  // namespace hmg
