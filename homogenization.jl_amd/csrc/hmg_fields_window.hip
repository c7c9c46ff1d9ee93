// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell pair moments of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the raw sums of k_cell_pair_moments
// (hmg_fields.hip, hmg_fields.hpp) in the same row layout,
//   raw[c][t]            = sum_i v_i (T_t w_c)_i,   raw[c][nq + a] = sum_i dphi[3 i + a] v_i,   raw[c][nq + dim + a] = sum_i dphi[3 i + a] w_i
// (the last set only where w is another vector), formed while the cell walks through a ROLLING window of the LDS, as the operator
// applies of those levels do (k_apply_slab of hmg_apply.hip, k_apply_rows of hmg_apply_rows.hip).  The window is filled by the
// walk that every window kernel of the per-cell results shares (hmg_cell_window.hpp): slab_window_fill in
// k_cell_pair_moments_slab (3D), rows_window_fill in k_cell_pair_moments_rows (2D).  The evaluation loops are this file's own:
// they read no mask, request vc[t] and dphi ahead of the branch, and take the interior class row through an opaque pointer.
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
// window 76.8 KB + table and sums 2 KB, at most 60 VGPRs: two workgroups per CU, as k_apply_rows
// (tests/test_cell_moments_kernel_resources.py holds the 64).
#include "hmg_fields.hpp"
#include "hmg_fields_device.hpp"
#include "hmg_cell_window.hpp"

namespace hmg {

namespace {

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
__global__ void __launch_bounds__(CW_NT)
k_cell_pair_moments_slab(LevelDev lv, const double *v, const double *w, SlabTables st, double *__restrict__ raw)
{
    constexpr int DIM = 3, NDIR = 15, NTERM = 7, NQ = NTERM - 1, NR = NQ + (SAME ? 1 : 2) * DIM, NT = CW_NT;
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
    int lo_prev = 0;
    for (int sl = 0; sl < st.nslab; ++sl) {
        const SlabWindow sw = slab_window_fill(st, sl, m, img, wc, lo_prev);   // (only w goes into the window)
        const int lo = sw.lo, cp_off = sw.cp_off, cp_cnt = sw.cp_cnt, cp_surf = sw.cp_surf;
        const double *xs = img - lo;                                // xs[L] valid inside the window (+ zero guard)
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
__global__ void __launch_bounds__(CW_NT)
k_cell_pair_moments_rows(LevelDev lv, const double *v, const double *w, double *__restrict__ raw)
{
    constexpr int DIM = 2, NDIR = 7, NTERM = 4, NQ = NTERM - 1, NR = NQ + (SAME ? 1 : 2) * DIM, NT = CW_NT;
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
        const int lo = rows_window_fill(m, nei, off_int, j0, j1, img, wc, lo_prev).lo;   // (only w goes into the window)
        const double *xs = img - lo;                                // xs[L] valid inside the window (+ zero guard)
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
    return sizeof(double) * (ncw + (size_t)(CW_NT / 64) * 12 + (size_t)st.lds_nodes);
}

size_t rows_lds_bytes(const LevelDev &lv)
{
    const size_t ncw = ((size_t)lv.ncls * 7 * 3 + 1) & ~(size_t)1;
    return sizeof(double) * (ncw + (size_t)(CW_NT / 64) * 7 + (size_t)RW_WIN);
}

}  // namespace

// the walk's layout checks, the shape of the class table, and the window fits the LDS next to the table and the partial sums --
// once per CU in 3D, twice in 2D
bool cell_moments_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!lv.ctab || !lv.dphi || !window_layout_ok(lv, st)) return false;
    if (lv.dim == 3)
        return lv.ncls == 15 && lv.ndir == 15 && lv.nterm == 7 && lv.lds_g0 == 0 && slab_lds_bytes(lv, st) <= LDS_PER_CU;
    return lv.ncls == 7 && lv.ndir == 7 && lv.nterm == 4 && 2 * rows_lds_bytes(lv) <= LDS_PER_CU;
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
