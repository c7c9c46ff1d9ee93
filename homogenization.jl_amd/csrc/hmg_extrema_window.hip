// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell extrema and exceedance counts of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the results of k_cell_extrema
// (hmg_extrema.hip, hmg_extrema.hpp) in the same row layout, formed while the cell walks through a ROLLING window of the LDS, as
// the per-cell moments of those levels do (hmg_fields_window.hip):
//   k_cell_extrema_slab (3D) follows k_cell_pair_moments_slab<SAME = true> slab for slab: the window holds planes [k0-1, k1], the
//     first ld_word batch is requested before the window is rearranged, planes k0-1 and k0 move to its front through registers with
//     one barrier, the stale tail and the guard are zeroed, the new planes come from HBM through ld_word, the nodes of planes
//     [k0, k1) are taken from cp_word / cp_slot, surface entries first (decode32w), then the cell interior (decode_lattice), both
//     prefetched two trips ahead and every list load unconditional;
//   k_cell_extrema_rows (2D) follows k_cell_pair_moments_rows<true>: bands of lattice rows in closed form (rows_band_end, rows_ro,
//     rows_slot; the row of a lattice position by rows_row_near of hmg_rows_window.hpp, rows_row_of without its loops), two rows moved in registers,
//     no per-level tables.
// One workgroup of 1024 threads per cell.  The window holds v itself.  The element pass reads the centre and the 7 (2D: 3) upper
// taps 11, 8, 4, 5, 13, 10, 1 (2D: 5, 4, 1) of stencil_eval_v: from a node in plane k (row j) they lie in planes k-1 .. k+1 (rows
// j-1 .. j+1), inside the window of the slab (band) that evaluates the node.  Every address is clamped into the window and its
// guard -- 3D [lo, lo + st.lds_nodes - 1], 2D [lo, hi + RW_GUARD - 1] -- so that an element that does not exist reads some word
// of the window, never outside it; elem_mask[slot], requested one trip ahead of its use, keeps that element out of the results.
// The evaluation of a node is extrema_node (hmg_extrema_device.hpp), the one k_cell_extrema calls: maxima, minima and counts do
// not depend on order, so on a level both kernels serve they give the same bits.  Running maximum and minimum, the two NaN
// trackers and the int32 counters (a cell of 3D level 7 has 262 144 elements, one of 2D level 11 has 1 048 576: exact, also as a
// double) stay in registers across slabs / bands and are folded ONCE per cell; no global store before that fold.
// LDS: the window, per-wave partials [16][2] doubles and [16][8] ints; no class table.  3D: window <= 70 KB, one workgroup per CU
// (<= 128 VGPRs); 2D: window 76.8 KB + 768 B, two workgroups per CU (<= 64 VGPRs; no occupancy bound in __launch_bounds__, as the
// rows moment kernel notes; tests/test_cell_extrema_window_kernel_resources.py holds both).
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_rows_window.hpp"

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr int EW_NT = 1024;          // threads per workgroup of both forms
constexpr int EW_NW = EW_NT / 64;
constexpr int EW_MV = 5;             // values per thread of the slab form's window move (two planes of level 7: 4225 nodes)
constexpr int EW_HB = 4;             // loads in flight per thread in the load phases
constexpr int EW_RED = 2 * EW_NW + EW_NW * EX_MAX_THRESHOLDS / 2;   // doubles in front of the window: red [16][2], redc [16][8] ints
constexpr int EW_REDW = EW_NW;       // located forms: doubles more in front of the window, redw [16][2] ints
static_assert(RW_NT == EW_NT, "the row bands are those of a 1024-thread workgroup");

// The bodies of the kernels below.  W = ExtremaWhere is the located form (hmg_cell_extrema_where): the codes slot * 8 + k of the
// elements that hold maximum and minimum stay in two registers across slabs / bands, like the extrema, and are folded with them,
// once per cell; every value is formed and picked as in the other form, which this parameter leaves as it was.
template <class W>
__device__ __forceinline__ void cell_extrema_slab_body(const LevelDev &lv, const double *v, const SlabTables &st,
                                                       const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                                                       const ExtremaThresholds &thr, int nthr, double *__restrict__ out,
                                                       int *__restrict__ codes)
{
    constexpr int DIM = 3, NQ = 6, NROW = NQ + DIM, NT = EW_NT, HB = EW_HB, MV = EW_MV;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lv.m;
    double *red = smem;                       // [NW][2]: maximum, minimum
    int *redc = (int *)(red + 2 * EW_NW);     // [NW][EX_MAX_THRESHOLDS]
    int *redw = (int *)(smem + EW_RED);       // located form: [NW][2] codes
    double *img = smem + EW_RED + (WHERE ? EW_REDW : 0);   // st.lds_nodes doubles: [planes k0-1 .. k1 | zero guard]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    ExtremaAcc acc;
    acc.reset();
    W wh;
    if constexpr (WHERE) wh.reset();
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
        const int whi = lo + st.lds_nodes - 1;                      // last readable lattice position: the end of the guard
        double *xs = img - lo;                                      // xs[L] valid inside [lo, whi]
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
        // planes new in the window: HBM -> LDS, every slot of v once
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            uint32_t wd[HB];
            double xv[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) wd[q] = q0 == 0 ? wd0[q] : ld_at(q0 + q * NT + tid);
#pragma unroll
            for (int q = 0; q < HB; ++q) xv[q] = vc[wd[q] >> 16];
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (q0 + q * NT + tid < ld_cnt) xs[wd[q] & 0xffffu] = xv[q];
        }
        // evaluated planes, surface entities first: addressing word and slot fetched two trips ahead of use, the slot's mask one
        // (the lists are padded with valid slots: the loads of an entry behind the list's end are unconditional, their values unused)
        const int ib = cp_off + cp_surf;                            // start of the interior part of the list
        uint32_t p0 = st.cp_word[cp_off + tid], p1 = st.cp_word[cp_off + tid + NT];
        int s0 = (int)st.cp_slot[cp_off + tid], s1 = (int)st.cp_slot[cp_off + tid + NT];
        uint32_t q0 = st.cp_word[ib + tid], q1 = st.cp_word[ib + tid + NT];
        int t0 = (int)st.cp_slot[ib + tid], t1 = (int)st.cp_slot[ib + tid + NT];
        unsigned ms = elem_mask[s0], mi = elem_mask[t0];
        __syncthreads();
        const int nit_s = (cp_surf + NT - 1) / NT;
        for (int it = 0; it < nit_s; ++it) {
            const int e = it * NT + tid;
            const uint32_t pw = p0;
            const unsigned mk = ms;
            const int slot = s0;
            p0 = p1;
            s0 = s1;
            ms = elem_mask[s0];
            p1 = st.cp_word[cp_off + e + 2 * NT];
            s1 = (int)st.cp_slot[cp_off + e + 2 * NT];
            if (e < cp_surf && mk != 0) {                           // (mk == 0: no element has its lowest vertex here)
                int L, len, A, B, cls, k;
                decode32w(pw, m, L, len, A, B, cls, k);
                if constexpr (WHERE)
                    extrema_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, thr, nthr, acc, slot, &wh);
                else
                    extrema_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, thr, nthr, acc);
            }
        }
        const int n_int = cp_cnt - cp_surf;
        const int nit_i = (n_int + NT - 1) / NT;
        for (int it = 0; it < nit_i; ++it) {                        // cell interior
            const int e = it * NT + tid;
            const uint32_t pw = q0;
            const unsigned mk = mi;
            const int slot = t0;
            q0 = q1;
            t0 = t1;
            mi = elem_mask[t0];
            q1 = st.cp_word[ib + e + 2 * NT];
            t1 = (int)st.cp_slot[ib + e + 2 * NT];
            if (e < n_int && mk != 0) {
                int L, len, A, B;
                decode_lattice(pw, m, L, len, A, B);
                if constexpr (WHERE)
                    extrema_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, thr, nthr, acc, slot, &wh);
                else
                    extrema_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, thr, nthr, acc);
            }
        }
        lo_prev = lo;
    }
    if constexpr (WHERE)
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell, &wh, redw, codes);
    else
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell);
}

__global__ void __launch_bounds__(EW_NT)
k_cell_extrema_slab(LevelDev lv, const double *v, SlabTables st, const uint8_t *__restrict__ elem_mask,
                    const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    cell_extrema_slab_body<ExtremaNoWhere>(lv, v, st, elem_mask, rows, thr, nthr, out, nullptr);
}

// the located form of k_cell_extrema_slab
__global__ void __launch_bounds__(EW_NT)
k_extrema_where_slab(LevelDev lv, const double *v, SlabTables st, const uint8_t *__restrict__ elem_mask,
                     const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out,
                     int *__restrict__ codes)
{
    cell_extrema_slab_body<ExtremaWhere>(lv, v, st, elem_mask, rows, thr, nthr, out, codes);
}

template <class W>
__device__ __forceinline__ void cell_extrema_rows_body(const LevelDev &lv, const double *v, const uint8_t *__restrict__ elem_mask,
                                                       const double *__restrict__ rows, const ExtremaThresholds &thr, int nthr,
                                                       double *__restrict__ out, int *__restrict__ codes)
{
    constexpr int DIM = 2, NQ = 3, NROW = NQ + DIM, NT = EW_NT, HB = EW_HB;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lv.m, nei = lv.nei, off_int = lv.off_int;
    double *red = smem;                       // [NW][2]: maximum, minimum
    int *redc = (int *)(red + 2 * EW_NW);     // [NW][EX_MAX_THRESHOLDS]
    int *redw = (int *)(smem + EW_RED);       // located form: [NW][2] codes
    double *img = smem + EW_RED + (WHERE ? EW_REDW : 0);   // RW_WIN doubles: [rows j0-1 .. j1 | zero guard]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    ExtremaAcc acc;
    acc.reset();
    W wh;
    if constexpr (WHERE) wh.reset();

    int lo_prev = 0;
    for (int j0 = 0, j1 = 0; j0 <= m; j0 = j1) {
        j1 = rows_band_end(m, j0);
        const int lo = rows_ro(m, j0 - 1);                          // lattice range held in LDS: [lo, hi) + guard
        const int hi = rows_ro(m, j1 + 1);
        const int whi = hi + RW_GUARD - 1;                          // last readable lattice position: the end of the guard
        double *xs = img - lo;                                      // xs[L] valid inside [lo, whi]
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
        // rows new in the window: HBM -> LDS, every slot of v once; batches of HB slots per thread
        const int ld_cnt = hi - ld_first;
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            int tt[HB];
            double xv[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                // (a batch is completed with copies of the band's last position: every load is unconditional and inside the column)
                const int L = ld_first + min(q0 + q * NT + tid, ld_cnt - 1);
                tt[q] = rows_slot_at(m, L, rows_row_near(m, L), nei, off_int);
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) xv[q] = vc[tt[q]];
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (q0 + q * NT + tid < ld_cnt) img[ld_first - lo + q0 + q * NT + tid] = xv[q];
        }
        // rows [j0, j1): the node's row and its mask are formed one trip ahead of use (a trip behind the band's end repeats its last
        // node: every mask load is unconditional and inside the level's mask)
        const int e0 = rows_ro(m, j0), ecnt = rows_ro(m, j1) - e0;
        auto node_at = [&](int e, int &L, int &j, unsigned &mk, int &slot) {
            L = e0 + min(e, ecnt - 1);
            j = rows_row_near(m, L);
            slot = rows_slot_at(m, L, j, nei, off_int);
            mk = elem_mask[slot];
        };
        int Ln, jn, sn;                                             // (sn: the located form alone reads it)
        unsigned mkn;
        node_at(tid, Ln, jn, mkn, sn);
        __syncthreads();
        for (int q0 = 0; q0 < ecnt; q0 += NT) {
            const int e = q0 + tid, L = Ln, j = jn;
            const unsigned mk = mkn;
            const int slot = sn;
            node_at(e + NT, Ln, jn, mkn, sn);
            if (e < ecnt && mk != 0) {
                if constexpr (WHERE)
                    extrema_node<DIM>(xs, L, m + 1 - j, 0, 0, lo, whi, mk, Q, X, thr, nthr, acc, slot, &wh);
                else
                    extrema_node<DIM>(xs, L, m + 1 - j, 0, 0, lo, whi, mk, Q, X, thr, nthr, acc);
            }
        }
        lo_prev = lo;
    }
    if constexpr (WHERE)
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell, &wh, redw, codes);
    else
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell);
}

__global__ void __launch_bounds__(EW_NT)
k_cell_extrema_rows(LevelDev lv, const double *v, const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                    ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    cell_extrema_rows_body<ExtremaNoWhere>(lv, v, elem_mask, rows, thr, nthr, out, nullptr);
}

// the located form of k_cell_extrema_rows
__global__ void __launch_bounds__(EW_NT)
k_extrema_where_rows(LevelDev lv, const double *v, const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                     ExtremaThresholds thr, int nthr, double *__restrict__ out, int *__restrict__ codes)
{
    cell_extrema_rows_body<ExtremaWhere>(lv, v, elem_mask, rows, thr, nthr, out, codes);
}

size_t slab_lds_bytes(const SlabTables &st, bool where = false)
{
    return sizeof(double) * ((size_t)EW_RED + (where ? EW_REDW : 0) + (size_t)st.lds_nodes);
}

constexpr size_t rows_lds_bytes(bool where = false) { return sizeof(double) * ((size_t)EW_RED + (where ? EW_REDW : 0) + (size_t)RW_WIN); }

// the layout and packed-word ranges k_cell_extrema_slab relies on (those of the slab moment kernel, without its class table)
bool slab_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!st.head || !st.ld_word || !st.cp_word || !st.cp_slot || st.nslab < 1 || st.lds_nodes <= 0) return false;
    // the packed words (L and the slot in 16 bits each, i, j, k in 7 bits each) hold this level's values; two planes fit the move
    if (lv.m < 1 || lv.m > 127 || lv.nf > 0x10000 || (lv.m + 1) * (lv.m + 1) > EW_MV * EW_NT) return false;
    return slab_lds_bytes(st, true) <= LDS_PER_CU;          // (either form: both serve the same levels)
}

// ... and k_cell_extrema_rows (those of the row-band moment kernel: the storage order rows_slot assumes, the window of the widest band)
bool rows_ok(const LevelDev &lv)
{
    if (lv.ncorner != 3 || lv.nedge != 3 || lv.nface != 0) return false;
    if (lv.m < 2 || lv.m > 1024 || lv.nei != lv.m - 1 || lv.off_int != 3 + 3 * lv.nei || lv.nf != rows_ro(lv.m, lv.m + 1)) return false;
    if (rows_ro(lv.m, 3) + RW_GUARD > RW_WIN || 2 * (lv.m + 1) > RW_MV * RW_NT) return false;
    return 2 * rows_lds_bytes(true) <= LDS_PER_CU;          // (either form)
}

template <class K, class... Args>
void launch_cells(K kern, size_t lds, const Launch &L, int64_t ncells, Args... args)
{
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ncells), dim3(EW_NT), lds, L.stream, args...);
    check_launch();
}

}  // namespace

bool cell_extrema_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (lv.nf <= 0 || lv.ld < lv.nf) return false;
    return lv.dim == 3 ? slab_ok(lv, st) : lv.dim == 2 ? rows_ok(lv) : false;
}

void launch_cell_extrema_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                const uint8_t *elem_mask, const double *rows, const ExtremaThresholds &thr, int nthr, double *out,
                                int *codes)
{
    if (lv.dim != 2 && lv.dim != 3) throw std::runtime_error("cell extrema (window): not a 2D or 3D level");
    if (!cell_extrema_window_ok(lv, st))
        throw std::runtime_error(lv.dim == 3 ? "cell extrema (slabs): level layout out of range, no slab tables, or a slab does not fit the window"
                                             : "cell extrema (row bands): level layout out of range, or a band of rows does not fit the window");
    if (nthr < 0 || nthr > EX_MAX_THRESHOLDS) throw std::runtime_error("cell extrema (window): 0 to 8 thresholds");
    if (!v || !elem_mask || !rows || !out) throw std::runtime_error("cell extrema (window): null device pointer");
    if (ncells <= 0) return;
    if (ncells > 0x7fffffffLL) throw std::runtime_error("cell extrema (window): too many cells for one launch");
    if (lv.dim == 3 && codes)
        launch_cells(k_extrema_where_slab, slab_lds_bytes(st, true), L, ncells, lv, v, st, elem_mask, rows, thr, nthr, out, codes);
    else if (lv.dim == 3)
        launch_cells(k_cell_extrema_slab, slab_lds_bytes(st), L, ncells, lv, v, st, elem_mask, rows, thr, nthr, out);
    else if (codes)
        launch_cells(k_extrema_where_rows, rows_lds_bytes(true), L, ncells, lv, v, elem_mask, rows, thr, nthr, out, codes);
    else
        launch_cells(k_cell_extrema_rows, rows_lds_bytes(), L, ncells, lv, v, elem_mask, rows, thr, nthr, out);
}

}  // namespace hmg
