// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell histograms of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the rows of k_cell_histogram (hmg_histogram.hip,
// hmg_histogram.hpp) in the same layout, formed while the cell walks through a ROLLING window of the LDS.  The walk is that of the
// extrema window kernels (hmg_extrema_window.hip), slab for slab and band for band:
//   k_cell_histogram_slab (3D) follows cell_extrema_slab_body: the window holds planes [k0-1, k1], the first ld_word batch is
//     requested before the window is rearranged, planes k0-1 and k0 move to its front through registers with one barrier, the stale
//     tail and the guard are zeroed, the new planes come from HBM through ld_word with unconditional loads, the nodes of planes
//     [k0, k1) are taken from cp_word / cp_slot, surface entries first (decode32w), then the cell interior (decode_lattice), both
//     prefetched two trips ahead, elem_mask one trip ahead.  The tables are the level's SlabTables (slab_tables(g, lv)).
//   k_cell_histogram_rows (2D) follows cell_extrema_rows_body: bands of lattice rows in closed form (rows_band_end, rows_ro,
//     rows_row_near, rows_slot_at of hmg_rows_window.hpp), two rows moved in registers, no per-level tables.
// One workgroup of 1024 threads per cell (blockIdx.x is the cell).  Every address is clamped into the window and its guard -- 3D
// [lo, lo + st.lds_nodes - 1], 2D [lo, hi + RW_GUARD - 1] -- as in the extrema window kernels; an element whose bit of elem_mask
// is clear reads some word of the window and is counted nowhere.
// The node: extrema_values (hmg_extrema_device.hpp), the function k_cell_histogram calls -- the value bits of hmg_cell_extrema
// and of the LDS histogram kernel --, then histogram_node_bins and histogram_node_add (hmg_histogram_device.hpp), the text of
// k_cell_histogram's HIST_NODE form: the node's elements are combined in registers and one workgroup-scope LDS integer add is
// issued per distinct bin.  HIST_NODE is the only form here: the option "cell_histogram_variant" has no say in these kernels (the
// counts are the same ints from every variant anyway).
// LDS: [window | nbins int32 counters], sized for the call's nbins.  The counters are zeroed before the first slab / band and
// flushed ONCE, behind the barrier that ends the last one, as one coalesced row out[cell * nbins ..].  No global atomics and no
// floating-point sums: the same ints in every run.
// Budgets (tests/test_cell_histogram_window_kernel_resources.py holds them): 3D window <= 70 KB + at most 4 112 B of counters, one
// workgroup per CU, <= 128 vector registers; 2D 9600 * 8 + 4 112 = 80 912 B at 1 027 bins, two workgroups per CU (161 824 B of
// 163 840 B), <= 64 VGPRs and no AGPRs (no occupancy bound in __launch_bounds__, as the rows moment kernel notes).
#include "hmg_histogram.hpp"
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_rows_window.hpp"

namespace hmg {

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr int HW_NT = 1024;          // threads per workgroup of both forms
constexpr int HW_MV = 5;             // values per thread of the slab form's window move (two planes of level 7: 4225 nodes)
constexpr int HW_HB = 4;             // loads in flight per thread in the load phases
static_assert(RW_NT == HW_NT, "the row bands are those of a 1024-thread workgroup");

// the values of one node, binned, combined and added to the workgroup's histogram
template <int DIM>
__device__ __forceinline__ void histogram_node(const double *xs, int L, int len, int A, int B, int lo, int whi, unsigned mk,
                                               const double *Q, const double *X, const HistogramRule &rule, int *hist)
{
    constexpr int NEL = DIM == 3 ? 6 : 2;
    double q[NEL];
    extrema_values<DIM>(xs, L, len, A, B, lo, whi, Q, X, q);
    int bin[NEL], cnt[NEL];
    histogram_node_bins<NEL>(q, mk, rule, bin, cnt);
    histogram_node_add<NEL>(hist, bin, cnt);
}

// counters -> out[cell * nbins ..], one coalesced row; the caller's barrier says that every wave is done adding
__device__ __forceinline__ void histogram_flush(const int *hist, int nbins, int *__restrict__ out, int64_t cell)
{
    int *row = out + cell * nbins;
    for (int b = threadIdx.x; b < nbins; b += HW_NT) row[b] = hist[b];
}

__global__ void __launch_bounds__(HW_NT)
k_cell_histogram_slab(LevelDev lv, const double *v, SlabTables st, const uint8_t *__restrict__ elem_mask,
                      const double *__restrict__ rows, HistogramRule rule, int *__restrict__ out)
{
    constexpr int DIM = 3, NQ = 6, NROW = NQ + DIM, NT = HW_NT, HB = HW_HB, MV = HW_MV;
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int m = lv.m, nbins = rule.nreg + 3;
    double *img = smem;                                             // st.lds_nodes doubles: [planes k0-1 .. k1 | zero guard]
    int *hist = (int *)(smem + st.lds_nodes);                       // [nbins]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    for (int b = tid; b < nbins; b += NT) hist[b] = 0;              // (the first slab's barriers stand before the first add)
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
            p0 = p1;
            s0 = s1;
            ms = elem_mask[s0];
            p1 = st.cp_word[cp_off + e + 2 * NT];
            s1 = (int)st.cp_slot[cp_off + e + 2 * NT];
            if (e < cp_surf && mk != 0) {                           // (mk == 0: no element has its lowest vertex here)
                int L, len, A, B, cls, k;
                decode32w(pw, m, L, len, A, B, cls, k);
                histogram_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, rule, hist);
            }
        }
        const int n_int = cp_cnt - cp_surf;
        const int nit_i = (n_int + NT - 1) / NT;
        for (int it = 0; it < nit_i; ++it) {                        // cell interior
            const int e = it * NT + tid;
            const uint32_t pw = q0;
            const unsigned mk = mi;
            q0 = q1;
            t0 = t1;
            mi = elem_mask[t0];
            q1 = st.cp_word[ib + e + 2 * NT];
            t1 = (int)st.cp_slot[ib + e + 2 * NT];
            if (e < n_int && mk != 0) {
                int L, len, A, B;
                decode_lattice(pw, m, L, len, A, B);
                histogram_node<DIM>(xs, L, len, A, B, lo, whi, mk, Q, X, rule, hist);
            }
        }
        lo_prev = lo;
    }
    __syncthreads();                                                // the last slab is done: every add has landed
    histogram_flush(hist, nbins, out, cell);
}

__global__ void __launch_bounds__(HW_NT)
k_cell_histogram_rows(LevelDev lv, const double *v, const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                      HistogramRule rule, int *__restrict__ out)
{
    constexpr int DIM = 2, NQ = 3, NROW = NQ + DIM, NT = HW_NT, HB = HW_HB;
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int m = lv.m, nei = lv.nei, off_int = lv.off_int, nbins = rule.nreg + 3;
    double *img = smem;                                             // RW_WIN doubles: [rows j0-1 .. j1 | zero guard]
    int *hist = (int *)(smem + RW_WIN);                             // [nbins]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    for (int b = tid; b < nbins; b += NT) hist[b] = 0;              // (the first band's barrier stands before the first add)

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
        auto node_at = [&](int e, int &L, int &j, unsigned &mk) {
            L = e0 + min(e, ecnt - 1);
            j = rows_row_near(m, L);
            mk = elem_mask[rows_slot_at(m, L, j, nei, off_int)];
        };
        int Ln, jn;
        unsigned mkn;
        node_at(tid, Ln, jn, mkn);
        __syncthreads();
        for (int q0 = 0; q0 < ecnt; q0 += NT) {
            const int e = q0 + tid, L = Ln, j = jn;
            const unsigned mk = mkn;
            node_at(e + NT, Ln, jn, mkn);
            if (e < ecnt && mk != 0) histogram_node<DIM>(xs, L, m + 1 - j, 0, 0, lo, whi, mk, Q, X, rule, hist);
        }
        lo_prev = lo;
    }
    __syncthreads();                                                // the last band is done: every add has landed
    histogram_flush(hist, nbins, out, cell);
}

constexpr size_t counter_bytes(int nbins) { return sizeof(int) * (((size_t)nbins + 1) & ~(size_t)1); }

size_t slab_lds_bytes(const SlabTables &st, int nbins) { return sizeof(double) * (size_t)st.lds_nodes + counter_bytes(nbins); }

constexpr size_t rows_lds_bytes(int nbins) { return sizeof(double) * (size_t)RW_WIN + counter_bytes(nbins); }

template <class K, class... Args>
void launch_cells(K kern, size_t lds, const Launch &L, int64_t ncells, Args... args)
{
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ncells), dim3(HW_NT), lds, L.stream, args...);
    check_launch();
}

}  // namespace

// The layout checks are cell_extrema_window_ok's (the walks are the same ones: the storage order rows_slot assumes, the packed-word
// ranges, the slab tables); what this file's own constants add: two planes fit the slab form's move, and the window fits the LDS
// together with the largest histogram -- once per CU in 3D, twice in 2D.
bool cell_histogram_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!cell_extrema_window_ok(lv, st)) return false;
    if (lv.dim == 3) return (lv.m + 1) * (lv.m + 1) <= HW_MV * HW_NT && slab_lds_bytes(st, HIST_MAX_BINS) <= LDS_PER_CU;
    return 2 * (lv.m + 1) <= RW_MV * HW_NT && 2 * rows_lds_bytes(HIST_MAX_BINS) <= LDS_PER_CU;
}

void launch_cell_histogram_window(const Launch &L, const LevelDev &lv, const SlabTables &st, int64_t ncells, const double *v,
                                  const uint8_t *elem_mask, const double *rows, const HistogramRule &rule, int *out)
{
    if (lv.dim != 2 && lv.dim != 3) throw std::runtime_error("cell histogram (window): not a 2D or 3D level");
    if (!cell_histogram_window_ok(lv, st))
        throw std::runtime_error(lv.dim == 3 ? "cell histogram (slabs): level layout out of range, no slab tables, or a slab does not fit the window next to the histogram"
                                             : "cell histogram (row bands): level layout out of range, or a band of rows does not fit the window next to the histogram");
    if (rule.nreg < 1 || rule.nreg > HIST_MAX_REGULAR || rule.shift < 20 - HIST_MAX_SUB_BITS || rule.shift > 20 || rule.key0 < 0)
        throw std::runtime_error("cell histogram (window): bin parameters outside the rule");
    if (!v || !elem_mask || !rows || !out) throw std::runtime_error("cell histogram (window): null device pointer");
    if (ncells <= 0) return;
    if (ncells > 0x7fffffffLL) throw std::runtime_error("cell histogram (window): too many cells for one launch");
    const int nbins = rule.nreg + 3;
    if (lv.dim == 3)
        launch_cells(k_cell_histogram_slab, slab_lds_bytes(st, nbins), L, ncells, lv, v, st, elem_mask, rows, rule, out);
    else
        launch_cells(k_cell_histogram_rows, rows_lds_bytes(nbins), L, ncells, lv, v, elem_mask, rows, rule, out);
}

}  // namespace hmg
