// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell histograms of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the rows of k_cell_histogram (hmg_histogram.hip,
// hmg_histogram.hpp) in the same layout, formed while the cell walks through a ROLLING window of the LDS.  The walk is the one of
// hmg_cell_window.hpp, which every window kernel of the per-cell results shares: k_cell_histogram_slab (3D) fills the window slab
// by slab (slab_window_fill) and takes the nodes from slab_walk_masked, k_cell_histogram_rows (2D) band by band
// (rows_window_fill, rows_walk_masked).  One workgroup of 1024 threads per cell (blockIdx.x is the cell).  Every address is clamped
// into the window and its guard, [lo, whi] of the fill; an element whose bit of elem_mask is clear reads some word of the window
// and is counted nowhere.
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
// 163 840 B), <= 64 VGPRs and no AGPRs.
#include "hmg_histogram.hpp"
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_cell_window.hpp"

namespace hmg {

namespace {

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
    for (int b = threadIdx.x; b < nbins; b += CW_NT) row[b] = hist[b];
}

__global__ void __launch_bounds__(CW_NT)
k_cell_histogram_slab(LevelDev lv, const double *v, SlabTables st, const uint8_t *__restrict__ elem_mask,
                      const double *__restrict__ rows, HistogramRule rule, int *__restrict__ out)
{
    constexpr int DIM = 3, NQ = 6, NROW = NQ + DIM;
    extern __shared__ double smem[];
    const int m = lv.m, nbins = rule.nreg + 3;
    double *img = smem;                                             // st.lds_nodes doubles: [planes k0-1 .. k1 | zero guard]
    int *hist = (int *)(smem + st.lds_nodes);                       // [nbins]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    for (int b = threadIdx.x; b < nbins; b += CW_NT) hist[b] = 0;   // (the first slab's barriers stand before the first add)
    int lo_prev = 0;
    for (int sl = 0; sl < st.nslab; ++sl) {
        const SlabWindow w = slab_window_fill(st, sl, m, img, vc, lo_prev);
        const double *xs = img - w.lo;
        slab_walk_masked(st, w, m, elem_mask, [&](int L, int len, int A, int B, unsigned mk, int) {
            histogram_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, rule, hist);
        });
        lo_prev = w.lo;
    }
    __syncthreads();                                                // the last slab is done: every add has landed
    histogram_flush(hist, nbins, out, cell);
}

__global__ void __launch_bounds__(CW_NT)
k_cell_histogram_rows(LevelDev lv, const double *v, const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                      HistogramRule rule, int *__restrict__ out)
{
    constexpr int DIM = 2, NQ = 3, NROW = NQ + DIM;
    extern __shared__ double smem[];
    const int m = lv.m, nei = lv.nei, off_int = lv.off_int, nbins = rule.nreg + 3;
    double *img = smem;                                             // RW_WIN doubles: [rows j0-1 .. j1 | zero guard]
    int *hist = (int *)(smem + RW_WIN);                             // [nbins]
    const int64_t cell = blockIdx.x;
    const double *vc = v + cell * lv.ld;
    double Q[NQ], X[DIM];
    extrema_row<DIM>(rows + cell * NROW, Q, X);
    for (int b = threadIdx.x; b < nbins; b += CW_NT) hist[b] = 0;   // (the first band's barrier stands before the first add)
    int lo_prev = 0;
    for (int j0 = 0, j1 = 0; j0 <= m; j0 = j1) {
        j1 = rows_band_end(m, j0);
        const RowsWindow w = rows_window_fill(m, nei, off_int, j0, j1, img, vc, lo_prev);
        const double *xs = img - w.lo;
        rows_walk_masked(m, nei, off_int, j0, j1, elem_mask, [&](int L, int len, int A, int B, unsigned mk, int) {
            histogram_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, rule, hist);
        });
        lo_prev = w.lo;
    }
    __syncthreads();                                                // the last band is done: every add has landed
    histogram_flush(hist, nbins, out, cell);
}

constexpr size_t counter_bytes(int nbins) { return sizeof(int) * (((size_t)nbins + 1) & ~(size_t)1); }

size_t slab_lds_bytes(const SlabTables &st, int nbins) { return sizeof(double) * (size_t)st.lds_nodes + counter_bytes(nbins); }

constexpr size_t rows_lds_bytes(int nbins) { return sizeof(double) * (size_t)RW_WIN + counter_bytes(nbins); }

}  // namespace

// the walk's layout checks, and the window fits the LDS together with the largest histogram -- once per CU in 3D, twice in 2D
bool cell_histogram_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!window_layout_ok(lv, st)) return false;
    return lv.dim == 3 ? slab_lds_bytes(st, HIST_MAX_BINS) <= LDS_PER_CU : 2 * rows_lds_bytes(HIST_MAX_BINS) <= LDS_PER_CU;
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
