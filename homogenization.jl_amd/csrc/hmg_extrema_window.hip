// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// Per-cell extrema and exceedance counts of cells LARGER than the LDS (3D level 7, 2D levels 9..11): the results of k_cell_extrema
// (hmg_extrema.hip, hmg_extrema.hpp) in the same row layout, formed while the cell walks through a ROLLING window of the LDS.  The
// walk is the one of hmg_cell_window.hpp, which every window kernel of the per-cell results shares: k_cell_extrema_slab (3D) fills
// the window slab by slab (slab_window_fill) and takes the nodes from slab_walk_masked, k_cell_extrema_rows (2D) band by band
// (rows_window_fill, rows_walk_masked).
// One workgroup of 1024 threads per cell.  The window holds v itself.  The element pass reads the centre and the 7 (2D: 3) upper
// taps 11, 8, 4, 5, 13, 10, 1 (2D: 5, 4, 1) of stencil_eval_v: from a node in plane k (row j) they lie in planes k-1 .. k+1 (rows
// j-1 .. j+1), inside the window of the slab (band) that evaluates the node.  Every address is clamped into the window and its
// guard, [lo, whi] of the fill, so that an element that does not exist reads some word of the window, never outside it;
// elem_mask[slot], requested one trip ahead of its use, keeps that element out of the results.
// The evaluation of a node is extrema_node (hmg_extrema_device.hpp), the one k_cell_extrema calls: maxima, minima and counts do
// not depend on order, so on a level both kernels serve they give the same bits.  Running maximum and minimum, the two NaN
// trackers and the int32 counters (a cell of 3D level 7 has 262 144 elements, one of 2D level 11 has 1 048 576: exact, also as a
// double) stay in registers across slabs / bands and are folded ONCE per cell; no global store before that fold.
// LDS: the window, per-wave partials [16][2] doubles and [16][8] ints; no class table.  3D: window <= 70 KB, one workgroup per CU
// (<= 128 VGPRs); 2D: window 76.8 KB + 768 B, two workgroups per CU (<= 64 VGPRs;
// tests/test_cell_extrema_window_kernel_resources.py holds both).
#include "hmg_extrema.hpp"
#include "hmg_extrema_device.hpp"
#include "hmg_cell_window.hpp"

namespace hmg {

namespace {

constexpr int EW_NW = CW_NT / 64;
constexpr int EW_RED = 2 * EW_NW + EW_NW * EX_MAX_THRESHOLDS / 2;   // doubles in front of the window: red [16][2], redc [16][8] ints
constexpr int EW_REDW = EW_NW;       // located forms: doubles more in front of the window, redw [16][2] ints

// The bodies of the kernels below.  W = ExtremaWhere is the located form (hmg_cell_extrema_where): the codes slot * 8 + k of the
// elements that hold maximum and minimum stay in two registers across slabs / bands, like the extrema, and are folded with them,
// once per cell; every value is formed and picked as in the other form, which this parameter leaves as it was.
template <class W>
__device__ __forceinline__ void cell_extrema_slab_body(const LevelDev &lv, const double *v, const SlabTables &st,
                                                       const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                                                       const ExtremaThresholds &thr, int nthr, double *__restrict__ out,
                                                       int *__restrict__ codes)
{
    constexpr int DIM = 3, NQ = 6, NROW = NQ + DIM;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    extern __shared__ double smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
    int lo_prev = 0;
    for (int sl = 0; sl < st.nslab; ++sl) {
        const SlabWindow w = slab_window_fill(st, sl, m, img, vc, lo_prev);
        const double *xs = img - w.lo;
        slab_walk_masked(st, w, m, elem_mask, [&](int L, int len, int A, int B, unsigned mk, int slot) {
            if constexpr (WHERE)
                extrema_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, thr, nthr, acc, slot, &wh);
            else
                extrema_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, thr, nthr, acc);
        });
        lo_prev = w.lo;
    }
    if constexpr (WHERE)
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell, &wh, redw, codes);
    else
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell);
}

__global__ void __launch_bounds__(CW_NT)
k_cell_extrema_slab(LevelDev lv, const double *v, SlabTables st, const uint8_t *__restrict__ elem_mask,
                    const double *__restrict__ rows, ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    cell_extrema_slab_body<ExtremaNoWhere>(lv, v, st, elem_mask, rows, thr, nthr, out, nullptr);
}

// the located form of k_cell_extrema_slab
__global__ void __launch_bounds__(CW_NT)
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
    constexpr int DIM = 2, NQ = 3, NROW = NQ + DIM;
    constexpr bool WHERE = std::is_same<W, ExtremaWhere>::value;
    extern __shared__ double smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
        const RowsWindow w = rows_window_fill(m, nei, off_int, j0, j1, img, vc, lo_prev);
        const double *xs = img - w.lo;
        rows_walk_masked(m, nei, off_int, j0, j1, elem_mask, [&](int L, int len, int A, int B, unsigned mk, int slot) {
            if constexpr (WHERE)
                extrema_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, thr, nthr, acc, slot, &wh);
            else
                extrema_node<DIM>(xs, L, len, A, B, w.lo, w.whi, mk, Q, X, thr, nthr, acc);
        });
        lo_prev = w.lo;
    }
    if constexpr (WHERE)
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell, &wh, redw, codes);
    else
        extrema_fold<EW_NW>(acc, nthr, wave, red, redc, out, cell);
}

__global__ void __launch_bounds__(CW_NT)
k_cell_extrema_rows(LevelDev lv, const double *v, const uint8_t *__restrict__ elem_mask, const double *__restrict__ rows,
                    ExtremaThresholds thr, int nthr, double *__restrict__ out)
{
    cell_extrema_rows_body<ExtremaNoWhere>(lv, v, elem_mask, rows, thr, nthr, out, nullptr);
}

// the located form of k_cell_extrema_rows
__global__ void __launch_bounds__(CW_NT)
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

}  // namespace

// the walk's layout checks, and the window fits the LDS next to the partials of either form (both serve the same levels) -- once
// per CU in 3D, twice in 2D
bool cell_extrema_window_ok(const LevelDev &lv, const SlabTables &st)
{
    if (!window_layout_ok(lv, st)) return false;
    return lv.dim == 3 ? slab_lds_bytes(st, true) <= LDS_PER_CU : 2 * rows_lds_bytes(true) <= LDS_PER_CU;
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
