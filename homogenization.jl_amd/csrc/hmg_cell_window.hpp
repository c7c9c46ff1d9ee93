// The walk of one cell LARGER than the LDS (3D level 7, 2D levels 9..11) through a ROLLING window of the LDS: what the window
// kernels of the per-cell moments (hmg_fields_window.hip), extrema (hmg_extrema_window.hip) and histograms
// (hmg_histogram_window.hip) share.  One workgroup of CW_NT threads per cell; the window holds one column of the cell.
//   3D, slabs of k-planes from the level's SlabTables (slab_tables(g, lv)): the window holds planes [k0-1, k1] and a zero guard,
//     the nodes of planes [k0, k1) are evaluated from cp_word / cp_slot, surface entries first (decode32w), then the cell
//     interior (decode_lattice).
//   2D, bands of lattice rows in closed form (rows_band_end, rows_ro, rows_row_near, rows_slot_at of hmg_rows_window.hpp, no
//     per-level tables): the window holds rows [j0-1, j1] and a zero guard, the nodes of rows [j0, j1) are evaluated.
// A fill brings the window to its slab / band: the planes / rows the previous one shares with it move to the front through
// registers, what lies behind them is zeroed, the new ones come from HBM.  A fill ends with its last store: the caller issues
// what it wants in flight across the barrier, then the barrier, then evaluates -- or calls a masked walk, which does those
// three for a kernel that takes elem_mask[slot] per node and hands every node that has elements to its callable.
// The 2D kernels run two workgroups per CU on <= 64 VGPRs without an occupancy bound in __launch_bounds__: the bound caps the
// scalar registers at 80, and the rows moment kernel spilled them.
#pragma once

#include "hmg_rows_window.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr int CW_NT = 1024;          // threads per workgroup of both forms
constexpr int CW_HB = 4;             // loads in flight per thread in the load phases
constexpr int CW_MV = 5;             // values per thread of the slab form's window move (two planes of level 7: 4225 nodes)
static_assert(RW_NT == CW_NT, "the row bands are those of a 1024-thread workgroup");

__device__ __forceinline__ int plane_off(int m, int k)   // PO(k) = number of lattice nodes in planes < k
{
    if (k <= 0) return 0;
    if (k > m + 1) k = m + 1;
    const long long n1 = m + 1, n2 = m + 1 - k;
    return (int)((n1 * (n1 + 1) * (n1 + 2) - n2 * (n2 + 1) * (n2 + 2)) / 6);
}

// img[src .. src + cnt) moves to the front of the window: every thread takes its share into registers, one barrier, then writes
// (the ranges may overlap; window_layout_ok checks that cnt is at most MV * CW_NT)
template <int MV>
__device__ __forceinline__ void window_move(double *img, int src, int cnt)
{
    const int tid = threadIdx.x;
    double mv[MV];
#pragma unroll
    for (int c = 0; c < MV; ++c) {
        const int q = c * CW_NT + tid;
        mv[c] = q < cnt ? img[src + q] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MV; ++c) {
        const int q = c * CW_NT + tid;
        if (q < cnt) img[q] = mv[c];
    }
}

struct SlabWindow {
    int lo, whi;                     // lattice range readable in the window: xs = img - lo, xs[L] valid inside [lo, whi]
    int cp_off, cp_cnt, cp_surf;     // the slab's evaluated nodes in cp_word / cp_slot: cp_surf surface entries, then the interior
};

// The window img goes from slab sl - 1 (whose lo is lo_prev) to slab sl of the column col.
__device__ __forceinline__ SlabWindow slab_window_fill(const SlabTables &st, int sl, int m, double *img, const double *col, int lo_prev)
{
    constexpr int NT = CW_NT, HB = CW_HB;
    const int tid = threadIdx.x;
    // k0, ld_off, ld_cnt, cp_off, cp_cnt, cp_surf: all six are read here (the last three read behind the loads, where they are
    // returned, cost every slab kernel two vector registers, and the extrema and histogram kernels a wave per SIMD)
    const int *hd = st.head + 8 * sl;
    const int k0 = hd[0], ld_off = hd[1], ld_cnt = hd[2], cp_off = hd[3], cp_cnt = hd[4], cp_surf = hd[5];
    const int lo = plane_off(m, k0 - 1);                            // lattice range held in LDS: [lo, PO(k1 + 1))
    double *xs = img - lo;
    // the words of the first batch of loads are requested before the window is rearranged; a batch is completed with copies of
    // the list's last entry, so that every load of the phase is unconditional and inside the list
    auto ld_at = [&](int e) { return st.ld_word[ld_off + max(min(e, ld_cnt - 1), 0)]; };
    uint32_t wd0[HB];
#pragma unroll
    for (int q = 0; q < HB; ++q) wd0[q] = ld_at(q * NT + tid);
    if (sl > 0) {
        __syncthreads();                                            // previous slab fully consumed
        window_move<CW_MV>(img, lo - lo_prev, plane_off(m, k0 + 1) - lo);   // planes k0-1 and k0
    }
    for (int q = (sl > 0 ? plane_off(m, k0 + 1) - lo : 0) + tid; q < st.lds_nodes; q += NT) img[q] = 0.0;   // stale data + guard
    __syncthreads();
    // planes new in the window: HBM -> LDS, every slot of the column once
    for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
        uint32_t wd[HB];
        double xv[HB];
#pragma unroll
        for (int q = 0; q < HB; ++q) wd[q] = q0 == 0 ? wd0[q] : ld_at(q0 + q * NT + tid);
#pragma unroll
        for (int q = 0; q < HB; ++q) xv[q] = col[wd[q] >> 16];
#pragma unroll
        for (int q = 0; q < HB; ++q)
            if (q0 + q * NT + tid < ld_cnt) xs[wd[q] & 0xffffu] = xv[q];
    }
    // (whi: the end of the zero guard, the last position an address may be clamped to)
    return {lo, lo + st.lds_nodes - 1, cp_off, cp_cnt, cp_surf};
}

// The evaluated planes of the slab that slab_window_fill left in the window: f(L, len, A, B, mk, slot) for every node whose mask
// mk = elem_mask[slot] is not 0 (0: no element has its lowest vertex there).  Addressing word and slot are fetched two trips ahead
// of use, the slot's mask one; the lists are padded with valid slots: the loads of an entry behind the list's end are
// unconditional, their values unused.
template <class F>
__device__ __forceinline__ void slab_walk_masked(const SlabTables &st, const SlabWindow &w, int m, const uint8_t *__restrict__ elem_mask, F f)
{
    constexpr int NT = CW_NT;
    const int tid = threadIdx.x;
    const int cp_off = w.cp_off, cp_surf = w.cp_surf;
    const int ib = cp_off + cp_surf;                                // start of the interior part of the list
    uint32_t p0 = st.cp_word[cp_off + tid], p1 = st.cp_word[cp_off + tid + NT];
    int s0 = (int)st.cp_slot[cp_off + tid], s1 = (int)st.cp_slot[cp_off + tid + NT];
    uint32_t q0 = st.cp_word[ib + tid], q1 = st.cp_word[ib + tid + NT];
    int t0 = (int)st.cp_slot[ib + tid], t1 = (int)st.cp_slot[ib + tid + NT];
    unsigned ms = elem_mask[s0], mi = elem_mask[t0];
    __syncthreads();                                                // the window is whole
    const int nit_s = (cp_surf + NT - 1) / NT;
    for (int it = 0; it < nit_s; ++it) {                            // surface entities
        const int e = it * NT + tid;
        const uint32_t pw = p0;
        const unsigned mk = ms;
        const int slot = s0;
        p0 = p1;
        s0 = s1;
        ms = elem_mask[s0];
        p1 = st.cp_word[cp_off + e + 2 * NT];
        s1 = (int)st.cp_slot[cp_off + e + 2 * NT];
        if (e < cp_surf && mk != 0) {
            int L, len, A, B, cls, k;
            decode32w(pw, m, L, len, A, B, cls, k);
            f(L, len, A, B, mk, slot);
        }
    }
    const int n_int = w.cp_cnt - cp_surf;
    const int nit_i = (n_int + NT - 1) / NT;
    for (int it = 0; it < nit_i; ++it) {                            // cell interior
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
            f(L, len, A, B, mk, slot);
        }
    }
}

struct RowsWindow {
    int lo, whi;                     // as SlabWindow's
};

// The window img goes from the band before [j0, j1) (whose lo is lo_prev) to that band of the column col.
__device__ __forceinline__ RowsWindow rows_window_fill(int m, int nei, int off_int, int j0, int j1, double *img, const double *col,
                                                       int lo_prev)
{
    constexpr int NT = CW_NT, HB = CW_HB;
    const int tid = threadIdx.x;
    const int lo = rows_ro(m, j0 - 1);                              // lattice range held in LDS: [lo, hi) + guard
    const int hi = rows_ro(m, j1 + 1);
    int ld_first = 0;                                               // first lattice position that comes from HBM
    if (j0 > 0) {
        __syncthreads();                                            // previous band fully consumed
        ld_first = rows_ro(m, j0 + 1);
        window_move<RW_MV>(img, lo - lo_prev, ld_first - lo);       // rows j0-1 and j0
    }
    for (int q = hi - lo + tid; q < hi - lo + RW_GUARD; q += NT) img[q] = 0.0;   // guard behind the window
    // rows new in the window: HBM -> LDS, every slot of the column once; batches of HB slots per thread
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
        for (int q = 0; q < HB; ++q) xv[q] = col[tt[q]];
#pragma unroll
        for (int q = 0; q < HB; ++q)
            if (q0 + q * NT + tid < ld_cnt) img[ld_first - lo + q0 + q * NT + tid] = xv[q];
    }
    return {lo, hi + RW_GUARD - 1};
}

// Rows [j0, j1) of the band that rows_window_fill left in the window: f(L, len, 0, 0, mk, slot) as slab_walk_masked.  The node's
// row and its mask are formed one trip ahead of use; a trip behind the band's end repeats its last node: every mask load is
// unconditional and inside the level's mask.
template <class F>
__device__ __forceinline__ void rows_walk_masked(int m, int nei, int off_int, int j0, int j1, const uint8_t *__restrict__ elem_mask, F f)
{
    constexpr int NT = CW_NT;
    const int tid = threadIdx.x;
    const int e0 = rows_ro(m, j0), ecnt = rows_ro(m, j1) - e0;
    auto node_at = [&](int e, int &L, int &j, unsigned &mk, int &slot) {
        L = e0 + min(e, ecnt - 1);
        j = rows_row_near(m, L);
        slot = rows_slot_at(m, L, j, nei, off_int);
        mk = elem_mask[slot];
    };
    int Ln, jn, sn;
    unsigned mkn;
    node_at(tid, Ln, jn, mkn, sn);
    __syncthreads();                                                // the window is whole
    for (int q0 = 0; q0 < ecnt; q0 += NT) {
        const int e = q0 + tid, L = Ln, j = jn, slot = sn;
        const unsigned mk = mkn;
        node_at(e + NT, Ln, jn, mkn, sn);
        if (e < ecnt && mk != 0) f(L, m + 1 - j, 0, 0, mk, slot);
    }
}

// Host side.  Can the walks above address this level?  3D: the slab tables are there, the packed words (L and the slot in 16 bits
// each, i, j, k in 7 bits each) hold this level's values, two planes fit the move.  2D: the storage order rows_slot assumes, the
// window of the widest band (rows 0..2 at least) plus the guard fits, and so does the move of two rows.  What a kernel puts next
// to the window, and whether both fit the LDS, is its module's to check.
inline bool window_layout_ok(const LevelDev &lv, const SlabTables &st)
{
    if (lv.nf <= 0 || lv.ld < lv.nf) return false;
    if (lv.dim == 3) {
        if (!st.head || !st.ld_word || !st.cp_word || !st.cp_slot || st.nslab < 1 || st.lds_nodes <= 0) return false;
        return lv.m >= 1 && lv.m <= 127 && lv.nf <= 0x10000 && (lv.m + 1) * (lv.m + 1) <= CW_MV * CW_NT;
    }
    if (lv.dim != 2 || lv.ncorner != 3 || lv.nedge != 3 || lv.nface != 0) return false;
    if (lv.m < 2 || lv.m > 1024 || lv.nei != lv.m - 1 || lv.off_int != 3 + 3 * lv.nei || lv.nf != rows_ro(lv.m, lv.m + 1)) return false;
    return rows_ro(lv.m, 3) + RW_GUARD <= RW_WIN && 2 * (lv.m + 1) <= RW_MV * RW_NT;
}

// one workgroup per cell, lds bytes of dynamic LDS each
template <class K, class... Args>
void launch_cells(K kern, size_t lds, const Launch &L, int64_t ncells, Args... args)
{
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ncells), dim3(CW_NT), lds, L.stream, args...);
    check_launch();
}

}  // namespace hmg
