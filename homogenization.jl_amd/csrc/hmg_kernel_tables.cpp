// Addressing tables of the apply and transfer kernels, derived on the host from the reference tables (LevelTables) and the
// base mesh (MeshTables).  No device here: hmg_upload.cpp uploads what these builders return, as it is.
#include "hmg_device.hpp"
#include "hmg_host.hpp"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <utility>

namespace hmg {

namespace {

// i | j<<7 | k<<14 | cls<<21: the wide addressing word, decoded by decode32w (hmg_stencil.hpp)
uint32_t word32w(uint32_t i, uint32_t j, uint32_t k, uint32_t c) { return (i & 127u) | (j & 127u) << 7 | (k & 127u) << 14 | c << 21; }

// L | j<<16 | k<<23: the lattice-position word of cell-interior nodes, decoded by decode_lattice (hmg_stencil.hpp)
uint32_t word_lattice(uint32_t L, uint32_t j, uint32_t k) { return L | ((j & 127u) << 16) | ((k & 127u) << 23); }

uint32_t lattice_pos(const LevelTables &T, int slot) { return (uint32_t)(T.meta[(size_t)slot] & 0xffffu); }

// storage slot of lattice node (i,j,k) of a level (-1: no such node)
struct LatticeIndex {
    int n;
    std::vector<int32_t> slot;
    explicit LatticeIndex(const LevelTables &T) : n(T.m + 1), slot((size_t)n * n * (T.dim == 3 ? n : 1), -1)
    {
        for (int q = 0; q < T.nf; ++q) slot[idx(T.slot_ijk[3 * q], T.slot_ijk[3 * q + 1], T.slot_ijk[3 * q + 2])] = q;
    }
    size_t idx(int i, int j, int k) const { return ((size_t)k * n + j) * n + i; }
    int32_t operator()(int i, int j, int k) const { return slot[idx(i, j, k)]; }
};

// restriction weight of tap d of class c: 1 on the node itself, 0.5 on every other tap that exists (nonzero mass entry)
double restriction_weight(const LevelTables &T, int c, int d)
{
    return T.ctab[((size_t)c * T.ndir + d) * T.nterm + T.nterm - 1] != 0.0 ? (d == 0 ? 1.0 : 0.5) : 0.0;
}

// v in the XCD-aware order: workgroup b runs on XCD b % 8, and XCD x walks the x-th contiguous eighth of v
std::vector<int32_t> xcd_order(const std::vector<int32_t> &v)
{
    const int64_t n = (int64_t)v.size(), len = (n + 7) / 8;
    std::vector<int32_t> o((size_t)n);
    int64_t k = 0;
    for (int64_t b = 0; k < n; ++b) {
        const int64_t pos = b / 8, c = (b % 8) * len + pos;
        if (pos < len && c < n) o[(size_t)k++] = v[(size_t)c];
    }
    return o;
}

}  // namespace

AddressTables build_address_tables(const LevelTables &T)
{
    AddressTables A;
    if (!T.meta.empty()) {
        std::vector<int32_t> slot_of_L(T.nf, -1);   // storage slot of every lattice position
        for (int q = 0; q < T.nf; ++q) slot_of_L[lattice_pos(T, q)] = q;
        const bool compact_ok = T.dim == 3 ? T.m <= 63 : T.m <= 255;
        // L | j<<16 | k<<22 | cls<<28, decoded by decode32 (hmg_stencil.hpp)
        auto pack32 = [&](uint64_t mt, int cls) -> uint32_t {
            if (!compact_ok) return 0u;
            const int sl = slot_of_L[(size_t)(mt & 0xffffu)];
            const uint32_t j = T.slot_ijk[3 * sl + 1], k = T.slot_ijk[3 * sl + 2];
            return (uint32_t)(mt & 0xffffu) | (j << 16) | (T.dim == 3 ? (k << 22) : 0u) | ((uint32_t)cls << 28);
        };
        A.lpos.resize(T.meta.size());
        A.pos32.resize(T.meta.size());
        A.pos32w.resize(T.meta.size());
        A.sweep32.resize(T.sweep_meta.size());
        for (size_t q = 0; q < A.pos32.size(); ++q) {
            A.lpos[q] = (uint16_t)lattice_pos(T, (int)q);
            A.pos32[q] = pack32(T.meta[q], T.slot_cls[q]);
            const uint32_t i = T.slot_ijk[3 * q], j = T.slot_ijk[3 * q + 1], k = T.slot_ijk[3 * q + 2];
            if (T.dim == 3 && (i > 127 || j > 127 || k > 127)) throw std::runtime_error("lattice coordinate exceeds 127");
            A.pos32w[q] = word32w(i, j, k, T.slot_cls[q]);
        }
        for (size_t q = 0; q < A.sweep32.size(); ++q) A.sweep32[q] = pack32(T.sweep_meta[q], 0);
        // padding read (never used) by k_apply's two-ahead table prefetch: see TABLE_PAD there
        A.pos32.resize(A.pos32.size() + TABLE_PAD, 0u);
        A.sweep32.resize(A.sweep32.size() + TABLE_PAD, 0u);
    } else {
        // 2D levels 9..11 have no packed words (see build_level_tables): the row-band kernels (hmg_apply_rows.hip) derive slot
        // and class from (i,j) -- check that rule here
        for (int q = 0; q < T.nf; ++q) {
            int cls = -1;
            const int sl = rows_slot(T.m, T.slot_ijk[3 * q], T.slot_ijk[3 * q + 1], T.nei, T.off_int, cls);
            if (T.dim != 2 || sl != q || cls != (int)T.slot_cls[q]) throw std::runtime_error("row-band apply: slot rule broken");
        }
    }
    A.sweep_slot = T.sweep_slot;
    A.sweep_slot.resize(A.sweep_slot.size() + TABLE_PAD, (uint16_t)0xffff);
    return A;
}

BlockedInterior build_blocked_interior(const LevelTables &T)
{
    // every R-th interior k-plane, all its interior (i,j) in lattice order; R = 6 makes the 4495 interior nodes of level 6
    // 945 entries, one pass of a 1024-thread workgroup (level 5: R = 4, 152 entries for its 256-thread workgroup)
    BlockedInterior B;
    if (!(T.dim == 3 && T.nint > 0 && T.m <= 63 && (T.nf > 2048 || (T.nf > 256 && T.nf <= 1024)) &&
          sizeof(double) * (size_t)(T.nf + 512) <= 160 * 1024))
        return B;
    const int R = T.nf > 2048 ? 6 : 4, m = T.m;
    const LatticeIndex at(T);
    auto tri = [](int n) { return (n + 1) * (n + 2) / 2; };
    size_t covered = 0;
    for (int k0 = 1; k0 <= m - 3; k0 += R)
        for (int j = 1; j + k0 <= m - 2; ++j)
            for (int i = 1; i + j + k0 <= m - 1; ++i) {
                const int nv = std::min(R, m - i - j - k0);
                const int sl = at(i, j, k0);
                if (sl < T.off_int || T.slot_cls[sl] != 0) throw std::runtime_error("blocked interior: not an interior node");
                // the kernel derives the slots of the R nodes from the first: check that rule here
                int ds = tri(m - k0 - 3) - (j - 1), cur = sl;
                for (int r = 1; r < nv; ++r) {
                    cur += ds;
                    ds -= (m - k0) - 1 - r;
                    if (cur != at(i, j, k0 + r)) throw std::runtime_error("blocked interior: slot rule broken");
                }
                B.word.push_back(lattice_pos(T, sl) | ((uint32_t)j << 16) | ((uint32_t)k0 << 22) | ((uint32_t)nv << 28));
                B.slot.push_back((uint16_t)sl);
                covered += nv;
            }
    if ((int)covered != T.nint) throw std::runtime_error("blocked interior: tables do not cover the interior");
    // the same instantiation evaluates the faces one class per wave and skips the taps that leave the cell (face_tap_mask in
    // hmg_stencil.hpp: f0 k = 0, f1 j = 0, f2 i = 0, f3 i+j+k = m; an edge node keeps the taps both of its faces keep,
    // edge_tap_mask): check them against the class table, and the run counts the kernel is compiled for (4 waves x 2 runs of
    // 64 per face, 3 runs of 64 for corners + edges)
    const uint32_t f0 = 1u << 8 | 1u << 10 | 1u << 12 | 1u << 14, f1 = 1u << 4 | 1u << 6 | 1u << 7 | 1u << 13,
                   f2 = 1u << 2 | 1u << 3 | 1u << 9 | 1u << 14, f3 = 1u << 1 | 1u << 5 | 1u << 11 | 1u << 13;
    const uint32_t absent[10] = {f0, f1, f2, f3, f0 | f1, f0 | f2, f1 | f2, f0 | f3, f1 | f3, f2 | f3};   // classes 1..10
    const int nw = T.nf > 2048 ? 16 : 4;     // waves of the workgroup that runs this level
    bool ok = T.nface == 4 && T.nfi <= 128 * std::max(nw / 4, 1) && T.nei <= 64 && (int)B.word.size() <= (nw - 1) * 64;
    for (int c = 0; ok && c < (T.nedge == 6 ? 10 : 4); ++c)
        for (int d = 0; d < T.ndir; ++d)
            for (int t = 0; t < T.nterm; ++t)   // a tap the kernel skips carries weight
                if (((absent[c] >> d) & 1u) && T.ctab[((size_t)(1 + c) * T.ndir + d) * T.nterm + t] != 0.0) ok = false;
    if (!ok) throw std::runtime_error("blocked apply: the class table does not match the kernel's face / edge tap masks");
    B.nblk = (int)B.word.size();
    B.R = R;
    B.word.resize(B.word.size() + TABLE_PAD, 0u);
    B.slot.resize(B.slot.size() + TABLE_PAD, (uint16_t)0);
    return B;
}

SlabWindows build_slab_windows(const LevelTables &T, const LevelTables *coarse, int lds_kb)
{
    // needed by the apply of levels whose cell exceeds the LDS (level 7), and used by the restriction of every large 3D level
    // (level 6: the whole cell is one slab)
    SlabWindows S;
    if (!(T.dim == 3 && T.nf > 2048)) return S;
    // greedy slabs of k-planes: the rolling window [k0-1, k1] (+ guard) of k_apply_slab must fit lds_kb
    const int cap = (lds_kb * 1024) / 8 - 232;
    auto po = [&](int k) {
        long long n1 = T.m + 1, n2 = T.m + 1 - std::min(std::max(k, 0), T.m + 1);
        return (int)((n1 * (n1 + 1) * (n1 + 2) - n2 * (n2 + 1) * (n2 + 2)) / 6);
    };
    std::vector<int> sk{0};
    while (sk.back() <= T.m) {
        int k0 = sk.back(), k1 = k0 + 1;
        while (k1 <= T.m && T.lds_g1 + po(k1 + 2) - po(k0 - 1) <= cap) ++k1;
        int nn = T.lds_g1 + po(k1 + 1) - po(k0 - 1);
        if (nn > cap) throw std::runtime_error("apply slabs: a single plane does not fit the LDS");
        S.lds_nodes = std::max(S.lds_nodes, nn);
        sk.push_back(k1);
    }
    S.nslab = (int)sk.size() - 1;
    // Inside every entity segment the slots are ordered by plane k, so the slots of planes [ka, kb) are
    // one contiguous run.  15 segments: 4 corners, 6 edges, 4 faces, interior.
    std::vector<std::pair<int, int>> seg;
    for (int c = 0; c < T.ncorner; ++c) seg.push_back({c, c + 1});
    for (int e = 0; e < T.nedge; ++e) seg.push_back({T.off_edge + e * T.nei, T.off_edge + (e + 1) * T.nei});
    for (int f = 0; f < T.nface; ++f) seg.push_back({T.off_face + f * T.nfi, T.off_face + (f + 1) * T.nfi});
    seg.push_back({T.off_int, T.nf});                    // interior last: the kernel's fast path
    auto run = [&](std::pair<int, int> sg, int ka, int kb) {   // slots of the segment with ka <= k < kb
        auto in = [&](int t) { return T.slot_ijk[3 * t + 2] >= ka && T.slot_ijk[3 * t + 2] < kb; };
        int b = sg.second, e = sg.first;
        for (int t = sg.first; t < sg.second; ++t)
            if (in(t)) { b = std::min(b, t); e = t + 1; }
        for (int t = b; t < e; ++t)
            if (!in(t)) throw std::runtime_error("apply slabs: plane range is not contiguous");
        return b < e ? std::make_pair(b, e) : std::make_pair(0, 0);
    };
    // flat lists per slab (k_apply_slab): slots new in the rolling window (planes k0-1 and k0 come from the previous slab's
    // LDS image) ...
    S.head.assign((size_t)S.nslab * 8, 0);
    for (int sl = 0; sl < S.nslab; ++sl) {
        S.head[sl * 8 + 0] = sk[sl];
        S.head[sl * 8 + 1] = (int)S.ld_word.size();
        for (const auto &sg : seg) {
            const auto ld = run(sg, sl == 0 ? 0 : sk[sl] + 1, sk[sl + 1] + 1);
            for (int t = ld.first; t < ld.second; ++t) S.ld_word.push_back(lattice_pos(T, t) | ((uint32_t)t << 16));
        }
        S.head[sl * 8 + 2] = (int)S.ld_word.size() - S.head[sl * 8 + 1];
    }
    // ... and nodes evaluated, surface entities first (head fields 3..5), output slot out(t) or -1 (not evaluated): the surface in
    // the wide form, the cell interior (round 4) in the lattice form (decode_lattice: no tetrahedral-number arithmetic per node)
    auto eval_lists = [&](std::vector<int> &head, std::vector<uint32_t> &word, std::vector<uint16_t> &slot, int &max_surf,
                          int &max_int, auto out) {
        for (int sl = 0; sl < S.nslab; ++sl) {
            int *h = &head[(size_t)sl * 8];
            h[3] = (int)word.size();
            for (size_t si = 0; si < seg.size(); ++si) {
                const bool interior = si + 1 == seg.size();
                if (interior) h[5] = (int)word.size() - h[3];
                const auto cp = run(seg[si], sk[sl], sk[sl + 1]);
                for (int t = cp.first; t < cp.second; ++t) {
                    const int o = out(t);
                    if (o < 0) continue;
                    const uint32_t i = T.slot_ijk[3 * t], j = T.slot_ijk[3 * t + 1], k = T.slot_ijk[3 * t + 2];
                    word.push_back(interior ? word_lattice(lattice_pos(T, t), j, k) : word32w(i, j, k, T.slot_cls[t]));
                    slot.push_back((uint16_t)o);
                }
            }
            h[4] = (int)word.size() - h[3];
            max_surf = std::max(max_surf, h[5]);
            max_int = std::max(max_int, h[4] - h[5]);
        }
    };
    eval_lists(S.head, S.cp_word, S.cp_slot, S.max_surf, S.max_int, [](int t) { return t; });
    if ((int)S.ld_word.size() != T.nf || (int)S.cp_word.size() != T.nf)
        throw std::runtime_error("apply slabs: the slab lists do not cover the cell exactly once");
    // k_apply_slab2 (hmg_apply_slab.hip) takes the interior slots of a slab as one run of consecutive slots
    for (int sl = 0; sl < S.nslab; ++sl)
        for (int q = S.head[sl * 8 + 3] + S.head[sl * 8 + 5] + 1; q < S.head[sl * 8 + 3] + S.head[sl * 8 + 4]; ++q)
            if (S.cp_slot[(size_t)q] != S.cp_slot[(size_t)q - 1] + 1)
                throw std::runtime_error("apply slabs: interior slots of a slab are not consecutive");
    S.ld_word.resize(S.ld_word.size() + TABLE_PAD, 0u);
    S.cp_word.resize(S.cp_word.size() + TABLE_PAD, 0u);
    S.cp_slot.resize(S.cp_slot.size() + TABLE_PAD, (uint16_t)0);
    if (!coarse) return S;
    // restriction through the same window (launch_restrict_slab): evaluated nodes = the even lattice nodes (= nodes of the
    // coarser level), output slot = their COARSE storage slot
    const LatticeIndex cslot(*coarse);
    S.rs_head = S.head;
    eval_lists(S.rs_head, S.rs_word, S.rs_slot, S.rs_max_surf, S.rs_max_int, [&](int t) {
        const int i = T.slot_ijk[3 * t], j = T.slot_ijk[3 * t + 1], k = T.slot_ijk[3 * t + 2];
        if ((i | j | k) & 1) return -1;
        const int cs = cslot(i / 2, j / 2, k / 2);
        if (cs < 0) throw std::runtime_error("slab restriction: even node without a coarse slot");
        return cs;
    });
    if ((int)S.rs_word.size() != coarse->nf) throw std::runtime_error("slab restriction: lists do not cover the coarse cell");
    S.rs_word.resize(S.rs_word.size() + TABLE_PAD, 0u);
    S.rs_slot.resize(S.rs_slot.size() + TABLE_PAD, (uint16_t)0);
    // the weights in class-table layout: the mass term of every (class, tap)
    S.rtab.assign(T.ctab.size(), 0.0);
    for (int c = 0; c < T.ncls; ++c)
        for (int d = 0; d < T.ndir; ++d) S.rtab[((size_t)c * T.ndir + d) * T.nterm + T.nterm - 1] = restriction_weight(T, c, d);
    return S;
}

TransferTables build_transfer_tables(const LevelTables &T, const LevelTables *coarse, const BlockedInterior &blk)
{
    TransferTables X;
    if (!coarse || coarse->nf <= 0x10000) {
        // 16-bit parent pairs (not built where the coarse cell has more slots -- 2D level 11; its prolongation reads par_a / par_b)
        X.par32.resize(T.par_a.size());
        for (size_t q = 0; q < X.par32.size(); ++q) {
            if ((uint32_t)T.par_a[q] > 0xffffu || (uint32_t)T.par_b[q] > 0xffffu) throw std::runtime_error("coarse slot exceeds 16 bits");
            X.par32[q] = (uint32_t)T.par_a[q] | ((uint32_t)T.par_b[q] << 16);
        }
    }
    if (!(coarse && T.dim == 3 && blk.nblk > 0 && T.nf <= 0xffff)) return X;
    // folded prolongation, coarse column staged in the image itself (k_apply<.., CG>): coarse slot c = lattice node (ci,cj,ck)
    // of the coarser level sits at the fine lattice node (2ci,2cj,2ck); the restriction in the epilogue (k_apply<.., RS>) reads it
    const LevelTables &C = *coarse;
    const LatticeIndex fslot(T);
    X.clpos.resize((size_t)C.nf);
    X.rs_word.resize((size_t)C.nf);
    for (int c = 0; c < C.nf; ++c) {
        const int i = 2 * C.slot_ijk[3 * c], j = 2 * C.slot_ijk[3 * c + 1], k = 2 * C.slot_ijk[3 * c + 2];
        const int fs = fslot(i, j, k);
        if (fs < 0) throw std::runtime_error("prolongation tables: coarse node without a fine lattice node");
        if (i > 127 || j > 127 || k > 127) throw std::runtime_error("restriction tables: bad coarse node");
        X.clpos[c] = (uint16_t)lattice_pos(T, fs);
        X.rs_word[c] = word32w(i, j, k, T.slot_cls[fs]);
    }
    X.par64.resize((size_t)T.nf);
    for (int q = 0; q < T.nf; ++q) {
        const uint64_t a = X.clpos[(size_t)T.par_a[q]], b = X.clpos[(size_t)T.par_b[q]], self = lattice_pos(T, q);
        // (an identity row is its own parent: the coarse value sits where the slot's own value will go)
        if (T.par_a[q] == T.par_b[q] && a != self) throw std::runtime_error("prolongation tables: identity row off its node");
        X.par64[q] = a | (b << 16) | (self << 32);
    }
    // the epilogue's weights: those of the stand-alone restriction (SlabWindows::rtab / launch_restrict_slab) per (class, tap)
    X.rs_w.resize((size_t)T.ncls * T.ndir);
    for (int c = 0; c < T.ncls; ++c)
        for (int d = 0; d < T.ndir; ++d) X.rs_w[(size_t)c * T.ndir + d] = restriction_weight(T, c, d);
    if (T.nf <= 2048) {
        // levels whose stand-alone restriction is k_restrict: the epilogue sums in ITS order (the reference's: identity row
        // first, then the midpoints in ascending fine hierarchical id) -- same bits on both paths
        X.rs_lp.resize(T.ridx.size());
        for (size_t e = 0; e < X.rs_lp.size(); ++e) X.rs_lp[e] = (uint16_t)lattice_pos(T, T.ridx[e]);
    }
    return X;
}

WaveTables build_wave_tables(const LevelTables &T, const LevelTables *coarse, const BlockedInterior &blk,
                             const std::vector<uint16_t> &clpos)
{
    // Tables of k_apply_wave (hmg_apply_wave.hip): what lane l of the one wave that owns a cell needs, row by row.
    //   tab rows 0..7   faces: run r = 2 f + h covers nodes h * 64 + l of face f
    //       rows 8..9   corners and edges: slot r * 64 + l (< WNEC)
    //       rows 10..12 interior blocks u = r * 64 + l (< WNBLK): the block word of the blocked tables
    //       row 13      storage slot of block l | of block 64 + l << 16
    //       row 14      storage slot of block 128 + l | class of slot l << 16 | class of slot 64 + l << 24
    //   surface words: L | len << 10 | A << 15 | B << 23 | valid << 31 (rows have len = m+1-j-k nodes, A / B = offsets
    //   to the same (i,j) in the plane above / below, as decode32 derives them)
    WaveTables W;
    if (!(T.dim == 3 && T.m == WM && T.nf == WNF && blk.nblk == WNBLK && blk.R == WR && T.lds_g0 == 0 && T.nfi == WNFI &&
          T.nei == WNEI && T.ncorner == WNCORNER && T.nedge == 6 && T.nface == 4 && T.off_edge == WOFF_EDGE &&
          T.off_face == WOFF_FACE))
        return W;
    const int m = T.m, WDUMMY = WVZ - 1;   // (lanes without a slot write to the last spare double in front of the image)
    auto surf_word = [&](int t, bool valid) -> uint32_t {
        const uint32_t L = lattice_pos(T, t);
        const int j = T.slot_ijk[3 * t + 1], k = T.slot_ijk[3 * t + 2];
        const int len = m + 1 - j - k, n = m - k, Tk = (n + 1) * (n + 2) / 2, A = Tk - j, Bo = Tk + n + 2 - j;
        if (L > 1023u || len < 0 || len > 31 || A < 0 || A > 255 || Bo < 0 || Bo > 255)
            throw std::runtime_error("wave tables: addressing word out of range");
        return L | ((uint32_t)len << 10) | ((uint32_t)A << 15) | ((uint32_t)Bo << 23) | (valid ? 1u << 31 : 0u);
    };
    W.tab.assign((size_t)WAVE_TAB_ROWS * 64, 0u);
    W.lpos.assign(8 * 64, 0u);
    for (int l = 0; l < 64; ++l) {
        for (int r = 0; r < 8; ++r) {
            const int f = r >> 1, ti = (r & 1) * 64 + l;
            const bool valid = ti < WNFI;
            W.tab[(size_t)r * 64 + l] = surf_word(WOFF_FACE + f * WNFI + (valid ? ti : 0), valid);
        }
        uint32_t cls[2];
        for (int r = 0; r < 2; ++r) {
            const int t = r * 64 + l;
            const bool valid = t < WNEC;
            W.tab[(size_t)(8 + r) * 64 + l] = surf_word(valid ? t : 0, valid);
            cls[r] = T.slot_cls[(size_t)(valid ? t : WOFF_EDGE)];
            if (cls[r] < 5 || cls[r] > 14) throw std::runtime_error("wave tables: edge / corner class out of range");
        }
        uint32_t bsl[3];
        for (int r = 0; r < 3; ++r) {
            const int u = r * 64 + l;
            const bool valid = u < WNBLK;
            // (no block: block 0's addresses with no valid node -- nothing is stored)
            W.tab[(size_t)(10 + r) * 64 + l] = valid ? blk.word[(size_t)u] : (blk.word[0] & 0x0fffffffu);
            bsl[r] = blk.slot[(size_t)(valid ? u : 0)];
        }
        W.tab[(size_t)13 * 64 + l] = bsl[0] | (bsl[1] << 16);
        W.tab[(size_t)14 * 64 + l] = bsl[2] | (cls[0] << 16) | (cls[1] << 24);
        for (int q = 0; q < WNQ; ++q) {   // LDS byte offsets of the lane's slots l + 64 q, two per word
            const int t = l + 64 * q;
            W.lpos[(size_t)(q / 2) * 64 + l] |= 8u * (uint32_t)(t < WNF ? WVZ + (int)lattice_pos(T, t) : WDUMMY) << (16 * (q & 1));
        }
    }
    if (!(coarse && !clpos.empty() && coarse->nf == WNFC)) return W;
    W.par.assign(16 * 64, 0u);
    W.cl.assign(3 * 64, 8u * (uint32_t)WDUMMY);
    W.rs.assign((size_t)192 * 8, 0u);
    for (int t = 0; t < T.nf; ++t) W.par[(size_t)t] = (uint32_t)clpos[(size_t)T.par_a[t]] | ((uint32_t)clpos[(size_t)T.par_b[t]] << 16);
    for (int c = 0; c < coarse->nf; ++c) {
        W.cl[(size_t)c] = 8u * (uint32_t)(WVZ + clpos[(size_t)c]);
        const int b = T.rptr[c], n = T.rptr[c + 1] - b;
        if (n < 1 || n > 15) throw std::runtime_error("wave tables: restriction row longer than 15");
        uint16_t e[16] = {0};
        for (int q = 0; q < n; ++q) e[q] = (uint16_t)lattice_pos(T, T.ridx[b + q]);
        e[15] = (uint16_t)n;
        for (int q = 0; q < 8; ++q) W.rs[(size_t)c * 8 + q] = (uint32_t)e[2 * q] | ((uint32_t)e[2 * q + 1] << 16);
    }
    return W;
}

MeshKernelTables build_mesh_kernel_tables(const MeshTables &M, bool xcd_lists)
{
    MeshKernelTables K;
    K.face_partner.assign((size_t)M.ncells * 4, -1);
    for (size_t q = 3 * (size_t)M.ncut_face_pairs; q + 2 < M.face_pairs.size(); q += 3) {   // (cut pairs never ride in the r-update)
        const int32_t ca = M.face_pairs[q], cb = M.face_pairs[q + 1], la = M.face_pairs[q + 2] & 15, lb = M.face_pairs[q + 2] >> 4;
        K.face_partner[(size_t)ca * 4 + la] = (cb << 2) | lb;
        K.face_partner[(size_t)cb * 4 + lb] = (ca << 2) | la;
    }
    // the class-weight-cache kernels read the masks of two neighbouring cells as ONE 32-bit word (HMG_KP(uint32_t, dmask)[cell >> 1]
    // in hmg_apply.hip / hmg_apply_wave.hip / hmg_apply_small.hip): an even number of entries, whatever the cell count
    K.dmask = M.dmask;
    if (K.dmask.size() & 1) K.dmask.push_back((uint16_t)0);
    // XCD-aware cell order of the full-grid apply launches (option cell_order): workgroups are dispatched round-robin over
    // the 8 XCDs (workgroup b -> XCD b % 8), so with cell = b every XCD's L2 sees every eighth column of every vector.  Here
    // XCD x walks the x-th contiguous eighth of the cells instead: -0.7 ... -1.3 ms per V-cycle (2, 4, 16 regions: -0.1 ... -0.4;
    // 64 regions or runs of 8 cells per XCD: slower; profiles/r03_experiments.txt).  A performance hint only: any mapping is correct.
    std::vector<int32_t> cells((size_t)M.ncells);
    std::iota(cells.begin(), cells.end(), 0);
    K.cell_perm = xcd_order(cells);
    // the cell lists of the overlapped exchange in the same order (xcd_lists false: as the partition analysis made them)
    K.cells_cut = xcd_lists ? xcd_order(M.cells_cut) : M.cells_cut;
    K.cells_inner = xcd_lists ? xcd_order(M.cells_inner) : M.cells_inner;
    return K;
}

}  // namespace hmg
