// Operator apply for gfx950 (MI355X), cell-resident form: one workgroup per cell holds the cell's lattice image in LDS (k_apply), or
// walks it through a rolling window of k-planes where it does not fit (k_apply_slab); the reductions of the fused passes; the choice of
// the kernel for a launch (apply_family, apply_cell_shape, apply_cell_role) and the launchers.  The other families live in
// hmg_apply_wave.hip, hmg_apply_small.hip, hmg_apply_slab.hip (k_apply_slab2) and hmg_apply_rows.hip.  Wave = 64 lanes everywhere.
//
// Reference behaviour reproduced (file:line in the reference checkout):
//   k_apply, k_apply_slab  src/apply_local_operators.jl:85-133 (+ :7-27 residual, + constraint mask,
//                          + the p-update and dot products of src/multigrid.jl:54-68 when FUSED)
#include "hmg_apply_launch.hpp"
#include "hmg_device.hpp"
#include "hmg_stencil.hpp"

#include <cstdio>
#include <stdexcept>
#include <string>

namespace hmg {

// ---------------------------------------------------------------------------------------------
// operator apply
// ---------------------------------------------------------------------------------------------
#ifdef HMG_PHASE_TIMING   // dev build (make phase-timing): thread 0 of every workgroup stamps its phases into blockpart
#define HMG_STAMP(i)                                                                     \
    do {   /* stamps behind the 2 * ncells reduction partials (full-grid launches only) */ \
        if (a.blockpart && !a.cell_list && tid == 0)                                     \
            a.blockpart[2 * (size_t)a.nwork + 8 * cell + (i)] = (double)wall_clock64(); \
    } while (0)
// k_apply_slab: thread 0 adds up what it spends per phase over the cell's slabs (its own time line, barrier waits included)
#define HMG_SLAB_T0() const long long _t0 = wall_clock64(); long long _tl = _t0; double _ph[5] = {0, 0, 0, 0, 0}
#define HMG_SLAB_PHASE(i)                              \
    do {                                               \
        const long long _n = wall_clock64();           \
        _ph[i] += (double)(_n - _tl);                  \
        _tl = _n;                                      \
    } while (0)
#define HMG_SLAB_STORE()                                                                      \
    do {                                                                                      \
        if (a.blockpart && tid == 0) {                                                        \
            double *_o = a.blockpart + 2 * (size_t)a.nwork + 8 * cell;                        \
            _o[0] = (double)_t0;                                                              \
            for (int _q = 0; _q < 5; ++_q) _o[1 + _q] = _ph[_q];                              \
            _o[6] = (double)wall_clock64();                                                   \
        }                                                                                     \
    } while (0)
#else
#define HMG_STAMP(i)
#define HMG_SLAB_T0()
#define HMG_SLAB_PHASE(i)
#define HMG_SLAB_STORE()
#endif

// WD: instantiation for the driver integrals (flags bit 3); CG: the folded prolongation stages the coarse column at the even nodes
// of the lattice image itself (flags bit 6; cells that fill a third of the LDS have no room for it behind the image)
// RS: the results are restricted to the coarser level in the epilogue (ApplyArgs::rcoarse, see the end of the kernel)
// WC (register-blocked instantiations): the class weight rows come from the class-weight cache of hmg_grid_set_operator
// (LevelDev::wcache, one row set per distinct coefficient row and sign of alpha: hmg_apply_wave.hip) instead of being combined
// from the class table and the cell's seven scales by every wave: ONE load per lane, requested in front of the column loads, no
// table terms held across the load phase, no products -- the same weights to the last bit (same products, same order, formed once)
// LF (fused WC instantiations): the form of the load phase is known at compile time -- 1: one stream in one batch (CG step 0),
// 2: two streams in one batch, nothing stored (a dead step), 3: the batched general form; 0: decided at run time;
// 4: a residual that carries THREE pending x-updates (ApplyArgs::x4: a fourth stream, batches of a third) -- RS: the down leg's local
// residual, restricted in the epilogue; without RS: the first residual of a V-cycle that finishes the x of the cycle before it;
// 5 (CG): the coarse column is (x + a p) + c (r + b p) of three coarse columns (ApplyArgs::xc_p, xc_r: the coarser level's post-smoother
// left both its x-updates to this pass).  One form per
// instantiation: the other forms' values do not compete for the 80 registers, and the dead step can take its rows behind the
// column loads (two whole columns in one batch are 65 registers in flight: with the rows in front it lost 0.5 ms) while the
// others take them in front.
template <int DIM, int NT, int SPT, bool FUSED, int RB, bool WD = false, bool CG = false, bool RS = false, bool WC = false, int LF = 0>
__global__ void __launch_bounds__(NT, NT >= 640 ? 8 : RB && NT == 512 ? 6 : 1)   // 2 x 1024 threads per CU need <= 64 VGPRs, 3 x 512: 80
k_apply(LevelDev lv, const double *__restrict__ coef, const uint16_t *__restrict__ dmask, ApplyArgs a)
{
    constexpr int NDIR = DIM == 3 ? 15 : 7;
    constexpr int NTERM = DIM == 3 ? 7 : 4;
    constexpr int WS = RB ? WSZ_RB : WSZ;
    extern __shared__ double smem[];
    double *W = smem;
    double *xs = smem + WS + lv.lds_g0;
    const int tid = threadIdx.x;
    // One-wave workgroups (cells of up to 192 nodes) are PERSISTENT: a launch of 196 608 of them is bound by the rate at
    // which waves can be started and by what every start repeats (kernel arguments, LDS allocation), not by the cells'
    // work -- so the launcher starts as many as are resident at once and each walks its share of the cells.  (The body
    // below is not indented for the loop: every other instantiation runs it exactly once.)
    // (round 4: a persistent loop around the one-form level-6 instantiations LF = 1 / 2 -- 70 VGPRs without it -- still spills 552 /
    //  672 B per lane: the backend hoists the addresses of every table and column load out of the loop)
    constexpr bool LOOP = NT == 64;
    int64_t blk = blockIdx.x;
    do {
    const int64_t cell = a.cell_list ? (int64_t)a.cell_list[blk] : blk;
    const int nf = lv.nf;
    HMG_STAMP(0);

    // Class weight table of this cell: W[class][dir] = sum_t ctab[class][dir][t] * s[t].  Done by the LAST
    // waves of the workgroup (their share of the column load below is the smallest), while the others are
    // already issuing their column loads -- the table's L2 latency then overlaps the HBM latency.
    // RB instantiations share no weight table: every wave combines the class rows it needs itself (below, behind its
    // column loads); the cell's coefficients are requested first, one per lane
    size_t wbase16 = 0;                 // WC: first entry of this cell's row set in the cache (wave-uniform: scalar loads)
    if constexpr (WC) wbase16 = (size_t)(2 * HMG_KP(int32_t, a.cell_class)[cell] + (a.alpha < 0.0 ? 1 : 0)) * WAVE_WSTRIDE;
    const double cv = RB && !WC ? coef[cell * 8 + (tid & 7)] : 0.0;
    if (!RB && (tid >= NT - 256 || NT <= 256)) {
        const int first = NT <= 256 ? tid : tid - (NT - 256);
        const int step = NT <= 256 ? NT : 256;
        if constexpr (WC) {
            // the whole class table of this cell's class from the cache: 225 loads per cell instead of 1575 table terms and as
            // many products -- for the one-wave workgroups of the small levels the table was most of a cell's work (level 4: 12.6 KB
            // of table terms per 1.3 KB column)
            for (int idx = first; idx < lv.ncls * NDIR; idx += step)
                W[idx] = lv.wcache[wbase16 + (size_t)((idx / NDIR) * WAVE_ROW + idx % NDIR)];
        } else {
        double s[NTERM];
        cell_scales<DIM>(coef + cell * 8, a.alpha, a.lambda, s, a.flags);
        for (int idx = first; idx < lv.ncls * NDIR; idx += step) {
            const double *c = lv.ctab + (size_t)idx * NTERM;
            double w = 0.0;
#pragma unroll
            for (int t = 0; t < NTERM; ++t) w += c[t] * s[t];
            W[idx] = w;
        }
        }
    }
    for (int q = tid; q < lv.lds_g0; q += NT) smem[WS + q] = 0.0;
    for (int q = tid; q < lv.lds_g1; q += NT) xs[nf + q] = 0.0;
    // Roles and table words.  (pos32 / sweep32 / sweep_slot / blk_* carry TABLE_PAD entries of padding -- zero words, slot
    // 0xffff -- so the two-ahead prefetch needs no bounds checks and both loops have a wave-uniform trip count.)
    // RB: one entity class per wave.  NT/64/4 waves share a face (FI runs of 64 slots each), the edges are dealt to the
    // waves from the last one backwards (NE per wave: 1 of 16 waves, 2 of 4), the last wave takes the corners instead
    // of an interior block -- the 945 blocks of level 6 fill waves 0..14, the 152 of level 5 waves 0..2.
    // 512-thread instantiation (three workgroups per CU): 2 waves per face with 4 runs each, the interior blocks in two passes
    const int m = lv.m;
    constexpr int NW = NT / 64, WPF = NW / 4 > 0 ? NW / 4 : 1, NE = NW >= 6 ? 1 : 2;
    constexpr int FI = RB && NT == 512 ? 4 : 2;
    constexpr int NPASS = RB && NT == 512 ? 2 : 1;
    // EARLY (register-blocked instantiations with registers to spare, <= 512 threads): the class rows and the
    // multiplicities are requested BEFORE the column loads and combined while the first batch of them is in flight
    // (vmcnt counts in order: waiting for the rows does not wait for the column) -- two registers live across the load
    // phase -- instead of in an exposed chain of L2 round trips between the load phase and the barrier.  (Fetching the
    // addressing words early as well costs the fused instantiation 60 spilled VGPRs.)
    constexpr bool EARLY = RB && (NT <= 256 || WC);
    const int wave = tid >> 6, lane = tid & 63;
    const int face = wave / WPF, ft0 = (wave % WPF) * (FI * 64);
    int edge[NE], ebase[NE];
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        edge[q] = NW - 1 - wave + q * NW;
        if (edge[q] >= lv.nedge) edge[q] = -1;
        ebase[q] = lv.off_edge + (edge[q] < 0 ? 0 : edge[q]) * lv.nei;
    }
    uint32_t fw[FI], ew[NE][1], cw = 0u;
#pragma unroll
    for (int q = 0; q < FI; ++q) fw[q] = 0u;
    uint32_t p0 = 0u, p1 = 0u;
    double wv = 0.0;                 // RB: lane d: interior weight d; lane 16 + d: this wave's face; lane 32 + 16 q + d: its edge q
    double c7[NTERM];
    uint32_t q0 = 0u, q1 = 0u;
    int s0 = 0, s1 = 0;
    uint32_t mq[4] = {0, 0, 0, 0};   // the cell's 16 entity multiplicities, wave-uniform -> SGPRs
    uint32_t mqr[4] = {0, 0, 0, 0};
    uint32_t dm = 0u;
    const uint32_t *iw = RB ? lv.blk_word : lv.sweep32;
    const uint16_t *is = RB ? lv.blk_slot : lv.sweep_slot;
    double cwl = 0.0;                   // WC: the last wave's corner weights (60 of them, one per lane)
    auto issue_rows = [&]() {           // class rows (L2-resident table) x the cell's 7 scales, multiplicities, Dirichlet mask
        if constexpr (WC) {
            // (wave-uniform words by scalar loads: Dirichlet mask, multiplicities; the lane's weight by one vector load)
            if (a.flags & 1) {
                const uint32_t w2 = HMG_KP(uint32_t, dmask)[cell >> 1];
                dm = (cell & 1) ? w2 >> 16 : w2 & 0xffffu;
            }
            if (RB) {
                int row = 0;
                if (lane < 15)
                    row = lane;
                else if (lane >= 16 && lane < 31)
                    row = (1 + face) * WAVE_ROW + lane - 16;
                else if (lane >= 32 && lane < 47 && edge[0] >= 0)
                    row = (1 + lv.nface + edge[0]) * WAVE_ROW + lane - 32;
                else if (NE > 1 && lane >= 48 && lane < 63 && edge[NE - 1] >= 0)
                    row = (1 + lv.nface + edge[NE - 1]) * WAVE_ROW + lane - 48;
                wv = lv.wcache[wbase16 + row];
                if (wave == NW - 1) {
                    const int cl = lane < 60 ? lane : 59;
                    cwl = lv.wcache[wbase16 + (1 + lv.nface + lv.nedge + cl / 15) * WAVE_ROW + cl % 15];
                }
            }
            if (FUSED && a.mult) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mqr[q] = HMG_KP(uint32_t, a.mult)[cell * 4 + q];
            }
            return;
        }
        dm = (a.flags & 1) ? dmask[cell] : 0u;
        if (RB) {
            int row = 0;
            if (lane < 15)
                row = lane;
            else if (lane >= 16 && lane < 31)
                row = (1 + face) * NDIR + lane - 16;
            else if (lane >= 32 && lane < 47 && edge[0] >= 0)
                row = (1 + lv.nface + edge[0]) * NDIR + lane - 32;
            else if (NE > 1 && lane >= 48 && lane < 63 && edge[NE - 1] >= 0)
                row = (1 + lv.nface + edge[NE - 1]) * NDIR + lane - 48;
#pragma unroll
            for (int t = 0; t < NTERM; ++t) c7[t] = lv.ctab[(size_t)row * NTERM + t];
        }
        if (FUSED && a.mult) {
            const uint32_t *mp = reinterpret_cast<const uint32_t *>(a.mult + cell * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) mqr[q] = mp[q];
        }
    };
    auto issue_words = [&]() {          // addressing words of this thread's surface runs and interior blocks
        if (RB) {
#pragma unroll
            for (int q = 0; q < FI; ++q) {
                const int ti = ft0 + q * 64 + lane;
                if (ti < lv.nfi) fw[q] = lv.pos32[lv.off_face + face * lv.nfi + ti];
            }
#pragma unroll
            for (int q = 0; q < NE; ++q) ew[q][0] = edge[q] >= 0 && lane < lv.nei ? lv.pos32[ebase[q] + lane] : 0u;
            if (wave == NW - 1 && lane < lv.ncorner) cw = lv.pos32[lane];
        } else {
            p0 = lv.pos32[tid];
            p1 = lv.pos32[tid + NT];
        }
        q0 = iw[tid];
        q1 = RB && NPASS < 2 ? 0u : iw[tid + NT];
        s0 = (int)is[tid];
        s1 = RB && NPASS < 2 ? 0 : (int)is[tid + NT];
    };
    auto finish_tables = [&]() {
        if constexpr (WC) {
            if (RB && wave == NW - 1 && lane < 60) W[lane] = cwl;      // the corners' rows: the only ones in LDS
            if (FUSED) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mq[q] = a.mult ? mqr[q] : 0x01010101u;
            }
            return;
        }
        if (RB) {
            double sc7[NTERM];
#pragma unroll
            for (int t = 0; t < NTERM - 1; ++t) sc7[t] = (a.flags & 2) ? 0.0 : a.alpha * readlane_f64(cv, t);
            sc7[NTERM - 1] = a.alpha * a.lambda * ((a.flags & 16) ? 1.0 : readlane_f64(cv, NTERM - 1));
#pragma unroll
            for (int t = 0; t < NTERM; ++t) wv += c7[t] * sc7[t];
            if (wave == NW - 1) {        // the corners' rows: per-lane weights, private to this wave (LDS ops of a wave are in order)
                const int cbase = (1 + lv.nface + lv.nedge) * NDIR;        // (the only rows in LDS: stored from W[0] on)
                for (int idx = cbase + lane; idx < lv.ncls * NDIR; idx += 64) {
                    double w = 0.0;
#pragma unroll
                    for (int t = 0; t < NTERM; ++t) w += lv.ctab[(size_t)idx * NTERM + t] * sc7[t];
                    W[idx - cbase] = w;
                }
            }
        }
        if (FUSED) {
#pragma unroll
            for (int q = 0; q < 4; ++q) mq[q] = a.mult ? __builtin_amdgcn_readfirstlane(mqr[q]) : 0x01010101u;   // (no table: all 1)
        }
    };
    // (measured, profiles/r04_experiments.txt: the dead step with its rows in front as well, step 0 with the words of its interior
    //  blocks in front, the dead step through the general instantiation -- no difference beyond +-0.05 ms per launch)
    constexpr bool rows_late = WC && (LF == 2 || LF == 5);   // (LF == 5: behind the coarse columns, whose three streams need the registers first)
    // (the one-form instantiations have registers to spare -- 70 of 80 --: their addressing words are requested in front of the
    //  column as well, so that nothing but the barrier stands between the column's arrival and the evaluation)
    constexpr bool WEARLY = false;       // (measured: LF == 1 with its words in front goes from 70 to 80 registers + 16 B of scratch)
    if (EARLY && !rows_late) issue_rows();
    if (WEARLY) issue_words();
    const double *xc = a.x + cell * lv.ld;
    double rr = 0.0, pap = 0.0;
    {
        // Load phase, in batches of HB slots per thread: all loads of a batch first, then its stores / LDS
        // writes, so that a store to xout / xacc (which may alias x2) never sits between two loads of a batch.
        // FUSED extras: xacc += ax * x2 (the previous CG step's x-update, x2 = p_old), xin = x + beta * x2.
        const double *x2c = FUSED && a.x2 ? a.x2 + cell * lv.ld : nullptr;
        double *xoc = FUSED && a.xout ? a.xout + cell * lv.ld : nullptr;
        double *xac = FUSED && a.xacc ? a.xacc + cell * lv.ld : nullptr;
        // x3 mode (two pending CG x-updates folded into a residual): xin = (x + ax*p1) + c2*(r2 + beta*p1), x2 = p1,
        // x3 = r2; the same three roundings as x += ax*p1; p2 = r2 + beta*p1; x += c2*p2 done one after the other
        const double *x3c = FUSED && a.x3 ? a.x3 + cell * lv.ld : nullptr;
        const double beta = x2c ? a.scal[a.s.num] / a.scal[a.s.den] : 0.0;
        const double ax = xac || x3c ? a.scal[a.a.num] / a.scal[a.a.den] : 0.0;
        const double c2 = x3c ? a.scal[a.c.num] / a.scal[a.c.den] : 0.0;
        // x4 (own instantiations, LF == 4): a third pending x-update in front of the two, x + dx4*p0 in the place of x -- the
        // roundings of x += a0*p0; x += ax*p1; p2 = r2 + beta*p1; x += c2*p2 done one after the other
        constexpr bool X4 = FUSED && LF == 4;
        const double *x4c = X4 && a.x4 ? a.x4 + cell * lv.ld : nullptr;
        const double dx4 = x4c ? a.scal[a.d.num] / a.scal[a.d.den] : 0.0;
        // FUSED, optional: the prolongation of the coarse-grid correction, xin = x + P xcoarse (interpolate_and_sum_to!,
        // src/interpolation.jl:64-74: identity rows += 1.0 c[a], midpoints += 0.5 c[a], += 0.5 c[b] in the CSC
        // column order), from the cell's coarse column staged in LDS behind the lattice image
        const double *ccol = FUSED && !RS && a.xcoarse ? a.xcoarse + cell * a.ldc : nullptr;
        // (CG, flags bit 6: no room behind the image -- see the in-image path below)
        constexpr bool cgather = FUSED && CG;
        double *cs = xs + nf + lv.lds_g1;
        double cval = 0.0;
        if (ccol && !cgather) {
            if (tid < lv.nf_coarse) cval = ccol[tid];
            for (int q = tid + NT; q < lv.nf_coarse; q += NT) cs[q] = ccol[q];
        }
        auto prolong = [&](double v, uint32_t w) {
            const uint32_t pa = w & 0xffffu, pb = w >> 16;
            if (pa == pb) return v + cs[pa];
            v += 0.5 * cs[pa];
            return v + 0.5 * cs[pb];
        };
        // CG: the coarse column goes to the EVEN nodes of the lattice image (coarse node (i,j,k) = fine node (2i,2j,2k)),
        // every thread combines its slots' parents from there into registers, and only then -- behind a second barrier --
        // the image receives the fine values: no LDS beyond the image (three workgroups per CU stay resident), no gathers
        // from global memory (round 2: two dependent L1/L2 gathers per slot made this the slowest launch of the V-cycle,
        // 4.2 TB/s), the whole column in one batch of loads like the light passes.  Same roundings as the staged form.
        if (cgather && ccol) {
            constexpr int NC = 2;                                   // coarse slots per thread (host: nf_coarse <= NC * NT)
            // CX: the coarse x is not in memory yet -- its last two CG x-updates are done here, per coarse entry, before it is staged:
            // (x + cxa*p) + cxc*(r + cxb*p), the three roundings of k_cg_x2_update
            constexpr bool CX = cgather && LF == 5;
            const double *cpc = CX ? a.xc_p + cell * a.ldc : nullptr, *crc = CX ? a.xc_r + cell * a.ldc : nullptr;
            const double cxa = CX ? to_sgpr(a.scal[a.a.num] / a.scal[a.a.den]) : 0.0;
            const double cxb = CX ? to_sgpr(a.scal[a.s.num] / a.scal[a.s.den]) : 0.0;
            const double cxc = CX ? to_sgpr(a.scal[a.c.num] / a.scal[a.c.den]) : 0.0;
            double cv2[NC], cp2[CX ? NC : 1], cr2[CX ? NC : 1];
            int cl2[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int c = tid + q * NT;
                if (c < lv.nf_coarse) {
                    cv2[q] = ccol[c];
                    if (CX) {
                        cp2[q] = cpc[c];
                        cr2[q] = crc[c];
                    }
                    cl2[q] = lv.clpos[c];
                }
            }
            if (CX) {      // (before the fine column's loads: its 13 values and words need the registers)
#pragma unroll
                for (int q = 0; q < NC; ++q)
                    if (tid + q * NT < lv.nf_coarse) cv2[q] = axpy1(cxc, axpy1(cxb, cp2[q], cr2[q]), axpy1(cxa, cp2[q], cv2[q]));
                __builtin_amdgcn_sched_barrier(0);
                if (EARLY && rows_late) issue_rows();
            }
            double xv[SPT];
            uint64_t pw[SPT];
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    xv[q] = xc[t];
                    pw[q] = lv.par64[t];
                }
            }
            if (EARLY) finish_tables();
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (tid + q * NT < lv.nf_coarse) xs[cl2[q]] = cv2[q];
            __syncthreads();                                        // coarse values in place
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    const uint32_t pa = (uint32_t)pw[q] & 0xffffu, pb = ((uint32_t)pw[q] >> 16) & 0xffffu;
                    double v = xv[q];
                    if (pa == pb)
                        v = v + lds_ld(xs + pa);
                    else {
                        v += 0.5 * lds_ld(xs + pa);
                        v = v + 0.5 * lds_ld(xs + pb);
                    }
                    xv[q] = v;
                }
            }
            __syncthreads();                                        // every parent read: the image may take the fine values
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    const double v = xv[q];
                    if (xoc) xoc[t] = v;
                    rr += v * v;
                    xs[(int)(pw[q] >> 32)] = v;
                }
            }
        }
        // A fused pass that reads nothing but its own column (CG step 0 with r itself as p: no x2 / xacc / x3 / coarse
        // column) takes the whole column in ONE batch like the plain apply -- one memory round trip instead of two.
        // (RS: the local residual with pending CG updates -- never a light pass, never a prolongation)
        const bool light = LF == 1 || (LF == 0 && !RS && FUSED && NT >= 512 && !x2c && !xac && !x3c && !ccol);   // (level 5, 256 threads: the extra path costs a resident workgroup)
        if (FUSED && light) {
            double xv[SPT];
            int lp[SPT];
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    xv[q] = xc[t];
                    lp[q] = lv.lpos[t];
                }
            }
            if (EARLY) finish_tables();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    const double v = xv[q];
                    if (xoc) xoc[t] = v;
                    rr += v * v;
                    xs[lp[q]] = v;
                }
            }
        }
        // ... and the dead step of a pre-smoother (reads r and p, forms p_new only in LDS, writes nothing): two streams
        const bool light2 = LF == 2 || (LF == 0 && !RS && FUSED && NT >= 512 && x2c && !xoc && !xac && !x3c && !ccol);
        if (FUSED && light2) {
            double xv[SPT], x2v[SPT];
            int lp[SPT];
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    xv[q] = xc[t];
                    x2v[q] = x2c[t];
                    lp[q] = lv.lpos[t];
                }
            }
            if (EARLY && rows_late) issue_rows();
            if (EARLY) finish_tables();
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = tid + q * NT;
                if (t < nf) {
                    const double v = axpy1(beta, x2v[q], xv[q]);
                    if (LF == 2 && xoc) xoc[t] = v;      // (round 4: the step that writes its direction next to the old one, lazy_top = 2)
                    rr += v * v;
                    xs[lp[q]] = v;
                }
            }
        }
        constexpr int HB = X4 ? (SPT + 2) / 3 : FUSED ? (SPT + 1) / 2 : SPT;   // (four streams: three batches hold what two of three streams do)
        // flags bit 7 (fused passes through the batch path below): x is known to be zero -- a coarse level entered with the zero
        // initial guess of src/multigrid.jl:106 -- and is not read (its memory need not even hold the zeros yet)
        // (compiled into the instantiations that can meet it only -- the local residual of a register-blocked level is the RS
        //  one -- : in the main fused instantiation the extra live value cost three spilled registers)
        const bool xzero = FUSED && (RS || RB == 0) && (a.flags & 128);
        if (!light && !light2 && !(cgather && ccol)) {
#pragma unroll
        for (int q0 = 0; q0 < SPT; q0 += HB) {
            double xv[HB], x2v[HB], xav[HB], x4v[X4 ? HB : 1];
            int lp[HB];
            uint32_t pw[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int t = tid + (q0 + q) * NT;
                if (q0 + q < SPT && t < nf) {
                    xv[q] = xzero ? 0.0 : xc[t];
                    if (X4) x4v[q] = x4c ? x4c[t] : 0.0;
                    x2v[q] = x2c ? x2c[t] : 0.0;
                    xav[q] = xac ? xac[t] : x3c ? x3c[t] : 0.0;
                    lp[q] = lv.lpos[t];
                    if (FUSED && !cgather) pw[q] = ccol ? lv.par32[t] : 0u;
                }
            }
            if (EARLY && q0 == 0) finish_tables();          // (the rows were requested before this batch's loads)
            if (FUSED && q0 == 0 && ccol && !cgather) {   // coarse column complete before the first use
                if (tid < lv.nf_coarse) cs[tid] = cval;
                __syncthreads();
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int t = tid + (q0 + q) * NT;
                if (q0 + q < SPT && t < nf) {
                    double v = xv[q];
                    if (FUSED) {
                        if (!cgather && ccol) v = prolong(v, pw[q]);
                        if (xac) xac[t] = axpy1(ax, x2v[q], xav[q]);
                        if (x3c) {
                            if (X4 && x4c) v = axpy1(dx4, x4v[q], v);
                            const double t1 = axpy1(ax, x2v[q], v);
                            const double p2 = axpy1(beta, x2v[q], xav[q]);
                            v = axpy1(c2, p2, t1);
                        } else if (x2c)
                            v = axpy1(beta, x2v[q], v);
                        if (xoc) xoc[t] = v;
                        if (!RS) rr += v * v;      // (RS: the local residual -- nobody asks for its reductions)
                    }
                    xs[lp[q]] = v;
                }
            }
        }
        }
        for (int t = tid + SPT * NT; t < nf; t += NT) {   // only for cells larger than SPT*NT
            double v = xzero ? 0.0 : xc[t];
            if (FUSED) {
                const double pv = x2c ? x2c[t] : 0.0;
                if (!cgather && ccol) v = prolong(v, lv.par32[t]);
                if (xac) xac[t] = axpy1(ax, pv, xac[t]);
                if (x3c) {
                    if (X4 && x4c) v = axpy1(dx4, x4c[t], v);
                    const double t1 = axpy1(ax, pv, v);
                    const double p2 = axpy1(beta, pv, x3c[t]);
                    v = axpy1(c2, p2, t1);
                } else if (x2c)
                    v = axpy1(beta, pv, v);
                if (xoc) xoc[t] = v;
                rr += v * v;
            }
            xs[lv.lpos[t]] = v;
        }
    }

    HMG_STAMP(1);   // column in LDS (this wave)
    // (scheduling fence: keeps the table prefetch below out of the load phase's register budget -- the
    //  1024-thread variants must stay within 64 VGPRs to keep two workgroups resident per CU)
    __builtin_amdgcn_sched_barrier(0);
    if (!WEARLY) issue_words();
    if (!EARLY) {
        issue_rows();
        finish_tables();
    }
    const double *sc = a.src ? a.src + cell * lv.ld : nullptr;
    double *oc = a.out ? a.out + cell * lv.ld : nullptr;   // null: only the reductions of a FUSED pass are wanted
    const int nsurf = lv.off_int;
    const int nsw = RB ? lv.nblk : lv.nsweep;
    const bool wdot = WD && FUSED && (a.flags & 8);   // src multiplies: out = alpha A x, pap += mult (x + src) out
    const double wself = (wdot && (a.flags & 256)) ? 0.0 : 1.0;   // ... pair form: x itself enters with weight 0, pap += mult src out
    HMG_STAMP(2);   // tables requested, before the barrier
    __syncthreads();
    HMG_STAMP(3);

    // surface entities
    const int wbase = RB ? (1 + lv.nface + lv.nedge) * NDIR : 0;     // RB: the LDS table starts at the corners' rows
    auto surface_node = [&](int t, uint32_t pw) -> double {   // any class: weight row read from the LDS class table tap by tap
        const double sv = sc ? sc[t] : 0.0;
        int L, len, A, B, cls;
        decode32<DIM>(pw, m, L, len, A, B, cls);
        double ctr;
        double o = stencil_eval_c<DIM>(W + cls * NDIR - wbase, xs, L, len, A, B, ctr);
        if (!wdot) o = sv + o;
        if ((dm >> (cls - 1)) & 1u) o = 0.0;
        if (!FUSED || oc) oc[t] = o;
        if (FUSED && !RS) {
            const int e = cls - 1;
            const uint32_t word = e < 4 ? mq[0] : e < 8 ? mq[1] : e < 12 ? mq[2] : mq[3];
            const uint32_t mu = (word >> (8 * (e & 3))) & 0xffu;
            pap += (double)mu * ((wdot ? fma(wself, ctr, sv) : ctr) * o);
        }
        return o;
    };
    // RS: every thread keeps what it evaluates (faces FI, edges NE, corner 1, interior NPASS x R values) for the epilogue
    // (dead arrays in every other instantiation)
    double kf[FI], ke[NE], kc = 0.0, ki[NPASS][RB ? RB : 1];
    if constexpr (RS && RB != 0 && DIM == 3) {
        // RS: the interior FIRST -- its sums stay in registers, and the surface runs need fewer registers beside them than the
        // blocked walk would beside the surface results (no reduction of this launch depends on the order)
        double w0e[15];
#pragma unroll
        for (int d = 0; d < NDIR; ++d) w0e[d] = readlane_f64(wv, d);
        if (tid < nsw) interior_block_keep<RB ? RB : 1, FUSED>(w0e, xs, m, nf >> 1, q0, s0, sc, oc, ki[0]);
        if (NPASS > 1 && tid + NT < nsw) interior_block_keep<RB ? RB : 1, FUSED>(w0e, xs, m, nf >> 1, q1, s1, sc, oc, ki[NPASS - 1]);
    }
    if (RB) {
        if (DIM == 3) {
            const bool fdir = (dm >> face) & 1u;
            const double fmult = (double)((mq[0] >> (8 * (face & 3))) & 0xffu);
            const int fbase = lv.off_face + face * lv.nfi;
            double nopre[FI];
#pragma unroll
            for (int q = 0; q < FI; ++q) nopre[q] = 0.0;
            if (face >= 4)
                ;
            else if (face == 0)
                face_items<0, FI, FUSED, FUSED && !RS>(wv, 16, xs, m, lv.nfi, fbase, ft0, fw, fdir, fmult, sc, oc, pap, lane, nopre, false, wdot, RS ? kf : nullptr, wself);
            else if (face == 1)
                face_items<1, FI, FUSED, FUSED && !RS>(wv, 16, xs, m, lv.nfi, fbase, ft0, fw, fdir, fmult, sc, oc, pap, lane, nopre, false, wdot, RS ? kf : nullptr, wself);
            else if (face == 2)
                face_items<2, FI, FUSED, FUSED && !RS>(wv, 16, xs, m, lv.nfi, fbase, ft0, fw, fdir, fmult, sc, oc, pap, lane, nopre, false, wdot, RS ? kf : nullptr, wself);
            else
                face_items<3, FI, FUSED, FUSED && !RS>(wv, 16, xs, m, lv.nfi, fbase, ft0, fw, fdir, fmult, sc, oc, pap, lane, nopre, false, wdot, RS ? kf : nullptr, wself);
#pragma unroll
            for (int q = 0; q < NE; ++q) {
                if (edge[q] < 0) continue;
                const int eb = lv.nface + edge[q];
                const bool edir = (dm >> eb) & 1u;
                const double emult = (double)(((eb < 4 ? mq[0] : eb < 8 ? mq[1] : mq[2]) >> (8 * (eb & 3))) & 0xffu);
                const double nop1[1] = {0.0};
                const int wl = 32 + 16 * q;
                switch (edge[q]) {
                case 0: class_items<edge_tap_mask(0), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                case 1: class_items<edge_tap_mask(1), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                case 2: class_items<edge_tap_mask(2), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                case 3: class_items<edge_tap_mask(3), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                case 4: class_items<edge_tap_mask(4), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                default: class_items<edge_tap_mask(5), 1, FUSED, FUSED && !RS>(wv, wl, xs, m, lv.nei, ebase[q], 0, ew[q], edir, emult, sc, oc, pap, lane, nop1, false, wdot, RS ? &ke[q] : nullptr, wself); break;
                }
            }
            if (wave == NW - 1 && lane < lv.ncorner) kc = surface_node(lane, cw);
        }
    } else {
        const int nit_surf = (nsurf + NT - 1) / NT;
        for (int it = 0; it < nit_surf; ++it) {
            const int t = tid + it * NT;
            const uint32_t pw = p0;
            p0 = p1;
            p1 = lv.pos32[t + 2 * NT];
            if (t < nsurf) surface_node(t, pw);
        }
    }
    HMG_STAMP(4);
    // cell interior: one weight row for all nodes
    double w0[15];
#pragma unroll
    for (int d = 0; d < NDIR; ++d) w0[d] = RB ? readlane_f64(wv, d) : to_sgpr(W[d]);
    if (RB) {
        // register-blocked interior: one pass (the host selects this instantiation only if nblk <= NT), its word
        // was fetched before the barrier
        if constexpr (!RS) {
        if (DIM == 3 && tid < nsw) {
            if (sc)
                interior_block<RB ? RB : 1, FUSED, true>(w0, xs, m, nf >> 1, q0, s0, sc, oc, pap, wdot, wself);
            else
                interior_block<RB ? RB : 1, FUSED, false>(w0, xs, m, nf >> 1, q0, s0, sc, oc, pap);
        }
        if (DIM == 3 && NPASS > 1 && tid + NT < nsw) {      // second pass (the host selects NT >= nblk / 2)
            if (sc)
                interior_block<RB ? RB : 1, FUSED, true>(w0, xs, m, nf >> 1, q1, s1, sc, oc, pap, wdot, wself);
            else
                interior_block<RB ? RB : 1, FUSED, false>(w0, xs, m, nf >> 1, q1, s1, sc, oc, pap);
        }
        }
    } else {
        const int nit_sweep = (nsw + NT - 1) / NT;
        for (int it = 0; it < nit_sweep; ++it) {
            const int u = tid + it * NT;
            const uint32_t pw = q0;
            const int t = s0;
            q0 = q1;
            s0 = s1;
            q1 = iw[u + 2 * NT];
            s1 = (int)is[u + 2 * NT];
            if (t != 0xffff) {
                const double sv = sc ? sc[t] : 0.0;
                int L, len, A, B, cls;
                decode32<DIM>(pw, m, L, len, A, B, cls);
                double ctr;
                double o = stencil_eval_v<DIM>(w0, xs + L, len, A, B, ctr);
                if (!wdot) o = sv + o;
                if (!FUSED || oc) oc[t] = o;
                if (FUSED) pap += (wdot ? fma(wself, ctr, sv) : ctr) * o;
            }
        }
    }
    HMG_STAMP(5);
    if constexpr (RS && RB != 0 && DIM == 3) {
        // Restriction in the epilogue (restrict_to!, src/interpolation.jl:52-62, of the cell-local residual this launch has just
        // formed -- src/multigrid.jl:104-105): the results go from the registers into the lattice image, which nobody reads
        // any more behind the barrier, and the coarse right-hand side is the 15-point sum 1 x own + 0.5 x neighbours at the
        // EVEN lattice nodes, taps that leave the cell weighted 0 -- tap for tap the arithmetic of the stand-alone restriction
        // (k_apply_slab with flags bit 2), so the coarse vector is the same to the last bit.  The residual itself need not go
        // to HBM at all (oc == nullptr): 16 B per fine DOF and one launch less per V-cycle.
        // (the image positions are fetched again here, in front of the barrier that hides their latency, instead of keeping the
        //  addressing words of the evaluation alive across the kernel: held, one of them was spilled, and every reload of a spilled
        //  register waits for ALL outstanding global loads -- vmcnt(0) -- in the middle of the face runs)
        int fl[FI], el[NE], cl = 0;
        uint32_t b0 = 0u, b1 = 0u;
        if (face < 4) {
#pragma unroll
            for (int q = 0; q < FI; ++q) {
                const int ti = ft0 + q * 64 + lane;
                fl[q] = ti < lv.nfi ? (int)lv.lpos[lv.off_face + face * lv.nfi + ti] : 0;
            }
        }
#pragma unroll
        for (int q = 0; q < NE; ++q) el[q] = edge[q] >= 0 && lane < lv.nei ? (int)lv.lpos[ebase[q] + lane] : 0;
        if (wave == NW - 1 && lane < lv.ncorner) cl = (int)lv.lpos[lane];
        if (tid < nsw) b0 = lv.blk_word[tid];
        if (NPASS > 1 && tid + NT < nsw) b1 = lv.blk_word[tid + NT];
        __syncthreads();
        if (face < 4) {
#pragma unroll
            for (int q = 0; q < FI; ++q)
                if (ft0 + q * 64 + lane < lv.nfi) xs[fl[q]] = kf[q];
        }
#pragma unroll
        for (int q = 0; q < NE; ++q)
            if (edge[q] >= 0 && lane < lv.nei) xs[el[q]] = ke[q];
        if (wave == NW - 1 && lane < lv.ncorner) xs[cl] = kc;
        {
            int pos[RB ? RB : 1];
            if (tid < nsw) {
                block_positions<RB ? RB : 1>(m, b0, pos);
                const int nv = (int)(b0 >> 28);
#pragma unroll
                for (int r = 0; r < (RB ? RB : 1); ++r)
                    if (r < nv) xs[pos[r]] = ki[0][r];
            }
            if (NPASS > 1 && tid + NT < nsw) {
                block_positions<RB ? RB : 1>(m, b1, pos);
                const int nv = (int)(b1 >> 28);
#pragma unroll
                for (int r = 0; r < (RB ? RB : 1); ++r)
                    if (r < nv) xs[pos[r]] = ki[NPASS - 1][r];
            }
        }
        __syncthreads();
        double *rc = a.rcoarse + cell * a.ldrc;
        if (lv.rs_lp) {
            // (levels whose stand-alone restriction is k_restrict: its order -- the reference's -- and its roundings)
            for (int c = tid; c < lv.nf_coarse; c += NT) {
                const int b = lv.rptr[c], n = lv.rptr[c + 1] - b;
                int lp[15];
#pragma unroll
                for (int q = 0; q < 15; ++q) lp[q] = lv.rs_lp[b + (q < n ? q : 0)];
                double tmp = 0.0;
                tmp += 1.0 * lds_ld(xs + lp[0]);
#pragma unroll
                for (int q = 1; q < 15; ++q)
                    if (q < n) tmp += 0.5 * lds_ld(xs + lp[q]);
                rc[c] = tmp;
            }
        } else
        for (int c = tid; c < lv.nf_coarse; c += NT) {
            int L, len, A, B, cls, k;
            decode32w(lv.rs_word[c], m, L, len, A, B, cls, k);
            const double *w = lv.rs_w + cls * NDIR;
            auto at = [&](int off) { return lds_ld(xs + max(L + off, 0)); };
            double acc = w[0] * lds_ld(xs + L);
            acc += w[1] * lds_ld(xs + L + 1);
            acc += w[2] * at(-1);
            acc += w[3] * lds_ld(xs + L + len - 1);
            acc += w[4] * at(-len);
            acc += w[5] * lds_ld(xs + L + len);
            acc += w[6] * at(-len - 1);
            acc += w[7] * lds_ld(xs + L + A - len);
            acc += w[8] * at(len + 1 - B);
            acc += w[9] * lds_ld(xs + L + A - 1);
            acc += w[10] * at(1 - B);
            acc += w[11] * lds_ld(xs + L + A);
            acc += w[12] * at(-B);
            acc += w[13] * lds_ld(xs + L + A + 1 - len);
            acc += w[14] * at(len - B);
            rc[c] = 0.0 + acc;               // (the stand-alone kernel adds its absent source value first: 0 + acc)
        }
    }
    if (FUSED && !RS) {
        __syncthreads();                     // W / xs no longer read: reuse the front of LDS for the reduction
        const double s_pap = block_sum(pap, smem);
        const double s_rr = block_sum(rr, smem);
        if (tid == 0) {
            a.blockpart[2 * cell] = s_pap;
            a.blockpart[2 * cell + 1] = s_rr;
        }
    }
    HMG_STAMP(6);
    if (LOOP) {
        blk += gridDim.x;
        if (blk >= a.nwork) break;
        __syncthreads();                         // the next cell's table and image overwrite this one's
    }
    } while (LOOP);
}

// Slab variant for cells whose lattice image exceeds the LDS (level 7 in 3D: 374 KiB).  The cell is processed in
// slabs of consecutive k-planes through a ROLLING window: the LDS holds planes [k0-1, k1] of the lattice image, the
// nodes of planes [k0, k1) are evaluated, then planes k1-1 and k1 are moved to the front of the window (LDS -> LDS)
// and only planes k1+1 .. k1' come from HBM -- every slot is read from HBM exactly once, so the load-phase side
// effects of the fused CG pass (p-update, x-update, r.r) can be attached to it as in k_apply.  Per slab the host
// provides two flat lists (SlabTables): the slots that are new in the window (LDS position | slot << 16) and the
// slots that are evaluated (addressing word + slot; surface entities first, then the cell interior), so that both
// phases are single batched / software-pipelined loops instead of one latency-bound loop per entity.  The window
// is sized so that two workgroups are resident per CU (one loads while the other computes).  Same arithmetic as
// k_apply.
template <int DIM, int NT, bool FUSED, bool WD = false>
__global__ void __launch_bounds__(NT, 8)
k_apply_slab(LevelDev lv, const double *__restrict__ coef, const uint16_t *__restrict__ dmask, ApplyArgs a, SlabTables st)
{
    constexpr int NDIR = DIM == 3 ? 15 : 7;
    constexpr int NTERM = DIM == 3 ? 7 : 4;
    constexpr int HB = FUSED ? 3 : 4;               // loads in flight per thread and stream in the load phase (64-VGPR budget)
    constexpr int MV = 5;                           // values per thread of the window move (two planes of level 7: <= 4225 nodes)
    extern __shared__ double smem[];
    double *W = smem;
    double *img = smem + WSZ;                       // lds_nodes doubles: [planes k0-1..k1 | zero guard]
    const int tid = threadIdx.x;
    const int64_t cell = a.cell_list ? (int64_t)a.cell_list[blockIdx.x] : (int64_t)blockIdx.x;
    const int m = lv.m;

    if (a.flags & 4) {   // cell-independent stencil (restriction): the weight is the last term of the class table
        for (int idx = tid; idx < lv.ncls * NDIR; idx += NT) W[idx] = lv.ctab[(size_t)idx * NTERM + NTERM - 1];
    } else {
        double s[NTERM];
        cell_scales<DIM>(coef + cell * 8, a.alpha, a.lambda, s, a.flags);
        for (int idx = tid; idx < lv.ncls * NDIR; idx += NT) {
            const double *c = lv.ctab + (size_t)idx * NTERM;
            double w = 0.0;
#pragma unroll
            for (int t = 0; t < NTERM; ++t) w += c[t] * s[t];
            W[idx] = w;
        }
    }
    const double *xc = a.x + cell * lv.ld;
    const double *x2c = FUSED && a.x2 ? a.x2 + cell * lv.ld : nullptr;
    double *xoc = FUSED && a.xout ? a.xout + cell * lv.ld : nullptr;
    double *xac = FUSED && a.xacc ? a.xacc + cell * lv.ld : nullptr;
    const double *x3c = FUSED && a.x3 ? a.x3 + cell * lv.ld : nullptr;   // two pending x-updates, see k_apply
    const double beta = to_sgpr(x2c ? a.scal[a.s.num] / a.scal[a.s.den] : 0.0);
    const double ax = to_sgpr(xac || x3c ? a.scal[a.a.num] / a.scal[a.a.den] : 0.0);
    const double c2 = to_sgpr(x3c ? a.scal[a.c.num] / a.scal[a.c.den] : 0.0);
    const uint32_t dm = (a.flags & 1) ? dmask[cell] : 0u;
    const double *sc = a.src ? a.src + cell * lv.ld : nullptr;
    double *oc = a.out ? a.out + cell * (a.out_ld ? a.out_ld : (int64_t)lv.ld) : nullptr;
    uint32_t mq[4] = {0, 0, 0, 0};   // the cell's 16 entity multiplicities, wave-uniform -> SGPRs
    if (FUSED) {
        const uint32_t *mp = reinterpret_cast<const uint32_t *>(a.mult + cell * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) mq[q] = a.mult ? __builtin_amdgcn_readfirstlane(mp[q]) : 0x01010101u;
    }
    const bool wdot = WD && FUSED && (a.flags & 8);   // src multiplies: out = alpha A x, pap += mult (x + src) out
    const double wself = (wdot && (a.flags & 256)) ? 0.0 : 1.0;   // ... pair form: x itself enters with weight 0, pap += mult src out
    double rr = 0.0, pap = 0.0;
    auto plane_off = [&](int k) {   // PO(k) = number of lattice nodes in planes < k
        if (k <= 0) return 0;
        if (k > m + 1) k = m + 1;
        const long long n1 = m + 1, n2 = m + 1 - k;
        return (int)((n1 * (n1 + 1) * (n1 + 2) - n2 * (n2 + 1) * (n2 + 2)) / 6);
    };
    HMG_SLAB_T0();
    __syncthreads();                                                // W complete
    HMG_SLAB_PHASE(0);                                              // (0: weight table)
    double w0[NDIR];                                                // interior weight row, SGPR-resident
#pragma unroll
    for (int d = 0; d < NDIR; ++d) w0[d] = to_sgpr(W[d]);
    int lo_prev = 0;
    for (int sl = 0; sl < st.nslab; ++sl) {
        const int *hd = st.head + 8 * sl;                           // k0, ld_off, ld_cnt, cp_off, cp_cnt, cp_surf
        const int k0 = hd[0], ld_off = hd[1], ld_cnt = hd[2], cp_off = hd[3], cp_cnt = hd[4], cp_surf = hd[5];
        const int lo = plane_off(k0 - 1);                           // lattice range held in LDS: [lo, PO(k1 + 1))
        double *xs = img - lo;                                      // xs[L] valid inside that range (+ zero guard)
        // (round 4) the words of the slab's first batch of loads are requested before the window is rearranged: their L2 round
        // trip -- the column loads depend on them -- runs behind the move and the zero fill instead of after them
        uint32_t wd0[HB];
#pragma unroll
        for (int q = 0; q < HB; ++q) wd0[q] = st.ld_word[ld_off + q * NT + tid];
        if (sl > 0) {
            __syncthreads();                                        // previous slab fully consumed
            // planes k0-1 and k0 (the last evaluated plane and the upper halo of the previous slab) move to the
            // front of the window; destination below source, ascending chunks, one barrier between a chunk's
            // reads and its writes
            const int cnt = plane_off(k0 + 1) - lo, src = lo - lo_prev;
            if (cnt <= MV * NT) {
                // (round 4) every thread takes its share of the two planes into registers, ONE barrier, then writes: the chunked form
                // below pays a barrier per 1024 values -- five per slab near the base of the cell
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
            } else {
            const int nchunk = (cnt + NT - 1) / NT;
            for (int c = 0; c < nchunk; ++c) {
                const int q = c * NT + tid;
                const double v = q < cnt ? img[src + q] : 0.0;
                __syncthreads();
                if (q < cnt) img[q] = v;
            }
            }
        }
        for (int q = (sl > 0 ? plane_off(k0 + 1) - lo : 0) + tid; q < st.lds_nodes; q += NT) img[q] = 0.0;   // stale data + guard
        __syncthreads();
        HMG_SLAB_PHASE(1);                                          // (1: window move + zero fill, with the wait for the previous slab's consumers)
        // planes new in the window: HBM -> LDS, every slot once; batches of HB slots per thread, all loads of a
        // batch before its stores (xout / xacc may alias x2)
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            uint32_t wd[HB];
            double xv[HB], x2v[HB], xav[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int v = q0 + q * NT + tid;
                wd[q] = q0 == 0 ? wd0[q] : st.ld_word[ld_off + v];   // (list is padded: no bounds check)
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int v = q0 + q * NT + tid;
                if (v < ld_cnt) {
                    const int t = (int)(wd[q] >> 16);
                    xv[q] = xc[t];
                    x2v[q] = x2c ? x2c[t] : 0.0;
                    xav[q] = xac ? xac[t] : x3c ? x3c[t] : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int v = q0 + q * NT + tid;
                if (v < ld_cnt) {
                    const int t = (int)(wd[q] >> 16);
                    double val = xv[q];
                    if (FUSED) {
                        if (xac) xac[t] = axpy1(ax, x2v[q], xav[q]);
                        if (x3c) {
                            const double t1 = axpy1(ax, x2v[q], val);
                            const double p2 = axpy1(beta, x2v[q], xav[q]);
                            val = axpy1(c2, p2, t1);
                        } else if (x2c)
                            val = axpy1(beta, x2v[q], val);
                        if (xoc) xoc[t] = val;
                        rr += val * val;
                    }
                    xs[wd[q] & 0xffffu] = val;
                }
            }
        }
        // evaluated planes, surface entities first: addressing word and slot fetched two iterations ahead of use
        const int ib = cp_off + cp_surf;                            // start of the interior part of the list
        uint32_t p0 = st.cp_word[cp_off + tid], p1 = st.cp_word[cp_off + tid + NT];
        int s0 = (int)st.cp_slot[cp_off + tid], s1 = (int)st.cp_slot[cp_off + tid + NT];
        uint32_t q0 = st.cp_word[ib + tid], q1 = st.cp_word[ib + tid + NT];
        int t0 = (int)st.cp_slot[ib + tid], t1 = (int)st.cp_slot[ib + tid + NT];
        __syncthreads();
        HMG_SLAB_PHASE(2);                                          // (2: HBM -> LDS, to the barrier behind it)
        const int nit_s = (cp_surf + NT - 1) / NT;
        for (int it = 0; it < nit_s; ++it) {
            const int v = it * NT + tid;
            const uint32_t pw = p0;
            const int t = s0;
            p0 = p1;
            s0 = s1;
            p1 = st.cp_word[cp_off + v + 2 * NT];
            s1 = (int)st.cp_slot[cp_off + v + 2 * NT];
            if (v < cp_surf) {
                const double sv = sc ? sc[t] : 0.0;
                int L, len, A, B, cls, k;
                decode32w(pw, m, L, len, A, B, cls, k);
                double ctr;
                double o = stencil_eval_c<DIM>(W + cls * NDIR, xs, L, len, A, B, ctr);
                if (!wdot) o = sv + o;
                if ((dm >> (cls - 1)) & 1u) o = 0.0;
                if (!FUSED || oc) oc[t] = o;
                if (FUSED) {
                    const int en = cls - 1;
                    const uint32_t word = en < 4 ? mq[0] : en < 8 ? mq[1] : en < 12 ? mq[2] : mq[3];
                    const uint32_t mu = (word >> (8 * (en & 3))) & 0xffu;
                    pap += (double)mu * ((wdot ? fma(wself, ctr, sv) : ctr) * o);
                }
            }
        }
        HMG_SLAB_PHASE(3);                                          // (3: surface entities)
        const int n_int = cp_cnt - cp_surf;
        const int nit_i = (n_int + NT - 1) / NT;
        for (int it = 0; it < nit_i; ++it) {                        // cell interior: one weight row for all nodes
            const int v = it * NT + tid;
            const uint32_t pw = q0;
            const int t = t0;
            q0 = q1;
            t0 = t1;
            q1 = st.cp_word[ib + v + 2 * NT];
            t1 = (int)st.cp_slot[ib + v + 2 * NT];
            if (v < n_int) {
                const double sv = sc ? sc[t] : 0.0;
                int L, len, A, B;
                decode_lattice(pw, m, L, len, A, B);
                double ctr;
                double o = stencil_eval_v<DIM>(w0, xs + L, len, A, B, ctr);
                if (!wdot) o = sv + o;
                if (!FUSED || oc) oc[t] = o;
                if (FUSED) pap += (wdot ? fma(wself, ctr, sv) : ctr) * o;
            }
        }
        lo_prev = lo;
        HMG_SLAB_PHASE(4);                                          // (4: cell interior)
    }
    HMG_SLAB_STORE();
    if (FUSED) {
        __syncthreads();
        const double s_pap = block_sum(pap, smem);
        const double s_rr = block_sum(rr, smem);
        if (tid == 0) {
            a.blockpart[2 * cell] = s_pap;
            a.blockpart[2 * cell + 1] = s_rr;
        }
    }
}

// blockpart[2*c + {0,1}] -> partials[b], partials[2048 + b]  (256 blocks, fixed order: deterministic)
__global__ void __launch_bounds__(256)
k_reduce_pairs(const double *__restrict__ blockpart, int64_t n, double *partials)
{
    __shared__ double red[4];
    double s0 = 0.0, s1 = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) {
        s0 += blockpart[2 * c];
        s1 += blockpart[2 * c + 1];
    }
    const double r0 = block_sum(s0, red);
    const double r1 = block_sum(s1, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = r0;
        partials[2048 + blockIdx.x] = r1;
    }
}

// driver integrals: sum over the first n cells of |J_c| * blockpart[2 c]  (|J| = last term of the cell's coefficients)
__global__ void __launch_bounds__(256)
k_reduce_weighted(const double *__restrict__ blockpart, const double *__restrict__ coef, int jterm, int64_t n, double *partials)
{
    __shared__ double red[4];
    double s0 = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256)
        s0 += blockpart[2 * c] * coef[c * 8 + jterm];
    const double r0 = block_sum(s0, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = r0;
}

size_t apply_lds_bytes(const LevelDev &lv)
{
    return sizeof(double) * (size_t)(WSZ + lv.lds_g0 + lv.nf + lv.lds_g1);
}

static size_t apply_lds_bytes_rb(const LevelDev &lv)   // register-blocked instantiations: only the corners' weight rows in LDS
{
    return sizeof(double) * (size_t)(WSZ_RB + lv.lds_g0 + lv.nf + lv.lds_g1);
}

// ---------------------------------------------------------------------------------------------
// The choice of the kernel, made once: apply_family (which kernel family takes the launch), apply_cell_shape (k_apply's <NT, SPT, RB>
// for the level), apply_cell_role (<CG, RS, WC, LF> for the operands).  launch_apply_dim maps (shape, role) to an instantiation;
// apply_restricts / apply_defers3 / apply_folds_coarse_x, by which the smoothers plan their launches, are questions put to the shape.
// ---------------------------------------------------------------------------------------------
enum class ApplyFamily { wave, small, rows, slab2, slab, cell };

enum { ROLE_WC = 1, ROLE_RS = 2, ROLE_CG = 4, ROLE_ALL = ROLE_WC | ROLE_RS | ROLE_CG };   // (see k_apply's template parameters)

struct CellShape {
    int nt, spt, rb;   // k_apply<DIM, NT, SPT, FUSED, RB, ..>; nt == 0: the cell does not fit the LDS, no k_apply for this level
    size_t lds;        // its dynamic LDS
    int roles;         // the roles this shape has instantiations for
};

struct CellRole {
    bool cg, rs, wc;
    int lf;
};

// A function of the level and the options alone, never of the operands.  wd: the driver-integral instantiations
static CellShape apply_cell_shape(const Launch &L, const LevelDev &lv, bool wd)
{
    const size_t lds = apply_lds_bytes(lv), lds_rb = apply_lds_bytes_rb(lv);
    if (lds > 160 * 1024) return {0, 0, 0, 0, 0};
    const int nf = lv.nf;
    int nt = wd ? 0 : L.apply_threads;   // (the integral instantiations exist for the automatic workgroup sizes only)
    // (small cells are bound by the number of waves launched, not by their work: as few waves per cell as hold it)
    // (level 4, 165 nodes: one wave per cell in three passes beats three waves -- 32 instead of 10 cells in flight per CU,
    //  V-cycle from level 4 down 11.26 -> 10.05 ms)
    if (nt == 0) nt = nf <= 192 ? 64 : nf <= 2048 ? 256 : 1024;
    // the surface layout the register-blocked instantiations are compiled for: one entity class per wave (see the kernel)
    const bool rb_surface = lv.dim == 3 && lv.nei <= 64 && lv.nedge == 6 && lv.ncorner == 4;
    // (level 4, 165 nodes per wave: three slots per lane loaded as batches, not one dependent round trip per slot; WC: the cell's
    //  class table from the class-weight cache)
    if (nt <= 64) return {64, nf > 64 ? 3 : 1, 0, lds, lv.dim == 3 && !wd ? ROLE_WC : 0};
    if (nt <= 192 && nf <= 192) return {192, 1, 0, lds, 0};
    if (nt <= 256 && nf <= 1024) {      // level 5
        if (rb_surface && lv.blk_R == 4 && lv.nblk <= 192 && lv.nfi <= 128) return {256, 4, 4, lds_rb, wd ? 0 : ROLE_RS};
        return {256, 4, 0, lds, 0};
    }
    if (nt <= 256) return {256, 8, 0, lds, 0};
    if (nt <= 512) {                    // (by apply_threads only: no roles)
        if (rb_surface && lv.blk_R == 6 && lv.nblk <= 1024 && lv.nfi <= 512) return {512, 13, 6, lds_rb, 0};
        return {512, 13, 0, lds, 0};
    }
    if (nt <= 640) return {640, 11, 0, lds, 0};
    if (rb_surface && lv.blk_R == 6 && lv.nblk <= 960) {      // level 6
        if (!wd && L.apply_wg512 && lv.nfi <= 512) return {512, 13, 6, lds_rb, ROLE_ALL};
        return {1024, 7, 6, lds_rb, 0};
    }
    return {1024, 7, 0, lds, 0};
}

// the shape the smoothers can plan with: that of the automatic workgroup size (apply_threads is an experiment's option: no folds)
static CellShape planned_cell_shape(const Launch &L, const LevelDev &lv)
{
    return L.apply_threads == 0 ? apply_cell_shape(L, lv, false) : CellShape{0, 0, 0, 0, 0};
}

// CG stages the coarse column in the lattice image in one batch of 13 slots, two coarse slots per thread
static bool stages_coarse_column(const LevelDev &lv)
{
    return lv.par64 && lv.clpos && lv.nf <= 13 * 512 && lv.nf_coarse <= 2 * 512;
}

bool apply_restricts(const Launch &L, const LevelDev &lv)
{
    // level 6's 512-thread shape, or level 5's 256-thread shape (its stand-alone restriction is k_restrict: the epilogue needs that
    // kernel's lists)
    const CellShape s = planned_cell_shape(L, lv);
    return (s.roles & ROLE_RS) && lv.rs_word && lv.rs_w && lv.nf_coarse > 0 && (s.rb == 6 || lv.rs_lp != nullptr);
}

bool apply_defers3(const Launch &L, const LevelDev &lv)
{
    // level 6's 512-thread shape, the whole column in the batched load phase: the only instantiation with the fourth stream
    return apply_restricts(L, lv) && planned_cell_shape(L, lv).rb == 6 && lv.nf <= 13 * 512;
}

bool apply_folds_coarse_x(const Launch &L, const LevelDev &lv)
{
    // the residual with the folded prolongation (flags bit 6) through the 512-thread register-blocked instantiation that stages the
    // coarse column in the lattice image: level 6
    return (planned_cell_shape(L, lv).roles & ROLE_CG) && stages_coarse_column(lv) && lv.nf_coarse > 0;
}

// can this launch take its class weights from the class-weight cache?  (formed for |alpha| = 1, the grid's lambda, the full operator)
static bool weight_cache_ok(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a)
{
    return L.weight_cache && lv.wcache && mesh.cell_class && lv.dim == 3 && lv.ncls == 15 && !(a.flags & (2 | 8 | 16)) &&
           (a.alpha == 1.0 || a.alpha == -1.0) && a.lambda == mesh.wc_lambda;
}

bool apply_carries_x(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double lambda, int updates)
{
    // the stored first residual r = b - A x with x's last two or three CG updates in its load phase: level 6's 512-thread shape, the
    // whole column in the batched load phase; three updates through the one instantiation with the fourth stream (class weights
    // from the cache)
    const CellShape s = planned_cell_shape(L, lv);
    if (s.roles != ROLE_ALL || s.rb != 6 || lv.nf > 13 * 512 || L.slab2_force) return false;
    if (updates < 3) return true;
    ApplyArgs a{};
    a.alpha = -1.0;
    a.lambda = lambda;
    a.flags = 1;
    return weight_cache_ok(L, lv, mesh, a);
}

static CellRole apply_cell_role(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a, const CellShape &s,
                                bool fused)
{
    CellRole r{};
    // (CG, own instantiation: the in-image staging of the coarse column costs the others registers; it handles the residual of the
    //  coarse-grid correction only -- no pending CG updates -- and one batch of 13 slots.  RS: own instantiation again)
    r.cg = fused && (s.roles & ROLE_CG) && a.xcoarse && (a.flags & 64) && !a.x2 && !a.xacc && !a.x3 && stages_coarse_column(lv);
    r.rs = fused && (s.roles & ROLE_RS) && !r.cg && a.rcoarse && lv.rs_word && lv.rs_w && !a.xcoarse;
    r.wc = (s.roles & ROLE_WC) && weight_cache_ok(L, lv, mesh, a);      // class weights from the cache, else combined per cell
    if (!fused || s.roles != ROLE_ALL) return r;
    if (r.cg)
        r.lf = a.xc_p ? 5 : 0;
    else if (r.rs)
        r.lf = a.x4 ? 4 : 0;
    else if (a.x4)
        r.lf = 4;                  // (the carrying first residual: launch_apply_dim has checked its operands and the cache)
    else if (r.wc && !a.xacc && !a.x3 && !a.xcoarse && !a.rcoarse)
        // CG step 0; a dead step, or one that writes its direction elsewhere (no store may sit between the loads of a stream it aliases)
        r.lf = !a.x2 ? 1 : !a.xout || a.xout != a.x2 ? 2 : 0;
    return r;
}

static ApplyFamily apply_family(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a, const CellShape &s,
                                bool fused, bool wd)
{
    const bool plain3 = lv.dim == 3 && !wd;
    // level 5: one wave per cell, class weights from the cache (hmg_apply_wave.hip)
    if (plain3 && apply_wave_ok(L, lv, mesh, a, fused)) return ApplyFamily::wave;
    // levels 2-4: one persistent, software-pipelined wave per cell (hmg_apply_small.hip)
    if (plain3 && apply_small_ok(L, lv, mesh, a, fused)) return ApplyFamily::small;
    // 2D levels 9..11: the cell walks through LDS in bands of lattice rows (hmg_apply_rows.hip)
    if (lv.dim == 2 && s.nt == 0) return ApplyFamily::rows;
    // (experiment of round 5, option slab2_force + HMG_SLAB_LDS_KB <= 30: level 6 through the role-split window kernel of level 7 --
    //  VERDICT r4 item 4's "cell as two half-images, the second half's loads in flight while the first is evaluated")
    const bool force_slab2 = plain3 && L.slab2_force && mesh.slab.head && mesh.slab.nslab >= 2 && lv.nf > 2048 && !a.xcoarse &&
                             !a.rcoarse && !(a.flags & (4 | 8));
    if (s.nt != 0 && !force_slab2) return ApplyFamily::cell;
    if (lv.dim != 3 || !mesh.slab.head) throw std::runtime_error("operator apply: cell does not fit the LDS");
    return plain3 && apply_slab2_ok(L, lv, mesh, a) ? ApplyFamily::slab2 : ApplyFamily::slab;
}

static void check_apply_cell(const ApplyArgs &a, const MeshDev &mesh, bool fused)
{
    check_apply_bases(a, mesh, fused, true);
    check_apply_transfers(a);
    check_apply_zero_input(a, fused);
}

template <int DIM, int NT, int SPT, bool FUSED, int RB, bool WD, bool CG, bool RS, bool WC, int LF>
static void launch_apply_generic(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a, size_t lds)
{
    auto kern = k_apply<DIM, NT, SPT, FUSED, RB, WD, CG, RS, WC, LF>;
    if (a.rcoarse && !RS) throw std::runtime_error("operator apply: this instantiation cannot restrict in its epilogue");
    if (a.xc_p && !(CG && LF == 5)) throw std::runtime_error("operator apply: this instantiation cannot finish the coarse x");
    if (a.x4 && LF != 4) throw std::runtime_error("operator apply: this instantiation cannot carry a third pending x-update");
    if ((a.flags & 128) && !(FUSED && (RS || RB == 0)))
        throw std::runtime_error("operator apply: this instantiation cannot take a zero input that is not in memory");
    if (FUSED && a.xcoarse && !CG) lds += sizeof(double) * (size_t)lv.nf_coarse;   // coarse column behind the lattice image
    if (lds > 48 * 1024)
        HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t nblocks = apply_work_items(a, mesh);
    if (nblocks == 0) return;
    check_apply_cell(a, mesh, FUSED);
    if (WC && !weight_cache_ok(L, lv, mesh, a)) throw std::runtime_error("operator apply: class-weight cache not usable for this launch");
    ApplyArgs b = apply_work_args(L, mesh, a, nblocks, RB != 0);
    b.cell_class = WC ? mesh.cell_class : nullptr;
    // (NT == 64: persistent one-wave workgroups, see the kernel -- 32 waves per CU are resident)
    const int64_t grid = NT == 64 ? std::min<int64_t>(nblocks, 32 * (int64_t)L.num_cu) : nblocks;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), lds, L.stream, lv, mesh.coef, mesh.dmask, b);
    check_launch();
    if (WC && L.n_wc_launches) *L.n_wc_launches += 1;
}

// 3D cells larger than the LDS, the forms k_apply_slab2 does not have: slabs of k-planes through a rolling window
template <bool FUSED, bool WD>
static void launch_apply_slab(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a)
{
    auto kern = k_apply_slab<3, 1024, FUSED, WD>;
    const size_t bytes = sizeof(double) * (size_t)(WSZ + mesh.slab.lds_nodes);
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    const int64_t nblocks = apply_work_items(a, mesh);
    if (nblocks == 0) return;
    check_apply_cell(a, mesh, FUSED);
    const ApplyArgs b = apply_work_args(L, mesh, a, nblocks, true);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(1024), bytes, L.stream, lv, mesh.coef, mesh.dmask, b, mesh.slab);
    check_launch();
}

constexpr uint32_t cell_key(int nt, int spt, int rb, bool cg, bool rs, bool wc, int lf)
{
    return (uint32_t)nt | (uint32_t)spt << 11 | (uint32_t)rb << 15 | (uint32_t)cg << 18 | (uint32_t)rs << 19 | (uint32_t)wc << 20 |
           (uint32_t)lf << 21;
}

template <int DIM, bool FUSED, bool WD = false>
static void launch_apply_dim(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a)
{
    // a third pending x-update: the register-blocked residuals of level 6 alone have the stream (no other family is reached with it) --
    // the local residual that restricts in its epilogue, and the stored first residual with its class weights from the cache
    if (a.x4 && !(FUSED && DIM == 3 && !WD && a.x3 && a.x2 && a.xout && !a.xcoarse && !a.xacc && !(a.flags & 128) &&
                  (a.rcoarse ? apply_defers3(L, lv) : a.src && a.out && apply_carries_x(L, lv, mesh, a.lambda, 3))))
        throw std::runtime_error("operator apply: a third pending x-update (x4) where no kernel carries it");
    // the coarse x with its last two updates pending: the in-image prolongation of level 6 alone combines the three coarse columns
    if ((a.xc_p || a.xc_r) && !(FUSED && DIM == 3 && !WD && a.xc_p && a.xc_r && a.xcoarse && (a.flags & 64) && !a.x2 && !a.xacc && !a.x3 &&
                                !a.rcoarse && apply_folds_coarse_x(L, lv)))
        throw std::runtime_error("operator apply: pending coarse x-updates (xc_p, xc_r) where no kernel carries them");
    const CellShape s = apply_cell_shape(L, lv, WD);
    switch (apply_family(L, lv, mesh, a, s, FUSED, WD)) {
    case ApplyFamily::wave: return launch_apply_wave(L, lv, mesh, a, FUSED);
    case ApplyFamily::small: return launch_apply_small(L, lv, mesh, a, FUSED);
    case ApplyFamily::rows: return launch_apply_rows(L, lv, mesh, a, FUSED, WD);
    case ApplyFamily::slab2: return launch_apply_slab2(L, lv, mesh, a, FUSED);
    case ApplyFamily::slab: return launch_apply_slab<FUSED, WD>(L, lv, mesh, a);
    case ApplyFamily::cell: break;
    }
    const CellRole r = apply_cell_role(L, lv, mesh, a, s, FUSED);
    const uint32_t key = cell_key(s.nt, s.spt, s.rb, r.cg, r.rs, r.wc, r.lf);
    // Every k_apply there is, one row each: no other combination is compiled.  HAVE: the (DIM, FUSED, WD) that have the row
    constexpr bool D3 = DIM == 3, R3 = D3 && !WD, RF = R3 && FUSED;
#define HMG_CELL(HAVE, NT, SPT, RB, CG, RS, WC, LF)                 \
    if constexpr (HAVE)                                             \
        if (key == cell_key(NT, SPT, RB, CG, RS, WC, LF))           \
            return launch_apply_generic<DIM, NT, SPT, FUSED, RB, WD, CG, RS, WC, LF>(L, lv, mesh, a, s.lds)
    //       HAVE   NT  SPT RB   CG     RS     WC    LF
    HMG_CELL(true,   64,  1, 0, false, false, false, 0);
    HMG_CELL(true,   64,  3, 0, false, false, false, 0);
    HMG_CELL(true,  192,  1, 0, false, false, false, 0);
    HMG_CELL(true,  256,  4, 0, false, false, false, 0);
    HMG_CELL(true,  256,  8, 0, false, false, false, 0);
    HMG_CELL(!WD,   512, 13, 0, false, false, false, 0);
    HMG_CELL(!WD,   640, 11, 0, false, false, false, 0);
    HMG_CELL(true, 1024,  7, 0, false, false, false, 0);
    HMG_CELL(D3,    256,  4, 4, false, false, false, 0);
    HMG_CELL(D3,   1024,  7, 6, false, false, false, 0);
    HMG_CELL(R3,     64,  1, 0, false, false, true,  0);
    HMG_CELL(R3,     64,  3, 0, false, false, true,  0);
    HMG_CELL(RF,    256,  4, 4, false, true,  false, 0);
    HMG_CELL(R3,    512, 13, 6, false, false, false, 0);
    HMG_CELL(R3,    512, 13, 6, false, false, true,  0);
    HMG_CELL(RF,    512, 13, 6, false, false, true,  1);
    HMG_CELL(RF,    512, 13, 6, false, false, true,  2);
    HMG_CELL(RF,    512, 13, 6, false, false, true,  4);
    HMG_CELL(RF,    512, 13, 6, false, true,  false, 0);
    HMG_CELL(RF,    512, 13, 6, false, true,  false, 4);
    HMG_CELL(RF,    512, 13, 6, false, true,  true,  0);
    HMG_CELL(RF,    512, 13, 6, false, true,  true,  4);
    HMG_CELL(RF,    512, 13, 6, true,  false, false, 0);
    HMG_CELL(RF,    512, 13, 6, true,  false, false, 5);
    HMG_CELL(RF,    512, 13, 6, true,  false, true,  0);
    HMG_CELL(RF,    512, 13, 6, true,  false, true,  5);
#undef HMG_CELL
    throw std::runtime_error("operator apply: no instantiation for this shape and role");
}

void launch_apply(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double alpha, double lambda,
                  const double *x, const double *src, double *out, int use_mask)
{
    ApplyArgs a{};
    a.alpha = alpha;
    a.lambda = lambda;
    a.x = x;
    a.src = src;
    a.out = out;
    a.flags = (use_mask ? 1 : 0) | (L.apply_mass_only ? 2 : 0);
#ifdef HMG_PHASE_TIMING
    a.blockpart = mesh.blockpart;
#endif
    if (lv.dim == 3)
        launch_apply_dim<3, false>(L, lv, mesh, a);
    else
        launch_apply_dim<2, false>(L, lv, mesh, a);
}

void launch_apply_args(const Launch &L, const LevelDev &lv, const MeshDev &mesh, ApplyArgs a)
{
    a.flags = (a.flags & 1) | (L.apply_mass_only ? 2 : 0);
    if (lv.dim == 3)
        launch_apply_dim<3, false>(L, lv, mesh, a);
    else
        launch_apply_dim<2, false>(L, lv, mesh, a);
}

void launch_apply_fused_kernel(const Launch &L, const LevelDev &lv, const MeshDev &mesh, ApplyArgs a)
{
    if (!a.scal) a.scal = L.scal;                // (a caller's own scalars: the rebuilt Ap of a pending r-update, materialize_r())
    if (!(a.flags & 32)) a.mult = mesh.mult;     // (bit 5: caller wants unit multiplicities -- a.mult stays null)
    a.blockpart = mesh.blockpart;
    if (a.flags & 8) {                            // the driver integrals: src multiplies (own instantiations)
        if (lv.dim == 3)
            launch_apply_dim<3, true, true>(L, lv, mesh, a);
        else
            launch_apply_dim<2, true, true>(L, lv, mesh, a);
        return;
    }
    if (lv.dim == 3)
        launch_apply_dim<3, true>(L, lv, mesh, a);
    else
        launch_apply_dim<2, true>(L, lv, mesh, a);
}

void launch_apply_fused_reduce(const Launch &L, const MeshDev &mesh, int slot_pap, int slot_rr)
{
    hipLaunchKernelGGL(k_reduce_pairs, dim3(256), dim3(256), 0, L.stream, mesh.blockpart, mesh.ncells, L.partials);
    check_launch();
    launch_finalize(L, L.partials, 256, slot_pap);
    if (slot_rr >= 0)
        launch_finalize(L, L.partials + 2048, 256, slot_rr);
    check_launch();
}

// Restriction of a level whose cell exceeds the LDS: b_coarse[c] = r[c] + 0.5 * sum of r over the fine lattice
// neighbours of c that exist in the cell -- a cell-independent 15-point stencil evaluated at the even fine nodes,
// run through k_apply_slab's rolling window (fine.ctab -> restriction weights, st -> lists of the even nodes with
// their COARSE storage slots).
void launch_restrict_slab(const Launch &L, const LevelDev &fine_rtab, const MeshDev &mesh, const SlabTables &st,
                          int ldc, const double *rf, double *bc)
{
    ApplyArgs a{};
    a.alpha = 1.0;
    a.x = rf;
    a.out = bc;
    a.out_ld = ldc;
    a.flags = 4;
    {   // round 5: through the role-split window kernel with EIGHT loader waves -- an eighth of the nodes is evaluated (the even ones), so
        // the loaders set the pace (option restrict_slab2 = 0: k_apply_slab as in rounds 1-4; the coarse vector is the same to the last bit)
        MeshDev m2 = mesh;
        m2.slab = st;
        if (L.restrict_slab2 && apply_slab2_ok(L, fine_rtab, m2, a)) {
            launch_apply_slab2(L, fine_rtab, m2, a, false);
            return;
        }
    }
    auto kern = k_apply_slab<3, 1024, false>;
    const size_t bytes = sizeof(double) * (size_t)(WSZ + st.lds_nodes);
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)mesh.ncells), dim3(1024), bytes, L.stream, fine_rtab, mesh.coef, mesh.dmask, a, st);
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// driver integrals over a prefix of cells (ref: src/examples/homogenized_coefficients.jl:592-667)
//   mode 0: sum_cells |J| sum_i v_i (b_i + (M v)_i), b = dphi . P = the right-hand side of outer step 0   integrate_first_term
//   mode 1: sum_cells |J| sum_i (v_i + w_i) (M v)_i                                                        integrate_terms
//   mode 3: sum_cells |J| sum_i w_i (M v)_i                      the bilinear form of two correctors (w may be v)
// M = reference-element mass matrix of the level.  One pass of the FUSED operator apply in "reductions only" form
// (no output vector): mass term only and unscaled, unit multiplicities, no constraint; the per-cell sum it leaves
// in blockpart is sum_i x_i (src_i + (M x)_i), sum_i (x_i + src_i) (M x)_i resp. sum_i src_i (M x)_i, scaled by |J_c| in the reduction.
// Works for every level the apply works for (the slab kernel included) and moves 16 B per DOF.
// ---------------------------------------------------------------------------------------------
void launch_integrate(const Launch &L, const LevelDev &lv, const MeshDev &mesh, int mode, int64_t nsub, const double *v,
                      const double *second, int slot)
{
    ApplyArgs a{};
    a.alpha = 1.0;
    a.lambda = 1.0;
    a.x = v;
    a.src = second;
    a.flags = 2 | 16 | 32 | (mode == 1 ? 8 : mode == 3 ? 8 | 256 : 0);
    a.ncells_prefix = nsub;
    launch_apply_fused_kernel(L, lv, mesh, a);
    hipLaunchKernelGGL(k_reduce_weighted, dim3(256), dim3(256), 0, L.stream, mesh.blockpart, mesh.coef, lv.nterm - 1, nsub,
                       L.partials);
    launch_finalize(L, L.partials, 256, slot);
    check_launch();
}

}  // namespace hmg
