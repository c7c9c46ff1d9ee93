// 2D cells larger than the LDS (levels 9..11: 33 153 .. 525 825 nodes per cell, 265 KB .. 4.2 MB per column): operator apply,
// prolongation and the unique-copy norm on levels that have no packed addressing words (build_level_tables).
//
// Row-band apply (k_apply_rows): the 2D counterpart of k_apply_slab (hmg_apply.hip) with lattice rows in place of k-planes.  In
// 2D the lattice image is L(i,j) = RO(j) + i, RO(j) = j (m+1) - j (j-1) / 2, row j holds m+1-j nodes, and the 7-point stencil
// reaches the rows j-1 and j+1 only.  One workgroup per cell walks the cell in bands of rows [j0, j1) through a ROLLING window: the
// LDS holds rows [j0-1, j1] (+ a zero guard), the nodes of rows [j0, j1) are evaluated, rows j1-1 and j1 move to the front of the
// window (LDS -> LDS) and only rows j1+1 .. come from HBM.  Every slot is read from HBM once per apply and every output is written
// once, so the load-phase side effects of the fused CG pass (p-update, pending x-updates, r.r) ride in the loads as in k_apply.
// No per-level tables: a node's storage slot and entity class follow from (i,j) (rows_slot, checked against the host tables by
// upload_levels).  Same arithmetic per node as k_apply / k_apply_slab (stencil_eval_c for surface nodes, stencil_eval_v with the
// interior weight row for the rest).
#include "hmg_apply_launch.hpp"
#include "hmg_device.hpp"
#include "hmg_rows_window.hpp"
#include "hmg_stencil.hpp"

#include <stdexcept>

namespace hmg {

namespace {

// the row-band form of every launch (class weights combined per cell; flags bit 2 -- restriction weights -- is refused by the launcher)
template <bool FUSED, bool WD>
__global__ void __launch_bounds__(RW_NT, 8)
k_apply_rows(LevelDev lv, const double *__restrict__ coef, const uint16_t *__restrict__ dmask, ApplyArgs a)
{
    constexpr int NDIR = 7;
    constexpr int NTERM = 4;
    constexpr int NT = RW_NT;
    constexpr int HB = FUSED ? 2 : 4;               // loads in flight per thread and stream in the load phase (64-VGPR budget: 3 in flight spilled 8 B)
    constexpr int EB = 2;                           // evaluated nodes per thread and trip: their src loads in flight together
    extern __shared__ double smem[];
    double *W = smem;
    double *img = smem + WSZ;                       // RW_WIN doubles: [rows j0-1 .. j1 | zero guard]
    const int tid = threadIdx.x;
    const int64_t cell = a.cell_list ? (int64_t)a.cell_list[blockIdx.x] : (int64_t)blockIdx.x;
    const int m = lv.m, nei = lv.nei, off_int = lv.off_int;

    {
        double s[NTERM];
        cell_scales<2>(coef + cell * 8, a.alpha, a.lambda, s, a.flags);
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
    const bool xzero = FUSED && (a.flags & 128);                          // x is zero and is not read (x3 form only)
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
    __syncthreads();                                                // W complete
    double w0[NDIR];                                                // interior weight row, SGPR-resident
#pragma unroll
    for (int d = 0; d < NDIR; ++d) w0[d] = to_sgpr(W[d]);

    int lo_prev = 0;
    for (int j0 = 0, j1 = 0; j0 <= m; j0 = j1) {
        j1 = rows_band_end(m, j0);
        const int lo = rows_ro(m, j0 - 1);                          // lattice range held in LDS: [lo, hi) + guard
        const int hi = rows_ro(m, j1 + 1);
        double *xs = img - lo;                                      // xs[L] valid inside that range
        int ld_first = 0;                                           // first lattice position that comes from HBM
        if (j0 > 0) {
            __syncthreads();                                        // previous band fully consumed
            // rows j0-1 and j0 (the last evaluated row and the upper halo of the previous band) move to the front of the window:
            // every thread takes its share into registers, one barrier, then writes (the ranges may overlap)
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
        // rows new in the window: HBM -> LDS, every slot once; batches of HB slots per thread, all loads of a batch before its
        // stores (xout / xacc may alias x2)
        const int ld_cnt = hi - ld_first;
        for (int q0 = 0; q0 < ld_cnt; q0 += HB * NT) {
            int tt[HB];
            double xv[HB], x2v[HB], xav[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int v = q0 + q * NT + tid;
                tt[q] = -1;
                if (v < ld_cnt) {
                    const int L = ld_first + v, j = rows_row_of(m, L), i = L - rows_ro(m, j);
                    int cls;
                    tt[q] = rows_slot(m, i, j, nei, off_int, cls);
                }
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int t = tt[q];
                if (t >= 0) {
                    xv[q] = xzero ? 0.0 : xc[t];
                    x2v[q] = x2c ? x2c[t] : 0.0;
                    xav[q] = xac ? xac[t] : x3c ? x3c[t] : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int t = tt[q];
                if (t >= 0) {
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
                    img[ld_first - lo + q0 + q * NT + tid] = val;
                }
            }
        }
        __syncthreads();
        // rows [j0, j1): EB nodes per thread and trip, their src loads issued together
        const int e0 = rows_ro(m, j0), ecnt = rows_ro(m, j1) - e0;
        for (int q0 = 0; q0 < ecnt; q0 += EB * NT) {
            int tt[EB], LL[EB], cl[EB], ln[EB];
            double sv[EB];
#pragma unroll
            for (int q = 0; q < EB; ++q) {
                const int v = q0 + q * NT + tid;
                tt[q] = -1;
                LL[q] = 0;
                cl[q] = 0;
                ln[q] = 1;
                if (v < ecnt) {
                    LL[q] = e0 + v;
                    const int j = rows_row_of(m, LL[q]), i = LL[q] - rows_ro(m, j);
                    ln[q] = m + 1 - j;
                    tt[q] = rows_slot(m, i, j, nei, off_int, cl[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < EB; ++q) sv[q] = sc && tt[q] >= 0 ? sc[tt[q]] : 0.0;
#pragma unroll
            for (int q = 0; q < EB; ++q) {
                const int t = tt[q];
                if (t < 0) continue;
                const int L = LL[q], cls = cl[q], len = ln[q];
                double ctr, o;
                if (cls == 0) {
                    o = stencil_eval_v<2>(w0, xs + L, len, 0, 0, ctr);
                    if (!wdot) o = sv[q] + o;
                    if (!FUSED || oc) oc[t] = o;
                    if (FUSED) pap += (wdot ? fma(wself, ctr, sv[q]) : ctr) * o;
                } else {
                    o = stencil_eval_c<2>(W + cls * NDIR, xs, L, len, 0, 0, ctr);
                    if (!wdot) o = sv[q] + o;
                    if ((dm >> (cls - 1)) & 1u) o = 0.0;
                    if (!FUSED || oc) oc[t] = o;
                    if (FUSED) {
                        const int en = cls - 1;
                        const uint32_t word = en < 4 ? mq[0] : en < 8 ? mq[1] : en < 12 ? mq[2] : mq[3];
                        const uint32_t mu = (word >> (8 * (en & 3))) & 0xffu;
                        pap += (double)mu * ((wdot ? fma(wself, ctr, sv[q]) : ctr) * o);
                    }
                }
            }
        }
        lo_prev = lo;
    }
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

// Prolongation of a coarse cell larger than the LDS (interpolate_and_sum_to!, src/interpolation.jl:64-74): the coarse column is
// gathered through L2 instead of staged -- the fine slots of a workgroup are consecutive, and consecutive fine slots (lattice order
// inside every entity) have their parents in one or two neighbouring coarse rows, so every coarse value comes from HBM about once
// per cell.  32-bit parents (par_a / par_b), the roundings of k_prolong_add: identity rows += 1.0 c[a], midpoints += 0.5 c[a]
// (the parent with the smaller hierarchical id) then += 0.5 c[b].
constexpr int PW_NT = 256, PW_SPT = 4;

__global__ void __launch_bounds__(PW_NT)
k_prolong_add_wide(LevelDev fine, int64_t nchunk, int ldc, const double *__restrict__ xc, double *xf)
{
    const int64_t cell = (int64_t)blockIdx.x / nchunk;
    const int t0 = (int)((int64_t)blockIdx.x - cell * nchunk) * (PW_NT * PW_SPT) + threadIdx.x;
    const double *c = xc + cell * ldc;
    double *f = xf + cell * fine.ld;
    double y[PW_SPT];
    int pa[PW_SPT], pb[PW_SPT];
#pragma unroll
    for (int q = 0; q < PW_SPT; ++q) {
        const int t = t0 + q * PW_NT;
        if (t < fine.nf) {
            y[q] = f[t];
            pa[q] = fine.par_a[t];
            pb[q] = fine.par_b[t];
        }
    }
    double ca[PW_SPT], cb[PW_SPT];
#pragma unroll
    for (int q = 0; q < PW_SPT; ++q) {
        const int t = t0 + q * PW_NT;
        if (t < fine.nf) {
            ca[q] = c[pa[q]];
            cb[q] = c[pb[q]];
        }
    }
#pragma unroll
    for (int q = 0; q < PW_SPT; ++q) {
        const int t = t0 + q * PW_NT;
        if (t < fine.nf) {
            double r = y[q];
            if (pa[q] == pb[q])
                r += 1.0 * ca[q];
            else {
                r += 0.5 * ca[q];   // CSC column order: parent with the smaller hierarchical id first
                r += 0.5 * cb[q];
            }
            f[t] = r;
        }
    }
}

// k_norm2_unique where the level has no packed words: the entity class of a slot follows from the segment it lies in
__global__ void __launch_bounds__(256)
k_norm2_unique_wide(LevelDev lv, int64_t ncells, const uint16_t *__restrict__ dupmask, const double *__restrict__ x,
                    double *partials)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const uint32_t dm = dupmask[cell];
        const double *xc = x + cell * lv.ld;
        for (int t = threadIdx.x; t < lv.nf; t += 256) {
            const int cls = t < lv.ncorner   ? 1 + lv.nface + lv.nedge + t
                            : t < lv.off_face ? 1 + lv.nface + (t - lv.off_edge) / lv.nei
                            : t < lv.off_int  ? 1 + (t - lv.off_face) / lv.nfi
                                              : 0;
            const bool dup = cls > 0 && ((dm >> (cls - 1)) & 1u);
            const double v = xc[t];
            if (!dup) acc += v * v;
        }
    }
    double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <bool FUSED, bool WD>
void launch_rows(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a, int64_t nblocks)
{
    auto kern = k_apply_rows<FUSED, WD>;
    const size_t bytes = sizeof(double) * (size_t)(WSZ + RW_WIN);
    HMG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(RW_NT), bytes, L.stream, lv, mesh.coef, mesh.dmask, a);
    check_launch();
}

}  // namespace

void launch_apply_rows(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const ApplyArgs &a, bool fused, bool wd)
{
    if (lv.dim != 2 || lv.ncls != 7 || lv.ndir != 7 || lv.nterm != 4 || lv.ncorner != 3 || lv.nedge != 3 || lv.nface != 0)
        throw std::runtime_error("operator apply (row bands): not a 2D level");
    if (lv.m < 2 || lv.m > 1024 || lv.nei != lv.m - 1 || lv.off_int != 3 + 3 * lv.nei || lv.nf != rows_ro(lv.m, lv.m + 1))
        throw std::runtime_error("operator apply (row bands): level layout out of range");
    // the window of the widest band (rows 0..2 at least) plus the guard must fit, and the move of two rows must fit RW_MV per thread
    if (rows_ro(lv.m, 3) + RW_GUARD > RW_WIN || 2 * (lv.m + 1) > RW_MV * RW_NT || lv.ncls * lv.ndir > WSZ)
        throw std::runtime_error("operator apply (row bands): a band of rows does not fit the window");
    check_apply_bases(a, mesh, fused, true);
    if (a.xcoarse || a.rcoarse) throw std::runtime_error("operator apply (row bands): no level transfer is folded into this kernel");
    if (a.flags & (4 | 64)) throw std::runtime_error("operator apply (row bands): restriction weights / in-image prolongation are not supported");
    if ((a.flags & 8) && !(fused && wd)) throw std::runtime_error("operator apply (row bands): the driver-integral form needs its instantiation");
    check_apply_pending(a, fused);
    check_apply_zero_input(a, fused);
    const int64_t nblocks = apply_work_items(a, mesh);
    if (nblocks == 0) return;
    if (nblocks > 0x7fffffffLL) throw std::runtime_error("operator apply (row bands): too many cells for one launch");
    if (L.n_rows_launches) *L.n_rows_launches += 1;
    const ApplyArgs b = apply_work_args(L, mesh, a, nblocks, false);   // (cells in storage order)
    if (!fused)
        launch_rows<false, false>(L, lv, mesh, b, nblocks);
    else if (wd)
        launch_rows<true, true>(L, lv, mesh, b, nblocks);
    else
        launch_rows<true, false>(L, lv, mesh, b, nblocks);
}

void launch_prolong_add_wide(const Launch &L, const LevelDev &fine, const LevelDev &coarse, int64_t ncells, const double *xc,
                             double *xf)
{
    if (!fine.par_a || !fine.par_b) throw std::runtime_error("prolongation: no parent tables on this level");
    if (fine.nf_coarse != coarse.nf) throw std::runtime_error("prolongation: levels do not match");
    if (ncells == 0) return;
    const int64_t nchunk = (fine.nf + PW_NT * PW_SPT - 1) / (PW_NT * PW_SPT);
    const int64_t blocks = nchunk * ncells;
    if (blocks > 0x7fffffffLL) throw std::runtime_error("prolongation: too many cells for one launch");
    hipLaunchKernelGGL(k_prolong_add_wide, dim3((unsigned)blocks), dim3(PW_NT), 0, L.stream, fine, nchunk, coarse.ld, xc, xf);
    check_launch();
}

int64_t launch_norm2_unique_wide(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const double *x)
{
    int64_t nb = mesh.ncells;
    if (nb > (int64_t)L.num_cu * 8) nb = (int64_t)L.num_cu * 8;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(k_norm2_unique_wide, dim3((unsigned)nb), dim3(256), 0, L.stream, lv, mesh.ncells, mesh.dupmask, x, L.partials);
    check_launch();
    return nb;
}

}  // namespace hmg
