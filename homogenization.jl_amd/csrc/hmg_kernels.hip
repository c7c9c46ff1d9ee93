// HIP kernels for gfx950 (MI355X) around the operator apply (which lives in hmg_apply.hip and the hmg_apply_*.hip families):
// interface sum, Dirichlet / duplicate masks, level transfer, fused CG vector kernels, level-1 gather/scatter and
// a (Chebyshev-)preconditioned CG for the coarse system.  Wave = 64 lanes everywhere.
//
// Reference behaviour reproduced (file:line in the reference checkout):
//   k_iface_*           src/implicit_fine_grid.jl:209-328   (copies summed in ascending cell order)
//   k_mask              src/implicit_fine_grid.jl:94-139 / :334-386
//   k_restrict/prolong  src/interpolation.jl:52-74
//   k_cg_*, k_dot*      src/multigrid.jl:46-71
//   k_gather/scatter    src/implicit_fine_grid.jl:148-202
#include "hmg_device.hpp"
#include "hmg_stencil.hpp"

#include <cstdio>
#include <stdexcept>
#include <string>

namespace hmg {

__global__ void __launch_bounds__(256) k_finalize(const double *__restrict__ partials, int n, double *scal, int slot)
{
    __shared__ double red[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += partials[i];
    double s = block_sum(v, red);
    if (threadIdx.x == 0) scal[slot] = s;
}

void launch_finalize(const Launch &L, const double *partials, int n, int slot)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, L.stream, partials, n, L.scal, slot);
}

// ---------------------------------------------------------------------------------------------
// interface sum: every shared entity is one contiguous, identically ordered run in each copy
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_iface_faces(const int32_t *__restrict__ pairs, int64_t npairs, int nfi, int off_face, int ld, double *x)
{
    // one wave per shared face; all loads of (up to) 8 x 64 DOFs of both copies in flight before the first store
    constexpr int U = 8;
    const int lane = threadIdx.x & 63;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < npairs; p += nw) {
        const int32_t ca = pairs[3 * p], cb = pairs[3 * p + 1], lf = pairs[3 * p + 2];
        double *a = x + (int64_t)ca * ld + off_face + (lf & 15) * nfi;
        double *b = x + (int64_t)cb * ld + off_face + (lf >> 4) * nfi;
        for (int k0 = 0; k0 < nfi; k0 += U * 64) {
            double va[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * 64 + lane;
                if (k < nfi) {
                    va[u] = a[k];
                    vb[u] = b[k];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * 64 + lane;
                if (k < nfi) {
                    const double s = va[u] + vb[u];   // (0 + a) + b, ascending cell order
                    a[k] = s;
                    b[k] = s;
                }
            }
        }
    }
}

// CSR entities in one launch: shared edges (nei values at offset off_edge + lid*nei) followed by shared nodes (one
// value at offset lid).  Copies are summed in list order (ascending cell, the reference's order).
__global__ void __launch_bounds__(256)
k_iface_csr(const int32_t *__restrict__ eptr, const int32_t *__restrict__ eent, int64_t nedge, int nei, int off_edge,
            const int32_t *__restrict__ nptr, const int32_t *__restrict__ nent, int64_t nnode, int ld, double *x)
{
    // Copies are read in batches of U: all entries of a batch first, then all values (independent loads in flight together
    // instead of one dependent entry -> value round trip per copy: a shared edge of the Kuhn lattice has 4 or 6 copies, a
    // node 24), summed in list order as before.
    constexpr int U = 8;
    const int64_t tedge = nedge * nei, total = tedge + nnode;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const bool is_edge = idx < tedge;
        const int64_t e = is_edge ? idx / nei : idx - tedge;
        const int k = is_edge ? (int)(idx - e * nei) : 0;
        const int per = is_edge ? nei : 1, off = is_edge ? off_edge : 0;
        const int32_t *ptr = is_edge ? eptr : nptr, *ent = is_edge ? eent : nent;
        const int b = ptr[e], end = ptr[e + 1];
        double s = 0.0;
        if (end - b <= U) {
            // one batch (a shared edge has 4-6 copies): the entries stay in registers for the stores -- the general path below reads
            // them a second time, one more dependent round trip per entity (round 4)
            int32_t v[U];
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = b + u < end ? ent[b + u] : -1;
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = v[u] >= 0 ? x[(int64_t)(v[u] >> 3) * ld + off + (v[u] & 7) * per + k] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v[u] >= 0) s += xv[u];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v[u] >= 0) x[(int64_t)(v[u] >> 3) * ld + off + (v[u] & 7) * per + k] = s;
            continue;
        }
        for (int q0 = b; q0 < end; q0 += U) {
            int32_t v[U];
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = q0 + u < end ? ent[q0 + u] : -1;
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = v[u] >= 0 ? x[(int64_t)(v[u] >> 3) * ld + off + (v[u] & 7) * per + k] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v[u] >= 0) s += xv[u];
        }
        for (int q0 = b; q0 < end; q0 += U) {
            int32_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = q0 + u < end ? ent[q0 + u] : -1;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v[u] >= 0) x[(int64_t)(v[u] >> 3) * ld + off + (v[u] & 7) * per + k] = s;
        }
    }
}

void launch_interface_sum(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double *x, int which, bool faces)
{
    const int cap = L.num_cu * 8;
    if (lv.dim == 3 && lv.nfi > 0 && mesh.nfacepairs > 0) {
        // pairs [0, ncut) count as cut (rehearsal partitions): summed with the cut groups, whatever `faces` says
        const int64_t ncut = mesh.ncut_face_pairs;
        const int64_t first = which == 2 ? ncut : 0;
        const int64_t last = which == 1 || !faces ? ncut : mesh.nfacepairs;
        const int64_t np = last - first;
        if (np > 0) {
            const int64_t blocks = (np + 3) / 4;              // one wave per pair, blocks dispatched in pair order
            hipLaunchKernelGGL(k_iface_faces, dim3((unsigned)blocks), dim3(256), 0, L.stream, mesh.face_pairs + 3 * first, np,
                               lv.nfi, lv.off_face, lv.ld, x);
            check_launch();
        }
    }
    // group ranges of the CSR lists: [0, ncut) are cut by the partition, [ncut, n) are not
    auto range = [&](int64_t n, int64_t ncut, int64_t &first, int64_t &count) {
        first = which == 2 ? ncut : 0;
        count = which == 1 ? ncut : which == 2 ? n - ncut : n;
    };
    int64_t efirst, ecount, nfirst, ncount;
    range(mesh.nsharededges, mesh.ncut_edge_groups, efirst, ecount);
    range(mesh.nsharednodes, mesh.ncut_node_groups, nfirst, ncount);
    if (lv.nei == 0) ecount = 0;
    const int64_t total = ecount * lv.nei + ncount;
    if (total > 0) {
        int64_t blocks = (total + 255) / 256;
        if (blocks > cap * 4) blocks = cap * 4;
        hipLaunchKernelGGL(k_iface_csr, dim3((unsigned)blocks), dim3(256), 0, L.stream, mesh.edge_ptr + efirst,
                           mesh.edge_ent, ecount, lv.nei, lv.off_edge, mesh.node_ptr + nfirst, mesh.node_ent, ncount,
                           lv.ld, x);
        check_launch();
    }
}

// ---------------------------------------------------------------------------------------------
// entity masks (Dirichlet constraint / duplicate zeroing)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void entity_range(const LevelDev &lv, int bit, int &off, int &len)
{
    if (bit < lv.nface) {
        off = lv.off_face + bit * lv.nfi;
        len = lv.nfi;
    } else if (bit < lv.nface + lv.nedge) {
        off = lv.off_edge + (bit - lv.nface) * lv.nei;
        len = lv.nei;
    } else {
        off = bit - lv.nface - lv.nedge;
        len = 1;
    }
}

__global__ void __launch_bounds__(64) k_mask(LevelDev lv, int64_t ncells, const uint16_t *__restrict__ mask, double *x)
{
    const int64_t cell = blockIdx.x;
    if (cell >= ncells) return;
    uint32_t m = mask[cell];
    double *xc = x + cell * lv.ld;
    while (m) {
        const int bit = __ffs((int)m) - 1;
        m &= m - 1;
        int off, len;
        entity_range(lv, bit, off, len);
        for (int k = threadIdx.x; k < len; k += 64) xc[off + k] = 0.0;
    }
}

void launch_mask(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double *x, int which)
{
    hipLaunchKernelGGL(k_mask, dim3((unsigned)mesh.ncells), dim3(64), 0, L.stream, lv, mesh.ncells,
                       which == 0 ? mesh.dmask : mesh.dupmask, x);
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// level transfer
// ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT)
k_prolong_add(LevelDev fine, int nfc, int ldc, const double *__restrict__ xc, double *xf)
{
    extern __shared__ double smem[];
    const int64_t cell = blockIdx.x;
    const double *c = xc + cell * ldc;
    for (int t = threadIdx.x; t < nfc; t += NT) smem[t] = c[t];
    __syncthreads();
    double *f = xf + cell * fine.ld;
    for (int t = threadIdx.x; t < fine.nf; t += NT) {
        const int a = fine.par_a[t], b = fine.par_b[t];
        double y = f[t];
        if (a == b)
            y += 1.0 * smem[a];
        else {
            y += 0.5 * smem[a];   // CSC column order: parent with the smaller hierarchical id first
            y += 0.5 * smem[b];
        }
        f[t] = y;
    }
}

// The same for cells of thousands of nodes (level 7: 47 905 fine, 6 545 coarse nodes per cell -- the prolongation of the
// slab levels is a pass of its own): 1024 threads, two workgroups per CU, SPT column entries and packed parent words per
// thread in flight before the first use (the one-entry-per-trip loop above ran at 3.8 TB/s there).  Same roundings.
template <int NT, int SPT>
__global__ void __launch_bounds__(NT)
k_prolong_add_big(LevelDev fine, int nfc, int ldc, const double *__restrict__ xc, double *xf)
{
    extern __shared__ double smem[];
    const int64_t cell = blockIdx.x;
    const double *c = xc + cell * ldc;
    for (int t0 = threadIdx.x; t0 < nfc; t0 += NT * SPT) {
        double v[SPT];
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int t = t0 + q * NT;
            v[q] = t < nfc ? c[t] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int t = t0 + q * NT;
            if (t < nfc) smem[t] = v[q];
        }
    }
    __syncthreads();
    double *f = xf + cell * fine.ld;
    for (int t0 = threadIdx.x; t0 < fine.nf; t0 += NT * SPT) {
        double y[SPT];
        uint32_t w[SPT];
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int t = t0 + q * NT;
            if (t < fine.nf) {
                y[q] = f[t];
                w[q] = fine.par32[t];
            }
        }
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int t = t0 + q * NT;
            if (t < fine.nf) {
                const uint32_t a = w[q] & 0xffffu, b = w[q] >> 16;
                double r = y[q];
                if (a == b)
                    r += 1.0 * smem[a];
                else {
                    r += 0.5 * smem[a];   // CSC column order: parent with the smaller hierarchical id first
                    r += 0.5 * smem[b];
                }
                f[t] = r;
            }
        }
    }
}

template <int NT, bool USE_LDS>
__global__ void __launch_bounds__(NT)
k_restrict(LevelDev fine, int nfc, int ldc, const double *__restrict__ rf, double *bc)
{
    extern __shared__ double smem[];
    const int64_t cell = blockIdx.x;
    const double *f = rf + cell * fine.ld;
    const double *fs = f;
    if (USE_LDS) {
        constexpr int SPT = 8;   // loads first, LDS writes second: keeps 8 loads per thread in flight
        for (int t0 = threadIdx.x; t0 < fine.nf; t0 += NT * SPT) {
            double v[SPT];
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = t0 + q * NT;
                v[q] = t < fine.nf ? f[t] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < SPT; ++q) {
                const int t = t0 + q * NT;
                if (t < fine.nf) smem[t] = v[q];
            }
        }
        __syncthreads();
        fs = smem;
    }
    double *c = bc + cell * ldc;
    for (int t = threadIdx.x; t < nfc; t += NT) {
        const int b = fine.rptr[t], n = fine.rptr[t + 1] - b;   // 1 <= n <= 15 (3D) / 7 (2D)
        int idx[15];
#pragma unroll
        for (int q = 0; q < 15; ++q) idx[q] = fine.ridx[b + (q < n ? q : 0)];   // all index loads in flight at once
        double tmp = 0.0;
        tmp += 1.0 * fs[idx[0]];
#pragma unroll
        for (int q = 1; q < 15; ++q)
            if (q < n) tmp += 0.5 * fs[idx[q]];
        c[t] = tmp;
    }
}

void launch_prolong_add(const Launch &L, const LevelDev &fine, const LevelDev &coarse, int64_t ncells,
                        const double *xc, double *xf)
{
    size_t lds = sizeof(double) * coarse.nf;
    if (lds > 160 * 1024 && fine.dim == 2) {   // 2D levels 10 and 11: coarse values gathered through L2 (hmg_apply_rows.hip)
        launch_prolong_add_wide(L, fine, coarse, ncells, xc, xf);
        return;
    }
    if (lds > 160 * 1024) throw std::runtime_error("prolongation: coarse cell does not fit LDS");
    if (fine.nf <= 256) {
        auto k = k_prolong_add<64>;
        hipLaunchKernelGGL(k, dim3((unsigned)ncells), dim3(64), lds, L.stream, fine, coarse.nf, coarse.ld, xc, xf);
    } else if (fine.nf > 8192) {
        auto k = k_prolong_add_big<1024, 4>;
        if (lds > 48 * 1024)
            HMG_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3((unsigned)ncells), dim3(1024), lds, L.stream, fine, coarse.nf, coarse.ld, xc, xf);
    } else {
        auto k = k_prolong_add<256>;
        if (lds > 48 * 1024)
            HMG_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3((unsigned)ncells), dim3(256), lds, L.stream, fine, coarse.nf, coarse.ld, xc, xf);
    }
    check_launch();
}

void launch_restrict(const Launch &L, const LevelDev &fine, const LevelDev &coarse, int64_t ncells,
                     const double *rf, double *bc)
{
    size_t lds = sizeof(double) * fine.nf;
    if (fine.nf <= 256) {
        hipLaunchKernelGGL((k_restrict<64, true>), dim3((unsigned)ncells), dim3(64), lds, L.stream, fine, coarse.nf,
                           coarse.ld, rf, bc);
    } else if (lds <= 160 * 1024 && fine.nf > 2048) {
        auto k = k_restrict<1024, true>;
        if (lds > 48 * 1024)
            HMG_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3((unsigned)ncells), dim3(1024), lds, L.stream, fine, coarse.nf, coarse.ld, rf, bc);
    } else if (lds <= 160 * 1024) {
        auto k = k_restrict<256, true>;
        if (lds > 48 * 1024)
            HMG_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3((unsigned)ncells), dim3(256), lds, L.stream, fine, coarse.nf, coarse.ld, rf, bc);
    } else {
        hipLaunchKernelGGL((k_restrict<256, false>), dim3((unsigned)ncells), dim3(256), 0, L.stream, fine, coarse.nf,
                           coarse.ld, rf, bc);
    }
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// streaming vector kernels (flat storage, every copy of a shared DOF counted -- BLAS semantics)
//
// Launch shape (profiles/r02_stream_variants.txt): ONE double2 per thread, 256-thread blocks, as many blocks as
// there are pairs -- no grid-stride loop.  The dispatcher hands out blocks in order, so the ~2000 resident blocks
// sweep one contiguous 8 MB window through every stream; a persistent grid-stride grid touches addresses one
// grid-stride (8 MB) apart instead and loses 15 % (5.1 vs 6.0 TB/s on the 24 B/DOF update, 5.1 vs 6.3 TB/s on a
// copy).  Reductions leave one partial per block in L.rpart (deterministic: fixed block order, two more stages).
// ---------------------------------------------------------------------------------------------
constexpr int SB = 256;   // threads per streaming block

// grid of the kernels that keep a grid-stride loop (index arithmetic per element: permutation, synthetic fill, ...)
static inline int strided_blocks(const Launch &L, int64_t n, int per_thread)
{
    int64_t b = (n + (int64_t)256 * per_thread - 1) / ((int64_t)256 * per_thread);
    int64_t cap = (int64_t)L.num_cu * 8;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

static inline int64_t stream_blocks(int64_t n)
{
    const int64_t b = ((n >> 1) + SB - 1) / SB;
    return b < 1 ? 1 : b;
}

static void check_grid(int64_t nb)
{
    if (nb > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
}

// block partials [nb] -> 256 partials in `out` (block b sums a contiguous range: fixed order)
__global__ void __launch_bounds__(256) k_reduce_partials(const double *__restrict__ part, int64_t nb, double *out)
{
    __shared__ double red[4];
    const int64_t per = (nb + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    double a = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) a += part[i];
    const double s = block_sum(a, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ void __launch_bounds__(SB) k_fill(double *x, int64_t n, double v)
{
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) reinterpret_cast<double2 *>(x)[i] = make_double2(v, v);
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = v;
}

__global__ void __launch_bounds__(SB) k_copy(double *dst, const double *__restrict__ src, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) reinterpret_cast<double2 *>(dst)[i] = reinterpret_cast<const double2 *>(src)[i];
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
}

__global__ void __launch_bounds__(SB) k_axpy(double a, const double *__restrict__ x, double *y, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *y2 = reinterpret_cast<double2 *>(y);
        const double2 xv = reinterpret_cast<const double2 *>(x)[i];
        double2 yv = y2[i];
        yv.x = axpy1(a, xv.x, yv.x);
        yv.y = axpy1(a, xv.y, yv.y);
        y2[i] = yv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = axpy1(a, x[n - 1], y[n - 1]);
}

__global__ void __launch_bounds__(SB) k_xpby(const double *__restrict__ r, double b, double *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *p2 = reinterpret_cast<double2 *>(p);
        const double2 rv = reinterpret_cast<const double2 *>(r)[i];
        double2 pv = p2[i];
        pv.x = axpy1(b, pv.x, rv.x);
        pv.y = axpy1(b, pv.y, rv.y);
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = axpy1(b, p[n - 1], r[n - 1]);
}

__global__ void __launch_bounds__(SB)
k_dot(const double *__restrict__ x, const double *__restrict__ y, int64_t n, double *partials)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        const double2 xv = reinterpret_cast<const double2 *>(x)[i], yv = reinterpret_cast<const double2 *>(y)[i];
        acc += xv.x * yv.x;
        acc += xv.y * yv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc += x[n - 1] * y[n - 1];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(SB)
k_copy_dot(double *p, const double *__restrict__ r, int64_t n, double *partials)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        const double2 rv = reinterpret_cast<const double2 *>(r)[i];
        reinterpret_cast<double2 *>(p)[i] = rv;
        acc += rv.x * rv.x;
        acc += rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        p[n - 1] = r[n - 1];
        acc += r[n - 1] * r[n - 1];
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(SB)
k_cg_update(double *x, double *r, const double *__restrict__ p, const double *__restrict__ q, int64_t n,
            const double *__restrict__ scal, int s_num, int s_den, double *partials)
{
    __shared__ double red[4];
    const double alpha = scal[s_num] / scal[s_den];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 *r2 = reinterpret_cast<double2 *>(r);
        double2 xv = x2[i], rv = r2[i];
        const double2 pv = reinterpret_cast<const double2 *>(p)[i], qv = reinterpret_cast<const double2 *>(q)[i];
        xv.x = axpy1(alpha, pv.x, xv.x);
        xv.y = axpy1(alpha, pv.y, xv.y);
        rv.x = axpy1(-alpha, qv.x, rv.x);
        rv.y = axpy1(-alpha, qv.y, rv.y);
        x2[i] = xv;
        r2[i] = rv;
        acc += rv.x * rv.x;
        acc += rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        x[n - 1] = axpy1(alpha, p[n - 1], x[n - 1]);
        double rv = axpy1(-alpha, q[n - 1], r[n - 1]);
        r[n - 1] = rv;
        acc += rv * rv;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// rout = r - alpha q, partial rout.rout   (alpha = scal[s_num] / scal[s_den]; rout may be r); the x-update rides with
// the next fused apply
__global__ void __launch_bounds__(SB)
k_cg_rupdate(const double *r, double *rout, const double *__restrict__ q, int64_t n, const double *__restrict__ scal,
             int s_num, int s_den, double *partials)
{
    __shared__ double red[4];
    const double alpha = scal[s_num] / scal[s_den];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        double2 rv = reinterpret_cast<const double2 *>(r)[i];
        const double2 qv = reinterpret_cast<const double2 *>(q)[i];
        rv.x = axpy1(-alpha, qv.x, rv.x);
        rv.y = axpy1(-alpha, qv.y, rv.y);
        reinterpret_cast<double2 *>(rout)[i] = rv;
        acc += rv.x * rv.x;
        acc += rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double rv = axpy1(-alpha, q[n - 1], r[n - 1]);
        rout[n - 1] = rv;
        acc += rv * rv;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// k_cg_rupdate with the FACE part of q's interface sum done on the fly: q holds cell-local values on the shared faces
// (edges, corners and partition-cut entities are already summed in place), the partner copy is fetched through the
// per-cell table fpart[4 * cell + face] = partner cell << 2 | partner face (-1: none) and added in ascending cell order --
// the bits of the separate pass (k_iface_faces + k_cg_rupdate).  Saves that pass's read-modify-write of 28 % of q
// (16 B per face DOF) for 8 B per face DOF more here.  q itself stays unsummed on the faces.
// XU > 0 (the last step of a smoother whose caller reads x and r only -- the finest level's post-smoother inside hmg_vcycle, option
// lazy_top): the apply of that step formed p_i = r_i + beta p_{i-1} in LDS only and wrote neither p nor x; both pending x-updates
// are done here, p_i formed again on the fly from the r this pass reads anyway:  x = (x + ax p) + alpha (r + beta p)  -- the
// roundings of  x += alpha_{i-1} p_{i-1};  p_i = r_i + beta p_{i-1};  x += alpha_i p_i  one after the other (k_cg_x2_update).
// XU == 2: a third pending update comes first, x += az p0 (the step before wrote its direction next to p0 instead of over it).
struct XUSlots {
    Ratio a, b, z;
};
static_assert(sizeof(XUSlots) == 6 * sizeof(int), "XUSlots is a kernel argument: six ints");
// (the two pending x-updates themselves: xupd2() of hmg_stencil.hpp, shared with the flexible CG's kernel that forms z from them)
template <int XU>
__global__ void __launch_bounds__(SB)
k_cg_rupdate_faces(const double *r, double *rout, const double *__restrict__ q, int64_t n, const double *__restrict__ scal,
                   int s_num, int s_den, double *partials, const int32_t *__restrict__ fpart, int ld, double inv_ld,
                   int off_face, int off_int, int nfi, double *x, const double *__restrict__ p, const double *__restrict__ p0,
                   XUSlots xs)
{
    __shared__ double red[4];
    const double alpha = scal[s_num] / scal[s_den];
    const double ax = XU ? scal[xs.a.num] / scal[xs.a.den] : 0.0;
    const double beta = XU ? scal[xs.b.num] / scal[xs.b.den] : 0.0;
    const double az = XU == 2 ? scal[xs.z.num] / scal[xs.z.den] : 0.0;
    auto xupd = [&](double xv, double pv, double rv) { return xupd2(ax, beta, alpha, xv, pv, rv); };
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    auto summed = [&](int64_t e, double own) {          // q[e] with its face partner, if it has one
        int64_t cell = (int64_t)((double)e * inv_ld);
        int64_t slot = e - cell * ld;
        if (slot < 0) {
            cell -= 1;
            slot += ld;
        } else if (slot >= ld) {
            cell += 1;
            slot -= ld;
        }
        if (slot < off_face || slot >= off_int) return own;
        const int s = (int)slot - off_face;
        const int f = (s >= nfi) + (s >= 2 * nfi) + (s >= 3 * nfi);
        const int32_t p = fpart[4 * cell + f];
        if (p < 0) return own;
        const int64_t pc = p >> 2;
        const double other = q[pc * ld + off_face + (p & 3) * nfi + (s - f * nfi)];
        return cell < pc ? own + other : other + own;
    };
    if (i < (n >> 1)) {
        double2 rv = reinterpret_cast<const double2 *>(r)[i];
        const double2 qv = reinterpret_cast<const double2 *>(q)[i];
        if (XU) {
            double2 xv = reinterpret_cast<double2 *>(x)[i];
            const double2 pv = reinterpret_cast<const double2 *>(p)[i];
            if (XU == 2) {
                const double2 zv = reinterpret_cast<const double2 *>(p0)[i];
                xv.x = axpy1(az, zv.x, xv.x);
                xv.y = axpy1(az, zv.y, xv.y);
            }
            xv.x = xupd(xv.x, pv.x, rv.x);
            xv.y = xupd(xv.y, pv.y, rv.y);
            reinterpret_cast<double2 *>(x)[i] = xv;
        }
        rv.x = axpy1(-alpha, summed(2 * i, qv.x), rv.x);
        rv.y = axpy1(-alpha, summed(2 * i + 1, qv.y), rv.y);
        reinterpret_cast<double2 *>(rout)[i] = rv;
        acc += rv.x * rv.x;
        acc += rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        if (XU) x[n - 1] = xupd(XU == 2 ? axpy1(az, p0[n - 1], x[n - 1]) : x[n - 1], p[n - 1], r[n - 1]);
        double rv = axpy1(-alpha, summed(n - 1, q[n - 1]), r[n - 1]);
        rout[n - 1] = rv;
        acc += rv * rv;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The x half of k_cg_rupdate_faces<XU> alone (XU = 1, 2), for a caller that leaves the r half pending (hmg_vcycle, option lazy_r):
// reads x, p (, p0) and r, writes x -- no q, no partner gather, no r store, no reduction.  The step length it formed goes to
// alpha_out[XS_ALPHA] with a 1.0 behind it: k_cg_rupdate_faces<0> run later with alpha_out as its scalars (the ratio XS_LAST) forms the
// same alpha, whatever the scalar bank holds by then.  alpha_out[XS_BETA_NUM / _DEN]: numerator and denominator of this step's beta, for
// a caller that did not store Ap either (option lazy_ap) and runs the step's apply again with alpha_out as its scalars (XS_BETA).
template <int XU>
__global__ void __launch_bounds__(SB)
k_cg_x_tail(double *x, const double *__restrict__ p, const double *__restrict__ p0, const double *__restrict__ r, int64_t n,
            const double *__restrict__ scal, int s_num, int s_den, XUSlots xs, double *alpha_out)
{
    static_assert(XU == 1 || XU == 2, "one or two stored directions");
    const double alpha = scal[s_num] / scal[s_den];
    const double ax = scal[xs.a.num] / scal[xs.a.den];
    const double beta = scal[xs.b.num] / scal[xs.b.den];
    const double az = XU == 2 ? scal[xs.z.num] / scal[xs.z.den] : 0.0;
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 xv = reinterpret_cast<double2 *>(x)[i];
        const double2 pv = reinterpret_cast<const double2 *>(p)[i];
        const double2 rv = reinterpret_cast<const double2 *>(r)[i];
        if (XU == 2) {
            const double2 zv = reinterpret_cast<const double2 *>(p0)[i];
            xv.x = axpy1(az, zv.x, xv.x);
            xv.y = axpy1(az, zv.y, xv.y);
        }
        xv.x = xupd2(ax, beta, alpha, xv.x, pv.x, rv.x);
        xv.y = xupd2(ax, beta, alpha, xv.y, pv.y, rv.y);
        reinterpret_cast<double2 *>(x)[i] = xv;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n & 1) x[n - 1] = xupd2(ax, beta, alpha, XU == 2 ? axpy1(az, p0[n - 1], x[n - 1]) : x[n - 1], p[n - 1], r[n - 1]);
        if (!alpha_out) return;                  // (run late from the saved scalars, k_cg_x_save: they hold all of this already)
        alpha_out[XS_ALPHA] = alpha;
        alpha_out[XS_ONE] = 1.0;
        alpha_out[XS_BETA_NUM] = scal[xs.b.num]; // beta as the apply of this step read it: the same division forms it again
        alpha_out[XS_BETA_DEN] = scal[xs.b.den];
    }
}

// What k_cg_x_tail reads from the scalar bank, saved instead of used (hmg_vcycle, option lazy_x: the x-updates stay pending as well):
// the whole saved block (hmg_device.hpp: XS_ALPHA ... XS_FIRST_DEN) -- its first four doubles as k_cg_x_tail leaves them, then numerator
// and denominator of ax and of az (0 / 1 without a third update).  k_cg_x_tail, or a residual that carries the updates in its load phase, run later with `out` as its scalars forms every
// ratio by the same division of the same numbers, whatever the scalar bank holds by then.
__global__ void k_cg_x_save(const double *__restrict__ scal, int s_num, int s_den, XUSlots xs, int three, double *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    out[XS_ALPHA] = scal[s_num] / scal[s_den];
    out[XS_ONE] = 1.0;
    out[XS_BETA_NUM] = scal[xs.b.num];
    out[XS_BETA_DEN] = scal[xs.b.den];
    out[XS_PREV_NUM] = scal[xs.a.num];
    out[XS_PREV_DEN] = scal[xs.a.den];
    out[XS_FIRST_NUM] = three ? scal[xs.z.num] : 0.0;
    out[XS_FIRST_DEN] = three ? scal[xs.z.den] : 1.0;
}

// x += alpha p (alpha = scal[a_num]/scal[a_den]) and, if with_p, p = r + beta p (beta = scal[s_num]/scal[s_den])
__global__ void __launch_bounds__(SB)
k_cg_xp_update(double *x, double *p, const double *__restrict__ r, int64_t n, const double *__restrict__ scal,
               int a_num, int a_den, int s_num, int s_den, int with_p)
{
    const double alpha = scal[a_num] / scal[a_den];
    const double beta = with_p ? scal[s_num] / scal[s_den] : 0.0;
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 *p2 = reinterpret_cast<double2 *>(p);
        double2 xv = x2[i], pv = p2[i];
        double2 rv = make_double2(0.0, 0.0);
        if (with_p) rv = reinterpret_cast<const double2 *>(r)[i];
        xv.x = axpy1(alpha, pv.x, xv.x);
        xv.y = axpy1(alpha, pv.y, xv.y);
        x2[i] = xv;
        if (with_p) {
            pv.x = axpy1(beta, pv.x, rv.x);
            pv.y = axpy1(beta, pv.y, rv.y);
            p2[i] = pv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        x[n - 1] = axpy1(alpha, p[n - 1], x[n - 1]);
        if (with_p) p[n - 1] = axpy1(beta, p[n - 1], r[n - 1]);
    }
}

// two CG x-updates at once, the second direction formed on the fly (a post-smoother's dead last step below the finest level,
// see smooth()): x = (x + (scal[a_num]/scal[a_den]) p) + (scal[c_num]/scal[c_den]) (r + (scal[b_num]/scal[b_den]) p) -- the three
// roundings of x += alpha_0 p_0; p_1 = r + beta p_0; x += alpha_1 p_1 done one after the other (k_apply's x3 mode does the same)
__global__ void __launch_bounds__(SB)
k_cg_x2_update(double *x, const double *__restrict__ p, const double *__restrict__ r, int64_t n, const double *__restrict__ scal,
               int a_num, int a_den, int b_num, int b_den, int c_num, int c_den)
{
    const double ax = scal[a_num] / scal[a_den];
    const double beta = scal[b_num] / scal[b_den];
    const double c2 = scal[c_num] / scal[c_den];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    auto upd = [&](double xv, double pv, double rv) {
        const double t1 = axpy1(ax, pv, xv);
        const double p2 = axpy1(beta, pv, rv);
        return axpy1(c2, p2, t1);
    };
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 xv = x2[i];
        const double2 pv = reinterpret_cast<const double2 *>(p)[i], rv = reinterpret_cast<const double2 *>(r)[i];
        xv.x = upd(xv.x, pv.x, rv.x);
        xv.y = upd(xv.y, pv.y, rv.y);
        x2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = upd(x[n - 1], p[n - 1], r[n - 1]);
}

__global__ void __launch_bounds__(SB)
k_cg_pupdate(double *p, const double *__restrict__ r, int64_t n, const double *__restrict__ scal, int s_num, int s_den)
{
    const double beta = scal[s_num] / scal[s_den];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *p2 = reinterpret_cast<double2 *>(p);
        const double2 rv = reinterpret_cast<const double2 *>(r)[i];
        double2 pv = p2[i];
        pv.x = axpy1(beta, pv.x, rv.x);
        pv.y = axpy1(beta, pv.y, rv.y);
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = axpy1(beta, p[n - 1], r[n - 1]);
}

static void finalize(const Launch &L, int nb, int slot)
{
    launch_finalize(L, L.partials, nb, slot);
    check_launch();
}

// Where a streaming reduction over nb blocks leaves its partials, and how they become scal[slot]: few blocks go to the
// small buffer and one finalize; many go to L.rpart, are folded to 256 partials, then finalized.
static double *reduce_target(const Launch &L, int64_t nb)
{
    if (nb <= 2048) return L.partials;
    if (!L.rpart || nb > L.rpart_cap) throw std::runtime_error("reduction scratch too small for this vector");
    return L.rpart;
}

static void reduce_finish(const Launch &L, int64_t nb, int slot)
{
    if (nb <= 2048) {
        finalize(L, (int)nb, slot);
        return;
    }
    hipLaunchKernelGGL(k_reduce_partials, dim3(256), dim3(256), 0, L.stream, L.rpart, nb, L.partials);
    check_launch();
    finalize(L, 256, slot);
}

void launch_fill(const Launch &L, double *x, int64_t n, double v)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, n, v);
    check_launch();
}
void launch_copy(const Launch &L, double *dst, const double *src, int64_t n)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_copy, dim3((unsigned)nb), dim3(SB), 0, L.stream, dst, src, n);
    check_launch();
}
void launch_axpy(const Launch &L, double a, const double *x, double *y, int64_t n)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_axpy, dim3((unsigned)nb), dim3(SB), 0, L.stream, a, x, y, n);
    check_launch();
}
void launch_xpby(const Launch &L, const double *r, double b, double *p, int64_t n)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_xpby, dim3((unsigned)nb), dim3(SB), 0, L.stream, r, b, p, n);
    check_launch();
}
void launch_dot(const Launch &L, const double *x, const double *y, int64_t n, int slot)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_dot, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, y, n, reduce_target(L, nb));
    check_launch();
    reduce_finish(L, nb, slot);
}
void launch_copy_dot(const Launch &L, double *p, const double *r, int64_t n, int slot)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_copy_dot, dim3((unsigned)nb), dim3(SB), 0, L.stream, p, r, n, reduce_target(L, nb));
    check_launch();
    reduce_finish(L, nb, slot);
}
void launch_cg_update(const Launch &L, double *x, double *r, const double *p, const double *q, int64_t n, Ratio alpha, int s_out)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_update, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, r, p, q, n, L.scal, alpha.num, alpha.den,
                       reduce_target(L, nb));
    check_launch();
    reduce_finish(L, nb, s_out);
}
void launch_cg_rupdate(const Launch &L, const double *r, double *rout, const double *q, int64_t n, Ratio alpha, int s_out)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_rupdate, dim3((unsigned)nb), dim3(SB), 0, L.stream, r, rout, q, n, L.scal, alpha.num, alpha.den,
                       reduce_target(L, nb));
    check_launch();
    reduce_finish(L, nb, s_out);
}

void launch_cg_rupdate_faces(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const double *r, double *rout,
                             const double *q, int64_t n, Ratio alpha, int s_out, const double *scal)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_rupdate_faces<0>, dim3((unsigned)nb), dim3(SB), 0, L.stream, r, rout, q, n, scal ? scal : L.scal, alpha.num,
                       alpha.den, reduce_target(L, nb), mesh.face_partner, lv.ld, 1.0 / (double)lv.ld, lv.off_face, lv.off_int, lv.nfi,
                       (double *)nullptr, (const double *)nullptr, (const double *)nullptr, XUSlots{});
    check_launch();
    reduce_finish(L, nb, s_out);
}

// The kernels' view of two or three pending x-updates: p = u.p1, p0 = u.p0 (three), r = u.r2, alpha = u.last, and these slots
static XUSlots xu_slots(const XUpdates &u)
{
    if ((u.count != 2 && u.count != 3) || !u.p1 || !u.r2 || (u.count == 3) != (u.p0 != nullptr))
        throw std::runtime_error("pending x-updates without their vectors");
    return XUSlots{u.prev, u.beta, u.count == 3 ? u.first : Ratio{0, 0}};
}

// ... with the pending x-updates of a lazy last step: x = ((x [+ first p0]) + prev p1) + last (r2 + beta p1)
void launch_cg_rupdate_faces_x(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double *rout, const double *q, int64_t n,
                               int s_out, double *x, const XUpdates &u)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    const XUSlots xs = xu_slots(u);
    if (u.scal) throw std::runtime_error("an r-update reads its step length from the scalar bank");
    if (u.p0)
        hipLaunchKernelGGL(k_cg_rupdate_faces<2>, dim3((unsigned)nb), dim3(SB), 0, L.stream, u.r2, rout, q, n, L.scal, u.last.num, u.last.den,
                           reduce_target(L, nb), mesh.face_partner, lv.ld, 1.0 / (double)lv.ld, lv.off_face, lv.off_int, lv.nfi, x, u.p1,
                           u.p0, xs);
    else
        hipLaunchKernelGGL(k_cg_rupdate_faces<1>, dim3((unsigned)nb), dim3(SB), 0, L.stream, u.r2, rout, q, n, L.scal, u.last.num, u.last.den,
                           reduce_target(L, nb), mesh.face_partner, lv.ld, 1.0 / (double)lv.ld, lv.off_face, lv.off_int, lv.nfi, x, u.p1,
                           u.p0, xs);
    check_launch();
    reduce_finish(L, nb, s_out);
}

// the x-updates of launch_cg_rupdate_faces_x alone
void launch_cg_x_tail(const Launch &L, double *x, int64_t n, const XUpdates &u, double *alpha_out)
{
    if ((!alpha_out && !u.scal) || n <= 0) throw std::runtime_error("x-only tail without a place for its step length");
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    const XUSlots xs = xu_slots(u);
    const double *scal = u.scal ? u.scal : L.scal;
    if (u.p0)
        hipLaunchKernelGGL(k_cg_x_tail<2>, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, u.p1, u.p0, u.r2, n, scal, u.last.num, u.last.den, xs,
                           alpha_out);
    else
        hipLaunchKernelGGL(k_cg_x_tail<1>, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, u.p1, u.p0, u.r2, n, scal, u.last.num, u.last.den, xs,
                           alpha_out);
    check_launch();
}

// ... not run at all: what it would read from the scalar bank goes to out[0 .. XS_COUNT) (k_cg_x_save)
void launch_cg_x_save(const Launch &L, const XUpdates &u, double *out)
{
    if (!out || u.scal) throw std::runtime_error("pending x-updates without a place for their scalars");
    hipLaunchKernelGGL(k_cg_x_save, dim3(1), dim3(1), 0, L.stream, L.scal, u.last.num, u.last.den, xu_slots(u), u.count == 3 ? 1 : 0, out);
    check_launch();
}

void launch_cg_xp_update(const Launch &L, double *x, double *p, const double *r, int64_t n, Ratio alpha, Ratio beta, int with_p)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_xp_update, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, p, r, n, L.scal, alpha.num, alpha.den, beta.num,
                       beta.den, with_p);
    check_launch();
}

void launch_cg_x2_update(const Launch &L, double *x, int64_t n, const XUpdates &u)
{
    if (u.count != 2 || !u.p1 || !u.r2 || u.scal) throw std::runtime_error("the one-pass x-update takes two pending updates from the scalar bank");
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_x2_update, dim3((unsigned)nb), dim3(SB), 0, L.stream, x, u.p1, u.r2, n, L.scal, u.prev.num, u.prev.den,
                       u.beta.num, u.beta.den, u.last.num, u.last.den);
    check_launch();
}

void launch_cg_pupdate(const Launch &L, double *p, const double *r, int64_t n, Ratio beta)
{
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    hipLaunchKernelGGL(k_cg_pupdate, dim3((unsigned)nb), dim3(SB), 0, L.stream, p, r, n, L.scal, beta.num, beta.den);
    check_launch();
}

// sum over first copies only: cell-wise, entities flagged in dupmask skipped
__global__ void __launch_bounds__(256)
k_norm2_unique(LevelDev lv, int64_t ncells, const uint16_t *__restrict__ dupmask, const double *__restrict__ x,
               double *partials)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const uint32_t dm = dupmask[cell];
        const double *xc = x + cell * lv.ld;
        for (int t = threadIdx.x; t < lv.nf; t += 256) {
            const int cls = (int)((lv.meta[t] >> 24) & 0xffu);
            const bool dup = cls > 0 && ((dm >> (cls - 1)) & 1u);
            const double v = xc[t];
            if (!dup) acc += v * v;
        }
    }
    double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

void launch_norm2_unique(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const double *x, int slot)
{
    if (!lv.meta) {   // 2D levels 9..11 have no packed words: entity classes from the slot ranges (hmg_apply_rows.hip)
        const int64_t nbw = launch_norm2_unique_wide(L, lv, mesh, x);
        if (nbw == 0) {
            launch_fill(L, L.scal + slot, 1, 0.0);
            return;
        }
        finalize(L, (int)nbw, slot);
        return;
    }
    int64_t nb = mesh.ncells;
    if (nb > (int64_t)L.num_cu * 8) nb = (int64_t)L.num_cu * 8;
    hipLaunchKernelGGL(k_norm2_unique, dim3((unsigned)nb), dim3(256), 0, L.stream, lv, mesh.ncells, mesh.dupmask, x,
                       L.partials);
    check_launch();
    finalize(L, (int)nb, slot);
}

// ---------------------------------------------------------------------------------------------
// level-1 gather / scatter (level-1 storage slot == local node id)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gather_base(const int32_t *__restrict__ node_first, int64_t nnodes, int ld1, const double *__restrict__ v1, double *u)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nnodes) return;
    const int32_t v = node_first[g];
    u[g] = v >= 0 ? v1[(int64_t)(v >> 3) * ld1 + (v & 7)] : 0.0;
}

__global__ void __launch_bounds__(256)
k_scatter_base(const int32_t *__restrict__ cells, int64_t ncells, int npc, int ld1, const double *__restrict__ u,
               double *v1)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncells * npc) return;
    const int64_t c = i / npc;
    const int l = (int)(i - c * npc);
    v1[c * ld1 + l] = u[cells[i]];
}

// partitioned gather: u_global[nodes_g[q]] = v1[first local copy of local node q], owned nodes only
__global__ void __launch_bounds__(256)
k_gather_owned(const int32_t *__restrict__ node_first, const int32_t *__restrict__ nodes_g,
               const int32_t *__restrict__ owned, int64_t nlocal, int ld1, const double *__restrict__ v1, double *ug)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nlocal || !owned[q]) return;
    const int32_t v = node_first[q];
    ug[nodes_g[q]] = v1[(int64_t)(v >> 3) * ld1 + (v & 7)];
}

void launch_gather_owned(const Launch &L, const MeshDev &mesh, const int32_t *nodes_g, const int32_t *owned, int ld1,
                         const double *v1, double *ug)
{
    hipLaunchKernelGGL(k_gather_owned, dim3((unsigned)((mesh.nnodes + 255) / 256)), dim3(256), 0, L.stream,
                       mesh.node_first, nodes_g, owned, mesh.nnodes, ld1, v1, ug);
    check_launch();
}

void launch_scatter_cells(const Launch &L, const int32_t *cell_nodes, int64_t ncells, int npc, int ld1, const double *u,
                          double *v1)
{
    hipLaunchKernelGGL(k_scatter_base, dim3((unsigned)((ncells * npc + 255) / 256)), dim3(256), 0, L.stream,
                       cell_nodes, ncells, npc, ld1, u, v1);
    check_launch();
}

void launch_gather_base(const Launch &L, const MeshDev &mesh, int ld1, const double *v1, double *u)
{
    hipLaunchKernelGGL(k_gather_base, dim3((unsigned)((mesh.nnodes + 255) / 256)), dim3(256), 0, L.stream,
                       mesh.node_first, mesh.nnodes, ld1, v1, u);
    check_launch();
}
void launch_scatter_base(const Launch &L, const MeshDev &mesh, int ld1, const double *u, double *v1)
{
    const int npc = mesh.dim + 1;
    hipLaunchKernelGGL(k_scatter_base, dim3((unsigned)((mesh.ncells * npc + 255) / 256)), dim3(256), 0, L.stream,
                       mesh.cells, mesh.ncells, npc, ld1, u, v1);
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// API order (hierarchical, Nf x Ne column-major) <-> storage order; deterministic synthetic fill
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_permute(LevelDev lv, int64_t ncells, const double *__restrict__ src, double *dst, int to_storage)
{
    const int64_t total = ncells * lv.nf;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i / lv.nf;
        const int h = (int)(i - c * lv.nf);
        const int s = lv.hier2slot[h];
        if (to_storage)
            dst[c * lv.ld + s] = src[i];
        else
            dst[i] = src[c * lv.ld + s];
    }
}

void launch_permute(const Launch &L, const LevelDev &lv, int64_t ncells, const double *src, double *dst, int to_storage)
{
    hipLaunchKernelGGL(k_permute, dim3(strided_blocks(L, ncells * lv.nf, 4)), dim3(256), 0, L.stream, lv, ncells, src,
                       dst, to_storage);
    check_launch();
}

__device__ __forceinline__ double hash_u01(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// x[hier h, cell c] = u01(seed, ((c + cell_offset) << 20) | h): independent of the storage order
__global__ void __launch_bounds__(256)
k_fill_random(LevelDev lv, int64_t ncells, double *x, uint64_t seed, int64_t cell_offset)
{
    const int64_t total = ncells * lv.nf;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i / lv.nf;
        const int h = (int)(i - c * lv.nf);
        x[c * lv.ld + lv.hier2slot[h]] = hash_u01(seed, ((uint64_t)(c + cell_offset) << 20) | (uint64_t)h);
    }
}

void launch_fill_random(const Launch &L, const LevelDev &lv, int64_t ncells, double *x, uint64_t seed,
                        int64_t cell_offset)
{
    hipLaunchKernelGGL(k_fill_random, dim3(strided_blocks(L, ncells * lv.nf, 4)), dim3(256), 0, L.stream, lv, ncells, x,
                       seed, cell_offset);
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// coarse (level-1) preconditioned CG (Jacobi, or Chebyshev iterates of the Jacobi-scaled operator: k_coarse_cheb) on the assembled interior matrix
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_coarse_gather_rhs(const int32_t *__restrict__ interior, int64_t n, const double *__restrict__ u, double *b)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = u[interior[i]];
}

__global__ void __launch_bounds__(256)
k_coarse_scatter_sol(const int32_t *__restrict__ interior, int64_t n, const double *__restrict__ x, double *u)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[interior[i]] = x[i];
}

// The level-1 matrix with the constants in its kernel (torus, lambda = 0: hmg_grid_set_mean_free): v <- v - mean(v), the
// orthogonal projection onto its range, on the right-hand side in front of the PCG and on the solution behind it.  One
// workgroup: thread t sums entries t, t + 1024, ... in ascending order, the wave and block sums are block_sum's -- the order of
// additions is fixed by n alone, so every run gives the same bits.  Two passes: the first leaves a mean of rounding size
// (eps |v|), which against a right-hand side that is almost a constant would be an inconsistent component the PCG cannot reduce;
// the second takes that out as well.  A level-1 system is at most a few 10^5 unknowns: n / 1024 loads per thread, a few
// microseconds next to the tens of launches of the solve between the two calls.
__global__ void __launch_bounds__(1024) k_coarse_remove_mean(double *v, int64_t n)
{
    __shared__ double red[16];
    __shared__ double mean;
    for (int pass = 0; pass < 2; ++pass) {
        double a = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += 1024) a += v[i];
        const double s = block_sum(a, red);
        if (threadIdx.x == 0) mean = s / (double)n;
        __syncthreads();
        const double m = mean;
        for (int64_t i = threadIdx.x; i < n; i += 1024) v[i] -= m;   // (a thread's own entries: nothing to wait for)
        __syncthreads();                                               // (mean is rewritten in the next pass)
    }
}

__global__ void __launch_bounds__(256)
k_coarse_init(CoarseDev A, const double *__restrict__ b, double *x, double *r, double *z, double *p, double *part0,
              double *part1, double zscale, double *dcheb)
{
    // zscale, dcheb: polynomial preconditioner (k_coarse_cheb) -- z = d_0 = (1 / theta) D^-1 r is the first Chebyshev iterate
    __shared__ double red[4];
    double rz = 0.0, bb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
        const double bi = b[i];
        const double zi = dcheb ? zscale * (bi / A.diag[i]) : bi / A.diag[i];
        x[i] = 0.0;
        r[i] = bi;
        z[i] = zi;
        p[i] = zi;
        if (dcheb) dcheb[i] = zi;
        rz += bi * zi;
        bb += bi * bi;
    }
    double s0 = block_sum(rz, red);
    double s1 = block_sum(bb, red);
    if (threadIdx.x == 0) {
        part0[blockIdx.x] = s0;
        part1[blockIdx.x] = s1;
    }
}

// Sparse product of the level-1 matrix, CR consecutive rows per group of 16 lanes: row r's entries go to the lanes as before (entry
// rowptr[r] + lane, then every 16th: the Freudenthal lattice has <= 15 per row) and are folded in the same xor tree, so a row's sum
// has the bits it always had -- but the (value, column) pairs and the gathers of CR rows are in flight together.  Round 4: with one
// row per group a product was a chain of dependent round trips, 16 rounds per group at 64^3 cubes with four waves per SIMD: 21 us
// for 49 MB.  Every lane of the group returns all CR sums.
constexpr int CR = 4;
__device__ __forceinline__ void coarse_rows_product(const CoarseDev &A, const double *__restrict__ z, int64_t i0, int sub, double (&s)[CR])
{
    int rp[CR + 1];
#pragma unroll
    for (int j = 0; j <= CR; ++j) rp[j] = A.rowptr[i0 + j < A.n ? i0 + j : A.n];
    double v[CR], zz[CR];
#pragma unroll
    for (int j = 0; j < CR; ++j) {
        const int k = rp[j] + sub;
        const bool ok = k < rp[j + 1];
        const int kc = ok ? k : 0;
        v[j] = A.val[kc];
        zz[j] = z[A.colidx[kc]];       // (not ok: entry 0, a valid address; its product is dropped)
        if (!ok) v[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < CR; ++j) {
        s[j] = 0.0;
        s[j] += v[j] * zz[j];
        for (int k = rp[j] + sub + 16; k < rp[j + 1]; k += 16) s[j] += A.val[k] * z[A.colidx[k]];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < CR; ++j) s[j] += __shfl_xor(s[j], o, 16);
    }
}

static_assert(CR == 4, "the row epilogues pick one of four sums");

// Two-launch form of one PCG iteration (round 3): `direction` + `update`.  With q = A p carried by its own recurrence,
//   p' = z + beta p,   q' = A z + beta q      (A p' = A z + beta A p),
// the sparse product reads z, which the previous update left complete, and never a neighbour's p -- so the p-update, the
// product and the partial sums of p.q are one kernel; beta, the convergence test and the bookkeeping that k_coarse_pupdate did
// ride in its head (every block sums the same partials in the same order: the decision is the same in all of them).  On the
// level-1 systems of configs 3-5 the recurrence changes neither the iteration count nor the true residual (7.7e-14 / 9.2e-14
// at contrast 9 / 100, x equal to 5e-16): tools/dev note in profiles/r03_experiments.txt.
//   mode 0: a regular iteration;  1: the first of a solve (p = z and rz come from k_coarse_init: q = A z);
//   2: bookkeeping only (behind the last update of a batch, so that the host finds the flag and the count up to date)
//   count_it = 0: the update before this launch has been counted already (by a mode-2 launch)
__global__ void __launch_bounds__(256)
k_coarse_direction(CoarseDev A, double *p, double *q, const double *__restrict__ z, double *scal, int slot_old, int slot_new,
                   const double *__restrict__ part_rz, const double *__restrict__ part_rr, int nb_upd, double rtol2, int mode,
                   int count_it, double *part_pq, int nb_rz)
{
    __shared__ double red[4];
    __shared__ double bc;
    __shared__ int skip;
    if (threadIdx.x == 0) skip = scal[S_DONE] != 0.0 || !(scal[S_C2] > 0.0);
    __syncthreads();
    if (skip) return;
    double beta = 0.0;
    if (mode != 1) {
        const double rz_new = sum_partials_all(part_rz, nb_rz, red, &bc);   // (polynomial preconditioner: from the last Chebyshev step)
        const double rr = sum_partials_all(part_rr, nb_upd, red, &bc);
        const double rz_old = scal[slot_old];
        beta = rz_old != 0.0 ? rz_new / rz_old : 0.0;
        const bool done = rr <= rtol2 * scal[S_C2];                 // (NaN compares false: the budget runs out, the host sees S_CRR)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            scal[slot_new] = rz_new;
            if (count_it) scal[S_ITER] += 1.0;
            scal[S_CRR] = rr;
            if (done) scal[S_DONE] = 1.0;
        }
        if (done || mode == 2) return;
    }
    // 16 lanes per row (the level-1 matrix of the Freudenthal lattice has <= 15 entries per row): the lanes of a row read
    // consecutive (value, column) pairs -- coalesced, where one thread per row strides by the row length -- and fold their
    // products in a fixed xor tree, so the result does not depend on the launch shape (64^3 cubes, 274 625 rows: 11.3 -> 4.9 ms
    // per solve in round 2)
    const int sub = threadIdx.x & 15;
    double acc = 0.0;
    for (int64_t i0 = CR * (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4); i0 < A.n; i0 += CR * (((int64_t)gridDim.x * blockDim.x) >> 4)) {
        const int64_t i = i0 + sub;                     // lane j < CR finishes row i0 + j
        const bool mine = sub < CR && i < A.n;
        double zi = 0.0, pi0 = 0.0, qi0 = 0.0;
        if (mine) {
            zi = z[i];
            if (mode != 1) {
                pi0 = p[i];
                qi0 = q[i];
            }
        }
        double sr[CR];
        coarse_rows_product(A, z, i0, sub, sr);
        if (mine) {
            const double s = sub == 0 ? sr[0] : sub == 1 ? sr[1] : sub == 2 ? sr[2] : sr[3];
            const double pi = mode == 1 ? zi : zi + beta * pi0;
            const double qi = mode == 1 ? s : s + beta * qi0;
            p[i] = pi;
            q[i] = qi;
            acc += pi * qi;
        }
    }
    const double sacc = block_sum(acc, red);
    if (threadIdx.x == 0) part_pq[blockIdx.x] = sacc;
}

// One step of the Chebyshev iteration for D^-1 A z = D^-1 r from z_1 = (1 / theta) D^-1 r (Saad, Iterative Methods, Alg. 12.1):
//   d <- c1 d + c2 D^-1 (r - A zin),  zout = zin + d          (c1 = rho_j rho_j-1, c2 = 2 rho_j / delta: host, launch_coarse_cheb)
// k - 1 of these between the update and the direction kernel make z = p_{k-1}(D^-1 A) D^-1 r, a symmetric positive definite
// polynomial preconditioner (the interval [lmax / ratio, lmax] with lmax a Gershgorin bound: the polynomial stays positive on the
// whole spectrum).  No reductions but the last step's partial sums of r.z: an outer CG iteration costs k + 1 launches for k
// sparse products, where plain Jacobi-PCG pays two launches and two grid-wide sums per product.  16 lanes per row as in
// k_coarse_direction.
__global__ void __launch_bounds__(256)
k_coarse_cheb(CoarseDev A, const double *__restrict__ r, const double *__restrict__ zin, double *zout, double *d, double c1, double c2,
              const double *__restrict__ scal, int last, double *part_rz)
{
    __shared__ double red[4];
    if (scal[S_DONE] != 0.0 || !(scal[S_C2] > 0.0)) return;
    const int sub = threadIdx.x & 15;
    double acc = 0.0;
    for (int64_t i0 = CR * (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4); i0 < A.n; i0 += CR * (((int64_t)gridDim.x * blockDim.x) >> 4)) {
        const int64_t i = i0 + sub;                     // lane j < CR finishes row i0 + j
        const bool mine = sub < CR && i < A.n;
        double ri = 0.0, dold = 0.0, dg = 1.0, zold = 0.0;
        if (mine) {
            ri = r[i];
            dold = d[i];
            dg = A.diag[i];
            zold = zin[i];
        }
        double sr[CR];
        coarse_rows_product(A, zin, i0, sub, sr);
        if (mine) {
            const double s = sub == 0 ? sr[0] : sub == 1 ? sr[1] : sub == 2 ? sr[2] : sr[3];
            const double di = c1 * dold + c2 * ((ri - s) / dg);
            const double zi = zold + di;
            d[i] = di;
            zout[i] = zi;
            acc += ri * zi;
        }
    }
    if (last) {
        const double sacc = block_sum(acc, red);
        if (threadIdx.x == 0) part_rz[blockIdx.x] = sacc;
    }
}

// update: sums the partials of p.q itself (P0); partials of r.z -> P1, r.r -> P2.  rz lives in scal[slot_old] /
// scal[slot_new], exchanged by the host every iteration, so no kernel overwrites a scalar that another block of the same
// launch may still read.
__global__ void __launch_bounds__(256)
k_coarse_update(CoarseDev A, double *x, double *r, double *z, const double *__restrict__ p, const double *__restrict__ q,
                const double *__restrict__ scal, int slot_old, const double *__restrict__ part_pap, int nb, double *part_rz,
                double *part_rr, double zscale, double *dcheb)
{
    __shared__ double red[4];
    __shared__ double bc;
    if (scal[S_DONE] != 0.0 || !(scal[S_C2] > 0.0)) return;
    const double pap = sum_partials_all(part_pap, nb, red, &bc);
    // exact convergence (r = 0, e.g. a 1-unknown system after one step) makes p.Ap = 0: stay at the solution
    const double alpha = pap != 0.0 ? scal[slot_old] / pap : 0.0;
    double rz = 0.0, rr = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        const double zi = dcheb ? zscale * (ri / A.diag[i]) : ri / A.diag[i];
        r[i] = ri;
        z[i] = zi;
        if (dcheb) dcheb[i] = zi;
        rz += ri * zi;
        rr += ri * ri;
    }
    double s0 = block_sum(rz, red);
    double s1 = block_sum(rr, red);
    if (threadIdx.x == 0) {
        part_rz[blockIdx.x] = s0;
        part_rr[blockIdx.x] = s1;
    }
}

static inline int coarse_blocks(const Launch &L, int64_t n)
{
    int64_t b = (n + 255) / 256;
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

static inline int coarse_spmv_blocks(int64_t n)      // 16 lanes per row
{
    int64_t b = (16 * n + 255) / 256;
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

void launch_coarse_gather_rhs(const Launch &L, const CoarseDev &A, const double *u, double *b)
{
    if (A.n == 0) return;                          // (every node is constrained: no unknown, and a launch of no blocks is an error)
    hipLaunchKernelGGL(k_coarse_gather_rhs, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, L.stream, A.interior,
                       A.n, u, b);
    check_launch();
}
void launch_coarse_scatter_sol(const Launch &L, const CoarseDev &A, int64_t nnodes, const double *x, double *u)
{
    launch_fill(L, u, nnodes, 0.0);
    if (A.n == 0) return;                          // (x = 0 on every node)
    hipLaunchKernelGGL(k_coarse_scatter_sol, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, L.stream, A.interior,
                       A.n, x, u);
    check_launch();
}
void launch_coarse_remove_mean(const Launch &L, const CoarseDev &A, double *v)
{
    if (A.n == 0) return;
    hipLaunchKernelGGL(k_coarse_remove_mean, dim3(1), dim3(1024), 0, L.stream, v, A.n);
    check_launch();
}
void launch_coarse_init(const Launch &L, const CoarseDev &A, const double *b, double *x, double *r, double *z, double *p,
                        double zscale, double *dcheb)
{
    int nb = coarse_blocks(L, A.n);
    hipLaunchKernelGGL(k_coarse_init, dim3(nb), dim3(256), 0, L.stream, A, b, x, r, z, p, L.partials, L.partials + 2048, zscale, dcheb);
    check_launch();
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, L.stream, L.partials, nb, L.scal, (int)S_C0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, L.stream, L.partials + 2048, nb, L.scal, (int)S_C2);
    HMG_HIP_CHECK(hipMemsetAsync(L.scal + S_DONE, 0, 3 * sizeof(double), L.stream));   // S_DONE, S_ITER, S_CRR
    check_launch();
}

void launch_coarse_cheb(const Launch &L, const CoarseDev &A, const double *r, const double *zin, double *zout, double *d, double c1,
                        double c2, int last)
{
    const int nb = coarse_spmv_blocks(A.n);
    hipLaunchKernelGGL(k_coarse_cheb, dim3(nb), dim3(256), 0, L.stream, A, r, zin, zout, d, c1, c2, L.scal, last, L.partials + 1024);
    check_launch();
}

// scal[S_C0] = r.z from the partials the last Chebyshev step left (first iteration of a solve)
void launch_coarse_rz_from_cheb(const Launch &L, const CoarseDev &A)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, L.stream, L.partials + 1024, coarse_spmv_blocks(A.n), L.scal, (int)S_C0);
    check_launch();
}
// partial buffers of the PCG inside L.partials (>= 4096 doubles, nb <= 1024): P0 p.q, P1 r.z, P2 r.r
void launch_coarse_direction(const Launch &L, const CoarseDev &A, double *p, double *q, const double *z, int slot_old, int slot_new,
                             double rtol2, int mode, int count_it, int rz_from_cheb)
{
    const int nb = mode == 2 ? 1 : coarse_spmv_blocks(A.n);
    hipLaunchKernelGGL(k_coarse_direction, dim3(nb), dim3(256), 0, L.stream, A, p, q, z, L.scal, slot_old, slot_new,
                       L.partials + 1024, L.partials + 2048, coarse_blocks(L, A.n), rtol2, mode, count_it, L.partials,
                       rz_from_cheb ? coarse_spmv_blocks(A.n) : coarse_blocks(L, A.n));
    check_launch();
}

void launch_coarse_update(const Launch &L, const CoarseDev &A, double *x, double *r, double *z, const double *p,
                          const double *q, int slot_old, double zscale, double *dcheb)
{
    int nb = coarse_blocks(L, A.n);
    hipLaunchKernelGGL(k_coarse_update, dim3(nb), dim3(256), 0, L.stream, A, x, r, z, p, q, L.scal, slot_old, L.partials,
                       coarse_spmv_blocks(A.n), L.partials + 1024, L.partials + 2048, zscale, dcheb);
    check_launch();
}
// r.r of the last update -> scal[S_TMP] (convergence check)
void launch_coarse_residual_norm(const Launch &L, const CoarseDev &A)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, L.stream, L.partials + 2048, coarse_blocks(L, A.n), L.scal,
                       (int)S_TMP);
    check_launch();
}

// Load pairing of the driver integrals: sum over the first nsub cells of |J_c| sum_i v_i s_i (s a load vector such as
// rhs_a.xi.grad(v)).  A streaming kernel in the launch shape of the others (one double2 per thread by FLAT index over the
// prefix's nsub * ld doubles, one block per 512 doubles, no loop): the pairs are aligned whatever ld is, a pair may straddle
// two columns, so each element finds its own cell.  The block's first cell comes from one 64-bit division per block, the
// thread's from a 32-bit one.  One partial per block, folded in block order: the same bits in every run.
__global__ void __launch_bounds__(SB)
k_dot_cellweighted(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ coef, int jterm,
                   int nf, int ld, int64_t n, double *partials)
{
    __shared__ double red[4];
    const int64_t e0 = (int64_t)blockIdx.x * (2 * SB);          // first element of this block
    const int64_t cb = e0 / ld;
    const uint32_t off = (uint32_t)(e0 - cb * ld) + 2u * threadIdx.x;   // < ld + 2 SB
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        const double2 xv = reinterpret_cast<const double2 *>(x)[i], yv = reinterpret_cast<const double2 *>(y)[i];
        const uint32_t dc = off / (uint32_t)ld;
        int64_t c = cb + dc;
        int t = (int)(off - dc * (uint32_t)ld);
        if (t < nf) acc += coef[c * 8 + jterm] * (xv.x * yv.x);
        if (++t == ld) {
            t = 0;
            ++c;
        }
        if (t < nf) acc += coef[c * 8 + jterm] * (xv.y * yv.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0 && (int)((n - 1) % ld) < nf)
        acc += coef[((n - 1) / ld) * 8 + jterm] * (x[n - 1] * y[n - 1]);
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

void launch_integrate_load(const Launch &L, const LevelDev &lv, const MeshDev &mesh, int64_t nsub, const double *v,
                           const double *load, int slot)
{
    const int64_t n = nsub * lv.ld;
    const int64_t nb = stream_blocks(n);
    check_grid(nb);
    if (!v || !load || !mesh.coef) throw std::runtime_error("load pairing: null vector or no operator coefficients on the device");
    hipLaunchKernelGGL(k_dot_cellweighted, dim3((unsigned)nb), dim3(SB), 0, L.stream, v, load, mesh.coef, lv.nterm - 1, lv.nf,
                       (int)lv.ld, n, reduce_target(L, nb));
    check_launch();
    reduce_finish(L, nb, slot);
}

// ---------------------------------------------------------------------------------------------
// right-hand side F(v) = -int a xi . grad v  (ref: src/examples/homogenized_coefficients.jl:449-474)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_rhs_dphi(LevelDev lv, int64_t ncells, const double *__restrict__ pvec, double *b)
{
    const int64_t total = ncells * lv.nf;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i / lv.nf;
        const int t = (int)(i - c * lv.nf);
        const double *d = lv.dphi + 3 * t;
        const double *p = pvec + 3 * c;
        double v = d[0] * p[0];
        v += d[1] * p[1];
        if (lv.dim == 3) v += d[2] * p[2];
        b[c * lv.ld + t] = v;
    }
}

void launch_rhs_dphi(const Launch &L, const LevelDev &lv, int64_t ncells, const double *pvec, double *b)
{
    hipLaunchKernelGGL(k_rhs_dphi, dim3(strided_blocks(L, ncells * lv.nf, 4)), dim3(256), 0, L.stream, lv, ncells, pvec,
                       b);
    check_launch();
}

// ---------------------------------------------------------------------------------------------
// multi-GPU: pack one value per cut DOF (first local copy) / write the summed value to all copies -- faces, edges and
// nodes in ONE launch per direction (29 exchanges per V-cycle: three launches each were 1 ms of launch-bound kernels)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cut_pack(LevelDev lv, CutPackArgs c, double *buf, double *x, int unpack)
{
    const int64_t t0 = c.n[0] * lv.nfi, t1 = t0 + c.n[1] * lv.nei, total = t1 + c.n[2];
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int kind = idx < t0 ? 0 : idx < t1 ? 1 : 2;
        const int per = kind == 0 ? lv.nfi : kind == 1 ? lv.nei : 1;
        const int off = kind == 0 ? lv.off_face : kind == 1 ? lv.off_edge : 0;
        const int64_t r = idx - (kind == 0 ? 0 : kind == 1 ? t0 : t1);
        const int64_t e = r / per;
        const int k = (int)(r - e * per);
        const int32_t v = c.cell_lid[kind][e];
        double *a = x + (int64_t)(v >> 3) * lv.ld + off + (v & 7) * per + k;
        double *b = buf + c.pos[kind][e] + k;
        if (unpack)
            *a = *b;
        else if (c.first[kind][e])
            *b = *a;
    }
}

void launch_cut_pack(const Launch &L, const LevelDev &lv, const CutPackArgs &c, double *buf, double *x, int unpack)
{
    const int64_t total = c.n[0] * lv.nfi + c.n[1] * lv.nei + c.n[2];
    if (total == 0) return;
    hipLaunchKernelGGL(k_cut_pack, dim3(strided_blocks(L, total, 1)), dim3(256), 0, L.stream, lv, c, buf, x, unpack);
    check_launch();
}

// plan: nseg, then per segment (offset, size, members, offset of its member table); member table: staging offset of every
// member in ascending rank order, -1 for this rank
__global__ void __launch_bounds__(256) k_seg_sum(const int64_t *__restrict__ plan, int64_t total, double *buf,
                                                 const double *__restrict__ stage)
{
    const int nseg = (int)plan[0];
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int sgi = 0;
        while (sgi + 1 < nseg && idx >= plan[1 + 4 * (sgi + 1)]) ++sgi;        // (a few dozen segments at most)
        const int64_t off = plan[1 + 4 * sgi], d = idx - off;
        const int nm = (int)plan[3 + 4 * sgi];
        const int64_t *mt = plan + plan[4 + 4 * sgi];
        double acc = 0.0;
        for (int m = 0; m < nm; ++m) {
            const int64_t so = mt[m];
            const double v = so < 0 ? buf[idx] : stage[so + d];
            acc = m == 0 ? v : acc + v;
        }
        buf[idx] = acc;
    }
}

void launch_seg_sum(const Launch &L, const int64_t *plan, int64_t ndoubles, double *buf, const double *stage)
{
    if (ndoubles == 0) return;
    hipLaunchKernelGGL(k_seg_sum, dim3(strided_blocks(L, ndoubles, 1)), dim3(256), 0, L.stream, plan, ndoubles, buf, stage);
    check_launch();
}

}  // namespace hmg
