// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// The four streaming passes of the V-cycle-preconditioned flexible CG (hmg_fcg.cpp) over the Nf x Ne storage of the top level:
//   k_fcg_dot_zq       z.q                                   16 B/DOF
//   k_fcg_direction    p = z + beta p                        24 B/DOF   (first step: p = z, 16 B/DOF)
//   k_fcg_dots_pq_pr   p.q and p.R in one pass               24 B/DOF
//   k_fcg_update       x += alpha p, R -= alpha q            48 B/DOF
// alpha and beta are formed on the device from device-resident scalars; the host never reads one inside a step.
//
// Launch shape: that of the streaming kernels of hmg_kernels.hip (measured there, profiles/r02_stream_variants.txt) -- one
// double2 (16 bytes) per thread and vector, 256-thread blocks, as many blocks as there are pairs, no grid-stride loop: the
// dispatcher hands the blocks out in order, so the resident blocks sweep one contiguous window through every stream.
// The storage is a prefix of the columns (a shrunk grid passes its current length) and may be empty (a rank without cells: one
// block that touches nothing and leaves zero partials).
// Reductions: one partial per block and dot product, folded by 256 blocks over contiguous ranges, then by one block -- a
// fixed order, the same bits on every run.
#include "hmg_fcg.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

namespace {

constexpr int FB = 256;   // threads per block

__global__ void __launch_bounds__(FB)
k_fcg_dot_zq(const double *__restrict__ z, const double *__restrict__ q, int64_t n, double *__restrict__ part)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        const double2 zv = reinterpret_cast<const double2 *>(z)[i], qv = reinterpret_cast<const double2 *>(q)[i];
        acc = __builtin_fma(zv.x, qv.x, acc);
        acc = __builtin_fma(zv.y, qv.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc = __builtin_fma(z[n - 1], q[n - 1], acc);
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ... where the V-cycle left z's last CG updates pending (option lazy_x): z = ((z [+ az p0]) + ax p1) + alpha (r2 + beta p1) formed
// here -- k_cg_x_tail's arithmetic from the saved block it would have read (sc: launch_cg_x_save, hmg_device.hpp XS_*) --, stored, and used in the
// dot product: 48 B/DOF (40 with two updates) instead of the tail's 40 (32) + 16.  XU == 2: three updates, p0 is read.
template <int XU>
__global__ void __launch_bounds__(FB)
k_fcg_dot_zq_x(double *z, const double *__restrict__ p1, const double *__restrict__ p0, const double *__restrict__ r2,
               const double *__restrict__ sc, const double *__restrict__ q, int64_t n, double *__restrict__ part)
{
    __shared__ double red[4];
    const double alpha = sc[XS_ALPHA] / sc[XS_ONE];
    const double ax = sc[XS_PREV_NUM] / sc[XS_PREV_DEN];
    const double beta = sc[XS_BETA_NUM] / sc[XS_BETA_DEN];
    const double az = XU == 2 ? sc[XS_FIRST_NUM] / sc[XS_FIRST_DEN] : 0.0;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        double2 zv = reinterpret_cast<double2 *>(z)[i];
        const double2 pv = reinterpret_cast<const double2 *>(p1)[i], rv = reinterpret_cast<const double2 *>(r2)[i],
                      qv = reinterpret_cast<const double2 *>(q)[i];
        if (XU == 2) {
            const double2 ov = reinterpret_cast<const double2 *>(p0)[i];
            zv.x = axpy1(az, ov.x, zv.x);
            zv.y = axpy1(az, ov.y, zv.y);
        }
        zv.x = xupd2(ax, beta, alpha, zv.x, pv.x, rv.x);
        zv.y = xupd2(ax, beta, alpha, zv.y, pv.y, rv.y);
        reinterpret_cast<double2 *>(z)[i] = zv;
        acc = __builtin_fma(zv.x, qv.x, acc);
        acc = __builtin_fma(zv.y, qv.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double zl = xupd2(ax, beta, alpha, XU == 2 ? axpy1(az, p0[n - 1], z[n - 1]) : z[n - 1], p1[n - 1], r2[n - 1]);
        z[n - 1] = zl;
        acc = __builtin_fma(zl, q[n - 1], acc);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// beta = -(z.q) / (p.q)_prev; a vanishing (p.q)_prev means the iteration had already arrived: the old direction is dropped
__global__ void __launch_bounds__(FB)
k_fcg_direction(double *p, const double *__restrict__ z, int64_t n, const double *__restrict__ bank, double *fs, int first)
{
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (first) {
        if (i < (n >> 1)) reinterpret_cast<double2 *>(p)[i] = reinterpret_cast<const double2 *>(z)[i];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (n & 1) p[n - 1] = z[n - 1];
            fs[F_BETA] = 0.0;
        }
        return;
    }
    const double zq = bank[FB_ZQ], pq = fs[F_PQ];
    const double beta = pq != 0.0 ? -zq / pq : 0.0;
    if (i < (n >> 1)) {
        double2 *p2 = reinterpret_cast<double2 *>(p);
        const double2 zv = reinterpret_cast<const double2 *>(z)[i];
        double2 pv = p2[i];
        pv.x = axpy1(beta, pv.x, zv.x);
        pv.y = axpy1(beta, pv.y, zv.y);
        p2[i] = pv;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n & 1) p[n - 1] = axpy1(beta, p[n - 1], z[n - 1]);
        fs[F_BETA] = beta;
    }
}

__global__ void __launch_bounds__(FB)
k_fcg_dots_pq_pr(const double *__restrict__ p, const double *__restrict__ q, const double *__restrict__ R, int64_t n,
                 double *__restrict__ part)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double aq = 0.0, ar = 0.0;
    if (i < (n >> 1)) {
        const double2 pv = reinterpret_cast<const double2 *>(p)[i], qv = reinterpret_cast<const double2 *>(q)[i],
                      rv = reinterpret_cast<const double2 *>(R)[i];
        aq = __builtin_fma(pv.x, qv.x, aq);
        aq = __builtin_fma(pv.y, qv.y, aq);
        ar = __builtin_fma(pv.x, rv.x, ar);
        ar = __builtin_fma(pv.y, rv.y, ar);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        aq = __builtin_fma(p[n - 1], q[n - 1], aq);
        ar = __builtin_fma(p[n - 1], R[n - 1], ar);
    }
    const double sq = block_sum(aq, red);
    const double sr = block_sum(ar, red);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = sq;
        part[2 * (int64_t)blockIdx.x + 1] = sr;
    }
}

// alpha = (p.R) / (p.q); p.q = 0 only for p = 0 (the operator is positive definite on the constrained space): nothing to add
__global__ void __launch_bounds__(FB)
k_fcg_update(double *x, double *R, const double *__restrict__ p, const double *__restrict__ q, int64_t n,
             const double *__restrict__ bank, double *fs)
{
    const double pq = bank[FB_PQ], pr = bank[FB_PR];
    const double alpha = pq != 0.0 ? pr / pq : 0.0;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 *r2 = reinterpret_cast<double2 *>(R);
        const double2 pv = reinterpret_cast<const double2 *>(p)[i], qv = reinterpret_cast<const double2 *>(q)[i];
        double2 xv = x2[i], rv = r2[i];
        xv.x = axpy1(alpha, pv.x, xv.x);
        xv.y = axpy1(alpha, pv.y, xv.y);
        rv.x = axpy1(-alpha, qv.x, rv.x);
        rv.y = axpy1(-alpha, qv.y, rv.y);
        x2[i] = xv;
        r2[i] = rv;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n & 1) {
            x[n - 1] = axpy1(alpha, p[n - 1], x[n - 1]);
            R[n - 1] = axpy1(-alpha, q[n - 1], R[n - 1]);
        }
        fs[F_ALPHA] = alpha;
        fs[F_PQ] = pq;
        fs[F_PR] = pr;
    }
}

// part[NV * b + v], b < nb  ->  fold[256 * v + blockIdx.x]: block j sums the contiguous range of blocks it owns
template <int NV>
__global__ void __launch_bounds__(FB) k_fcg_fold(const double *__restrict__ part, int64_t nb, double *__restrict__ fold)
{
    __shared__ double red[4];
    const int64_t per = (nb + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    for (int v = 0; v < NV; ++v) {
        double a = 0.0;
        for (int64_t b = b0 + threadIdx.x; b < b1; b += FB) a += part[NV * b + v];
        const double s = block_sum(a, red);
        if (threadIdx.x == 0) fold[256 * v + blockIdx.x] = s;
    }
}

template <int NV>
__global__ void __launch_bounds__(FB) k_fcg_final(const double *__restrict__ fold, double *out)
{
    __shared__ double red[4];
    for (int v = 0; v < NV; ++v) {
        const double s = block_sum(fold[256 * v + threadIdx.x], red);
        if (threadIdx.x == 0) out[v] = s;
    }
}

void check_blocks(int64_t nb)
{
    if (nb > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
}

template <int NV>
void reduce(const FcgLaunch &F, int64_t nb, int slot)
{
    hipLaunchKernelGGL(k_fcg_fold<NV>, dim3(256), dim3(FB), 0, F.stream, F.part, nb, F.fold);
    check_launch();
    hipLaunchKernelGGL(k_fcg_final<NV>, dim3(1), dim3(FB), 0, F.stream, F.fold, F.bank + slot);
    check_launch();
}

}  // namespace

int64_t fcg_blocks(int64_t n)
{
    const int64_t b = ((n >> 1) + FB - 1) / FB;
    return b < 1 ? 1 : b;
}

void launch_fcg_dot_zq(const FcgLaunch &F, const double *z, const double *q, int64_t n)
{
    const int64_t nb = fcg_blocks(n);
    check_blocks(nb);
    hipLaunchKernelGGL(k_fcg_dot_zq, dim3((unsigned)nb), dim3(FB), 0, F.stream, z, q, n, F.part);
    check_launch();
    reduce<1>(F, nb, FB_ZQ);
}

void launch_fcg_dot_zq_x(const FcgLaunch &F, double *z, const XUpdates &u, const double *q, int64_t n)
{
    // (the kernel reads the saved block at its own places: u is what saved_updates() makes of a record)
    if (!z || !u.p1 || !u.r2 || !u.scal || !q || (u.count == 3) != (u.p0 != nullptr))
        throw std::runtime_error("flexible CG: pending updates of z without their vectors");
    const int64_t nb = fcg_blocks(n);
    check_blocks(nb);
    if (u.p0)
        hipLaunchKernelGGL(k_fcg_dot_zq_x<2>, dim3((unsigned)nb), dim3(FB), 0, F.stream, z, u.p1, u.p0, u.r2, u.scal, q, n, F.part);
    else
        hipLaunchKernelGGL(k_fcg_dot_zq_x<1>, dim3((unsigned)nb), dim3(FB), 0, F.stream, z, u.p1, u.p0, u.r2, u.scal, q, n, F.part);
    check_launch();
    reduce<1>(F, nb, FB_ZQ);
}

void launch_fcg_direction(const FcgLaunch &F, double *p, const double *z, int64_t n, int first)
{
    const int64_t nb = fcg_blocks(n);
    check_blocks(nb);
    hipLaunchKernelGGL(k_fcg_direction, dim3((unsigned)nb), dim3(FB), 0, F.stream, p, z, n, F.bank, F.fs, first);
    check_launch();
}

void launch_fcg_dots_pq_pr(const FcgLaunch &F, const double *p, const double *q, const double *R, int64_t n)
{
    const int64_t nb = fcg_blocks(n);
    check_blocks(nb);
    hipLaunchKernelGGL(k_fcg_dots_pq_pr, dim3((unsigned)nb), dim3(FB), 0, F.stream, p, q, R, n, F.part);
    check_launch();
    static_assert(FB_PR == FB_PQ + 1, "p.q and p.R are summed over the ranks in one call");
    reduce<2>(F, nb, FB_PQ);
}

void launch_fcg_update(const FcgLaunch &F, double *x, double *R, const double *p, const double *q, int64_t n)
{
    const int64_t nb = fcg_blocks(n);
    check_blocks(nb);
    hipLaunchKernelGGL(k_fcg_update, dim3((unsigned)nb), dim3(FB), 0, F.stream, x, R, p, q, n, F.bank, F.fs);
    check_launch();
}

}  // namespace hmg
