// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// The Chebyshev-Jacobi smoother (smooth_cheb() in hmg_smooth.cpp) over the Nf x Ne storage of a level: a Chebyshev polynomial in
// dinv o A on [lambda_hi / ratio, lambda_hi], its coefficients kernel arguments -- no reduction, no scalar bank.
//   k_operator_rowabs  cell-local absolute row sum of lambda M + K_sigma        setup, once per operator
//   k_cheb_max         block maxima of dinv o s                                  setup
//   k_cheb_max_fold    ... folded in a fixed order into one scalar                setup
//   k_cheb_start       d = c0 dinv o r                                           24 B/DOF
//   k_cheb_step        x += d, r -= Ad, d = c1 d + c2 dinv o r                   64 B/DOF
//   k_cheb_tail<0>     x += d                                                    24 B/DOF
//   k_cheb_tail<1>     x += d, r -= Ad                                           48 B/DOF
// z = dinv o r is never stored.  Every vector update is one rounding: x + d and r - Ad are exact sums rounded once, the new d is
// fma(c1, d, c2 * z) with z and c2 * z rounded once each -- the same bits from every form of the tail.
//
// Launch shape of the streaming passes: that of the CG, PCG and FCG kernels -- one double2 per thread and vector by flat index,
// 256-thread blocks, as many blocks as there are pairs, no grid-stride loop; a flat pair may straddle two columns (dinv has the
// layout of the vectors), the last entry of an odd-length vector is thread 0's of block 0.  The maximum is independent of the
// order of its terms: the same bits on every run.
#include "hmg_cheb.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

namespace {

constexpr int PB = 256;   // threads per block

// the products and their order are those of the apply kernels' class weight table, tap by tap (k_operator_diag: the centre tap)
template <int DIM>
__global__ void __launch_bounds__(PB)
k_operator_rowabs(LevelDev lv, int64_t ncells, const double *__restrict__ coef, double lambda, double *__restrict__ s)
{
    constexpr int NTERM = DIM == 3 ? 7 : 4;
    constexpr int NDIR = DIM == 3 ? 15 : 7;
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= (int64_t)lv.ld * ncells) return;
    const int64_t cell = e / lv.ld;
    const int t = (int)(e - cell * lv.ld);
    double sum = 0.0;
    if (t < lv.nf) {
        double sc[NTERM];
        cell_scales<DIM>(coef + cell * 8, 1.0, lambda, sc);
        const double *c = lv.ctab + (size_t)slot_class(lv, t) * NDIR * NTERM;
#pragma unroll
        for (int d = 0; d < NDIR; ++d) {
            double w = 0.0;
#pragma unroll
            for (int q = 0; q < NTERM; ++q) w += c[d * NTERM + q] * sc[q];
            sum += fabs(w);
        }
    }
    s[e] = sum;
}

// The maximum that keeps a NaN: fmax drops one, and a bound folded with it comes back finite from an operator that is not (the
// host's check of the bound could then never fire).  A NaN operand gives a NaN whatever the order of the fold; without one these are
// fmax's bits (the terms are >= 0: no signed zeros to tell apart).
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }

// all threads of the block call; result valid in thread 0.  red: >= blockDim / 64 doubles of LDS
__device__ __forceinline__ double block_max(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double m = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) m = max_nan(m, red[i]);
    }
    __syncthreads();
    return m;
}

__global__ void __launch_bounds__(PB)
k_cheb_max(const double *__restrict__ dinv, const double *__restrict__ s, int64_t n, double *__restrict__ partials)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    double m = 0.0;
    if (i < (n >> 1)) {
        const double2 dv = reinterpret_cast<const double2 *>(dinv)[i], sv = reinterpret_cast<const double2 *>(s)[i];
        m = max_nan(dv.x * sv.x, dv.y * sv.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) m = max_nan(m, dinv[n - 1] * s[n - 1]);
    const double b = block_max(m, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

// block j of the fold takes the contiguous range of partials it owns; one block: the scalar itself
__global__ void __launch_bounds__(PB) k_cheb_max_fold(const double *__restrict__ part, int64_t nb, double *__restrict__ out)
{
    __shared__ double red[4];
    const int64_t per = (nb + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    double m = 0.0;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += PB) m = max_nan(m, part[b]);
    const double r = block_max(m, red);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

__global__ void __launch_bounds__(PB)
k_cheb_start(double *__restrict__ d, const double *__restrict__ r, const double *__restrict__ dinv, int64_t n, double c0)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < (n >> 1)) {
        const double2 rv = reinterpret_cast<const double2 *>(r)[i], dv = reinterpret_cast<const double2 *>(dinv)[i];
        reinterpret_cast<double2 *>(d)[i] = make_double2(c0 * (dv.x * rv.x), c0 * (dv.y * rv.y));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) d[n - 1] = c0 * (dinv[n - 1] * r[n - 1]);
}

__global__ void __launch_bounds__(PB)
k_cheb_step(double *x, double *d, double *r, const double *__restrict__ q, const double *__restrict__ dinv, int64_t n, double c1,
            double c2)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x), *d2 = reinterpret_cast<double2 *>(d), *r2 = reinterpret_cast<double2 *>(r);
        double2 xv = x2[i], pv = d2[i], rv = r2[i];
        const double2 qv = reinterpret_cast<const double2 *>(q)[i], dv = reinterpret_cast<const double2 *>(dinv)[i];
        xv.x = axpy1(1.0, pv.x, xv.x);
        xv.y = axpy1(1.0, pv.y, xv.y);
        rv.x = axpy1(-1.0, qv.x, rv.x);
        rv.y = axpy1(-1.0, qv.y, rv.y);
        pv.x = axpy1(c1, pv.x, c2 * (dv.x * rv.x));
        pv.y = axpy1(c1, pv.y, c2 * (dv.y * rv.y));
        x2[i] = xv;
        r2[i] = rv;
        d2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double pv = d[n - 1];
        const double rv = axpy1(-1.0, q[n - 1], r[n - 1]);
        x[n - 1] = axpy1(1.0, pv, x[n - 1]);
        r[n - 1] = rv;
        d[n - 1] = axpy1(c1, pv, c2 * (dinv[n - 1] * rv));
    }
}

template <int WITH_R>
__global__ void __launch_bounds__(PB)
k_cheb_tail(double *x, const double *__restrict__ d, double *r, const double *__restrict__ q, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 xv = x2[i];
        const double2 pv = reinterpret_cast<const double2 *>(d)[i];
        xv.x = axpy1(1.0, pv.x, xv.x);
        xv.y = axpy1(1.0, pv.y, xv.y);
        x2[i] = xv;
        if (WITH_R) {
            double2 *r2 = reinterpret_cast<double2 *>(r);
            double2 rv = r2[i];
            const double2 qv = reinterpret_cast<const double2 *>(q)[i];
            rv.x = axpy1(-1.0, qv.x, rv.x);
            rv.y = axpy1(-1.0, qv.y, rv.y);
            r2[i] = rv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        x[n - 1] = axpy1(1.0, d[n - 1], x[n - 1]);
        if (WITH_R) r[n - 1] = axpy1(-1.0, q[n - 1], r[n - 1]);
    }
}

int64_t blocks_of(int64_t n)
{
    const int64_t b = ((n >> 1) + PB - 1) / PB;
    if (b > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
    return b < 1 ? 1 : b;
}

}  // namespace

void launch_operator_rowabs(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double lambda, double *s)
{
    const int64_t nb = ((int64_t)lv.ld * mesh.ncells + PB - 1) / PB;
    if (nb > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
    if (nb == 0) return;
    if (lv.nterm != (lv.dim == 3 ? 7 : 4) || lv.ndir != (lv.dim == 3 ? 15 : 7) || !lv.ctab || !mesh.coef)
        throw std::runtime_error("operator row sums: no class table or no operator on this level");
    if (lv.dim == 3)
        hipLaunchKernelGGL(k_operator_rowabs<3>, dim3((unsigned)nb), dim3(PB), 0, L.stream, lv, mesh.ncells, mesh.coef, lambda, s);
    else
        hipLaunchKernelGGL(k_operator_rowabs<2>, dim3((unsigned)nb), dim3(PB), 0, L.stream, lv, mesh.ncells, mesh.coef, lambda, s);
    check_launch();
}

void launch_cheb_max(const Launch &L, const double *dinv, const double *s, int64_t n, int slot)
{
    int64_t nb = blocks_of(n);
    // few blocks leave their maxima in the small buffer, many in L.rpart (one per 512 entries, sized with the level vectors)
    double *part = L.partials;
    if (nb > 2048) {
        if (!L.rpart || nb > L.rpart_cap) throw std::runtime_error("reduction scratch too small for this vector");
        part = L.rpart;
    }
    hipLaunchKernelGGL(k_cheb_max, dim3((unsigned)nb), dim3(PB), 0, L.stream, dinv, s, n, part);
    check_launch();
    if (nb > 2048) {
        hipLaunchKernelGGL(k_cheb_max_fold, dim3(256), dim3(PB), 0, L.stream, L.rpart, nb, L.partials);
        check_launch();
        nb = 256;
    }
    hipLaunchKernelGGL(k_cheb_max_fold, dim3(1), dim3(PB), 0, L.stream, L.partials, nb, L.scal + slot);
    check_launch();
}

void launch_cheb_start(const Launch &L, double *d, const double *r, const double *dinv, int64_t n, double c0)
{
    hipLaunchKernelGGL(k_cheb_start, dim3((unsigned)blocks_of(n)), dim3(PB), 0, L.stream, d, r, dinv, n, c0);
    check_launch();
}

void launch_cheb_step(const Launch &L, double *x, double *d, double *r, const double *Ad, const double *dinv, int64_t n, double c1,
                      double c2)
{
    hipLaunchKernelGGL(k_cheb_step, dim3((unsigned)blocks_of(n)), dim3(PB), 0, L.stream, x, d, r, Ad, dinv, n, c1, c2);
    check_launch();
}

void launch_cheb_tail(const Launch &L, double *x, const double *d, double *r, const double *Ad, int64_t n)
{
    if (Ad)
        hipLaunchKernelGGL(k_cheb_tail<1>, dim3((unsigned)blocks_of(n)), dim3(PB), 0, L.stream, x, d, r, Ad, n);
    else
        hipLaunchKernelGGL(k_cheb_tail<0>, dim3((unsigned)blocks_of(n)), dim3(PB), 0, L.stream, x, d, r, Ad, n);
    check_launch();
}

}  // namespace hmg
