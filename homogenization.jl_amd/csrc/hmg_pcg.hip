// HIP kernels for AMD CDNA4 (gfx950, wave64).
//
// The Jacobi-preconditioned CG smoother (smooth_pcg() in hmg_smooth.cpp) over the Nf x Ne storage of a level:
//   k_operator_diag   cell-local diagonal of lambda M + K_sigma, one     setup, once per operator
//                     32-bit limb of its fixed-point form per launch
//   k_diag_accum      d (+)= summed limb * its weight                     setup
//   k_dinv_finish     0 on constrained entities, else 1 / d               setup
//   k_pcg_start       p = dinv o r, partial of r.p                       24 B/DOF
//   k_pcg_rupdate     r -= alpha Ap, partial of r.(dinv o r)             32 B/DOF
//   k_pcg_xp          x += alpha p_old, p = dinv o r + beta p_old        48 B/DOF
// z = dinv o r is never stored: the passes that need it form it from r and dinv (one rounding, the same in each of them).
// alpha and beta are formed on the device from the context's scalar bank; every vector update is one axpy1.
//
// Launch shape of the streaming passes: that of the CG and FCG kernels (hmg_kernels.hip, hmg_fcg.hip) -- one double2 per thread and
// vector by flat index, 256-thread blocks, as many blocks as there are pairs, no grid-stride loop; a flat pair may straddle two
// columns (dinv has the layout of the vectors, so nothing depends on the column), the last entry of an odd-length vector is
// thread 0's of block 0.  Reductions: one partial per block, folded in a fixed order -- the same bits on every run.
#include "hmg_pcg.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

namespace {

constexpr int PB = 256;   // threads per block

// (the entity class of a storage slot: slot_class(), hmg_device.hpp)

// The assembled diagonal is the interface sum of the cell-local ones.  A floating-point sum depends on the order of its terms, and
// the order differs between an unpartitioned grid (all copies of a node in ascending cell order) and a partitioned one (every rank's
// partial sum, then the ranks): the smoother, and every V-cycle behind it, would depend on the partition in the last bit.  So the
// diagonal is summed in FIXED POINT: a cell-local value d > 0 is the integer floor(d 2^96), cut into DIAG_LIMBS limbs of 32 bits
// (the top one open-ended); each limb travels through the ordinary interface sum as an integer-valued double -- exact in any order
// as long as a node has fewer than 2^21 copies -- and k_diag_accum adds the summed limbs from the top one down with their weights
// 2^(32 k - 96): a handful of roundings of identical numbers in a fixed order.  The same bits on every partition, within 2 ulp of the
// exact sum.  (Bits of d below 2^-96 are dropped; a diagonal entry of 2^53 or more loses the guarantee, not the value.)
constexpr int DIAG_LIMBS = 5;

// the centre tap is w[0] of stencil_eval_v; the products and their order are those of the apply kernels' class weight table
template <int DIM>
__global__ void __launch_bounds__(PB)
k_operator_diag(LevelDev lv, int64_t ncells, const double *__restrict__ coef, double lambda, int limb, double *__restrict__ d)
{
    constexpr int NTERM = DIM == 3 ? 7 : 4;
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= (int64_t)lv.ld * ncells) return;
    const int64_t cell = e / lv.ld;
    const int t = (int)(e - cell * lv.ld);
    double w = 0.0;
    if (t < lv.nf) {
        double s[NTERM];
        cell_scales<DIM>(coef + cell * 8, 1.0, lambda, s);
        const double *c = lv.ctab + (size_t)slot_class(lv, t) * lv.ndir * NTERM;
#pragma unroll
        for (int q = 0; q < NTERM; ++q) w += c[q] * s[q];
        double hi = floor(ldexp(w, 96 - 32 * limb));                      // floor(d 2^96 / 2^(32 limb)): exact scalings of a double
        if (limb < DIAG_LIMBS - 1) hi -= 0x1p32 * floor(hi * 0x1p-32);   // ... mod 2^32: a suffix of hi's mantissa, exact
        w = hi;
    }
    d[e] = w;
}

__global__ void __launch_bounds__(PB)
k_diag_accum(int64_t n, const double *__restrict__ t, double *d, int limb)
{
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= n) return;
    const double v = ldexp(t[e], 32 * limb - 96);
    d[e] = limb == DIAG_LIMBS - 1 ? v : d[e] + v;
}

// bit order of the Dirichlet mask: faces, edges, corners (entity_range in hmg_kernels.hip) = entity class - 1
__global__ void __launch_bounds__(PB)
k_dinv_finish(LevelDev lv, int64_t ncells, const uint16_t *__restrict__ dmask, double *d)
{
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= (int64_t)lv.ld * ncells) return;
    const int64_t cell = e / lv.ld;
    const int t = (int)(e - cell * lv.ld);
    double v = 0.0;
    if (t < lv.nf) {
        const int cls = slot_class(lv, t);
        const bool fixed = cls > 0 && dmask && ((dmask[cell] >> (cls - 1)) & 1u);
        if (!fixed) v = 1.0 / d[e];
    }
    d[e] = v;
}

__global__ void __launch_bounds__(PB)
k_pcg_start(double *__restrict__ p, const double *__restrict__ r, const double *__restrict__ dinv, int64_t n, double *partials)
{
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        const double2 rv = reinterpret_cast<const double2 *>(r)[i], dv = reinterpret_cast<const double2 *>(dinv)[i];
        const double2 zv = make_double2(dv.x * rv.x, dv.y * rv.y);
        reinterpret_cast<double2 *>(p)[i] = zv;
        acc = __builtin_fma(rv.x, zv.x, acc);
        acc = __builtin_fma(rv.y, zv.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double z = dinv[n - 1] * r[n - 1];
        p[n - 1] = z;
        acc = __builtin_fma(r[n - 1], z, acc);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(PB)
k_pcg_rupdate(double *r, const double *__restrict__ q, const double *__restrict__ dinv, int64_t n, const double *__restrict__ scal,
              int s_num, int s_den, double *partials)
{
    __shared__ double red[4];
    const double alpha = scal[s_num] / scal[s_den];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    double acc = 0.0;
    if (i < (n >> 1)) {
        double2 *r2 = reinterpret_cast<double2 *>(r);
        double2 rv = r2[i];
        const double2 qv = reinterpret_cast<const double2 *>(q)[i], dv = reinterpret_cast<const double2 *>(dinv)[i];
        rv.x = axpy1(-alpha, qv.x, rv.x);
        rv.y = axpy1(-alpha, qv.y, rv.y);
        r2[i] = rv;
        acc = __builtin_fma(rv.x, dv.x * rv.x, acc);
        acc = __builtin_fma(rv.y, dv.y * rv.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rv = axpy1(-alpha, q[n - 1], r[n - 1]);
        r[n - 1] = rv;
        acc = __builtin_fma(rv, dinv[n - 1] * rv, acc);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(PB)
k_pcg_xp(double *x, double *p, const double *__restrict__ r, const double *__restrict__ dinv, int64_t n,
         const double *__restrict__ scal, int a_num, int a_den, int b_num, int b_den)
{
    const double alpha = scal[a_num] / scal[a_den];
    const double beta = scal[b_num] / scal[b_den];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < (n >> 1)) {
        double2 *x2 = reinterpret_cast<double2 *>(x);
        double2 *p2 = reinterpret_cast<double2 *>(p);
        double2 xv = x2[i], pv = p2[i];
        const double2 rv = reinterpret_cast<const double2 *>(r)[i], dv = reinterpret_cast<const double2 *>(dinv)[i];
        xv.x = axpy1(alpha, pv.x, xv.x);
        xv.y = axpy1(alpha, pv.y, xv.y);
        pv.x = axpy1(beta, pv.x, dv.x * rv.x);
        pv.y = axpy1(beta, pv.y, dv.y * rv.y);
        x2[i] = xv;
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double pv = p[n - 1];
        x[n - 1] = axpy1(alpha, pv, x[n - 1]);
        p[n - 1] = axpy1(beta, pv, dinv[n - 1] * r[n - 1]);
    }
}

// block partials [nb] -> 256 partials (block j sums the contiguous range of blocks it owns)
__global__ void __launch_bounds__(PB) k_pcg_fold(const double *__restrict__ part, int64_t nb, double *__restrict__ fold)
{
    __shared__ double red[4];
    const int64_t per = (nb + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    double a = 0.0;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += PB) a += part[b];
    const double s = block_sum(a, red);
    if (threadIdx.x == 0) fold[blockIdx.x] = s;
}

__global__ void __launch_bounds__(PB) k_pcg_final(const double *__restrict__ part, int nb, double *scal, int slot)
{
    __shared__ double red[4];
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += PB) a += part[b];
    const double s = block_sum(a, red);
    if (threadIdx.x == 0) scal[slot] = s;
}

int64_t blocks_of(int64_t n)
{
    const int64_t b = ((n >> 1) + PB - 1) / PB;
    if (b > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
    return b < 1 ? 1 : b;
}

// few blocks leave their partials in the small buffer, many in L.rpart (one per 512 entries, sized with the level vectors)
double *partials_of(const Launch &L, int64_t nb)
{
    if (nb <= 2048) return L.partials;
    if (!L.rpart || nb > L.rpart_cap) throw std::runtime_error("reduction scratch too small for this vector");
    return L.rpart;
}

void reduce(const Launch &L, int64_t nb, int slot)
{
    if (nb > 2048) {
        hipLaunchKernelGGL(k_pcg_fold, dim3(256), dim3(PB), 0, L.stream, L.rpart, nb, L.partials);
        check_launch();
        nb = 256;
    }
    hipLaunchKernelGGL(k_pcg_final, dim3(1), dim3(PB), 0, L.stream, L.partials, (int)nb, L.scal, slot);
    check_launch();
}

int64_t entry_blocks(const LevelDev &lv, const MeshDev &mesh)
{
    const int64_t b = ((int64_t)lv.ld * mesh.ncells + PB - 1) / PB;
    if (b > 0x7fffffffLL) throw std::runtime_error("vector too long for one launch");
    return b;
}

}  // namespace

int diag_limbs() { return DIAG_LIMBS; }

void launch_operator_diag(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double lambda, int limb, double *d)
{
    if (limb < 0 || limb >= DIAG_LIMBS) throw std::runtime_error("operator diagonal: limb out of range");
    const int64_t nb = entry_blocks(lv, mesh);
    if (nb == 0) return;
    if (lv.nterm != (lv.dim == 3 ? 7 : 4) || !lv.ctab || !mesh.coef) throw std::runtime_error("operator diagonal: no class table or no operator on this level");
    if (lv.dim == 3)
        hipLaunchKernelGGL(k_operator_diag<3>, dim3((unsigned)nb), dim3(PB), 0, L.stream, lv, mesh.ncells, mesh.coef, lambda, limb, d);
    else
        hipLaunchKernelGGL(k_operator_diag<2>, dim3((unsigned)nb), dim3(PB), 0, L.stream, lv, mesh.ncells, mesh.coef, lambda, limb, d);
    check_launch();
}

void launch_diag_accum(const Launch &L, const LevelDev &lv, const MeshDev &mesh, const double *t, double *d, int limb)
{
    const int64_t nb = entry_blocks(lv, mesh);
    if (nb == 0) return;
    hipLaunchKernelGGL(k_diag_accum, dim3((unsigned)nb), dim3(PB), 0, L.stream, (int64_t)lv.ld * mesh.ncells, t, d, limb);
    check_launch();
}

void launch_dinv_finish(const Launch &L, const LevelDev &lv, const MeshDev &mesh, double *d)
{
    const int64_t nb = entry_blocks(lv, mesh);
    if (nb == 0) return;
    hipLaunchKernelGGL(k_dinv_finish, dim3((unsigned)nb), dim3(PB), 0, L.stream, lv, mesh.ncells, mesh.dmask, d);
    check_launch();
}

void launch_pcg_start(const Launch &L, double *p, const double *r, const double *dinv, int64_t n, int s_out)
{
    const int64_t nb = blocks_of(n);
    hipLaunchKernelGGL(k_pcg_start, dim3((unsigned)nb), dim3(PB), 0, L.stream, p, r, dinv, n, partials_of(L, nb));
    check_launch();
    reduce(L, nb, s_out);
}

void launch_pcg_rupdate(const Launch &L, double *r, const double *q, const double *dinv, int64_t n, Ratio alpha, int s_out)
{
    const int64_t nb = blocks_of(n);
    hipLaunchKernelGGL(k_pcg_rupdate, dim3((unsigned)nb), dim3(PB), 0, L.stream, r, q, dinv, n, L.scal, alpha.num, alpha.den,
                       partials_of(L, nb));
    check_launch();
    reduce(L, nb, s_out);
}

void launch_pcg_xp(const Launch &L, double *x, double *p, const double *r, const double *dinv, int64_t n, Ratio alpha, Ratio beta)
{
    const int64_t nb = blocks_of(n);
    hipLaunchKernelGGL(k_pcg_xp, dim3((unsigned)nb), dim3(PB), 0, L.stream, x, p, r, dinv, n, L.scal, alpha.num, alpha.den, beta.num, beta.den);
    check_launch();
}

}  // namespace hmg
