// Point evaluation of a level vector (hmg_grid_locate, hmg_sample, hmg_sample_raster): ONE text for the host loop of
// hmg_sample.cpp and for the kernel of hmg_sample.hip -- physical point -> coarse cell -> fine element -> dim + 1 storage slots
// with P1 weights, and the element's gradient.
//
// Cell.  The locator is a uniform bin grid over the bounding box of the current cells; a bin lists, ascending, the cells that may
// meet it.  Per cell 'geo' holds X0 (dim) and A = J^-1 (dim x dim, row-major): x^ = A (x - X0) are the reference coordinates, and
// with lambda_0 = 1 - sum x^ the barycentric ones.  A point is inside when all are >= -SAMPLE_TAU; the first cell of the bin's
// list that says so is the lowest cell id that does.
//
// Element.  In the lattice coordinates of a level (slot_ijk = m x^, m = 2^(level-1)) the fine elements are the Kuhn simplices of
// the basis a = (0,0,1), b = (0,1,-1), c = (1,-1,0) (2D: a = (0,1), b = (1,-1); ElementTables::dirs, checked by the host before
// anything here runs).  The coordinates in that basis are cumulative sums, Y = (t_i + t_j + t_k, t_i + t_j, t_i) (2D: (t_i + t_j,
// t_i)), and the cell is m >= Y_0 >= Y_1 >= Y_2 >= 0, a union of Kuhn simplices.  With P_a = min(floor Y_a, m - 1) and
// f_a = Y_a - P_a in [0, 1] the element is the path P, P + e_p1, P + e_p1 + e_p2, P + (1,1,1), p the order of f descending.
// TIE RULE: equal f in ascending index a (a stable sort).  With it every vertex of the path lies in the cell for every point of
// the closed cell: P is monotone like Y; where P_a = P_b for a < b, f_a >= f_b and a steps first, so Y_a >= Y_b holds along the
// path; and P_0 + 1 <= m by the min.  (That is why f = 1 is allowed: a point with Y_a = m belongs to the last interval.)  The
// weights are 1 - f_p1, f_p1 - f_p2, f_p2 - f_p3, f_p3: exact differences' roundings, never negative.
// ZERO WEIGHTS: a vertex whose weight is exactly 0 is not read for the value; the element's gradient reads all its vertices.
//
// Rounding.  Every multiply-add whose rounding decides an output is an explicit fma and the rest is compiled without contraction,
// so that host and device, and the point and raster instantiations of the kernel, do not drift apart.
#pragma once
#include "hmg_device.hpp"

#ifndef HMG_HD
#define HMG_HD __host__ __device__ __forceinline__
#endif

namespace hmg {

constexpr double SAMPLE_TAU = 0x1p-40;   // slack of the inside test, in reference (barycentric) coordinates

// device (or host) view of a grid's locator
struct SampleLocator {
    int nb[3];                  // bins per axis (1 on the axes a 2D grid does not have)
    double lo[3], hi[3];        // the box the bins cover: the cells' bounding box grown by the slack; outside it no cell is looked for
    double inv_h[3];            // bins per unit length
    const int32_t *bin_ptr;     // [nbins + 1]
    const int32_t *bin_cell;    // per bin its candidate cells, ascending
    const double *geo;          // per cell dim + dim * dim doubles: X0, then A = J^-1 row-major
};

// lattice -> storage slot of one level
struct SampleLevel {
    int m, nf, ld, nei, off_int;
    const int32_t *slot_of;     // 3D: slot of lattice node (i, j, k) at (k (m + 1) + j) (m + 1) + i; 2D: null (rows_slot)
};

template <int DIM>
struct SampleElement {
    int slot[DIM + 1];          // storage slots of the path's vertices (all inside the cell)
    double w[DIM + 1];          // P1 weights
    int perm[DIM];              // the basis index each step of the path adds
};

HMG_HD int sample_bin(const SampleLocator &L, int a, double x)
{
#pragma clang fp contract(off)
    const int b = (int)floor((x - L.lo[a]) * L.inv_h[a]);
    return b < 0 ? 0 : b >= L.nb[a] ? L.nb[a] - 1 : b;
}

// reference coordinates of x in the cell with this geometry; true: inside (the -tau slack included)
template <int DIM>
HMG_HD bool sample_in_cell(const double *geo, const double *x, double *xh)
{
#pragma clang fp contract(off)
    double d[DIM];
    for (int a = 0; a < DIM; ++a) d[a] = x[a] - geo[a];
    const double *A = geo + DIM;
    double l0 = 1.0;
    bool in = true;
    for (int b = 0; b < DIM; ++b) {
        double v = A[b * DIM] * d[0];
        for (int a = 1; a < DIM; ++a) v = __builtin_fma(A[b * DIM + a], d[a], v);
        xh[b] = v;
        l0 -= v;
        in = in && v >= -SAMPLE_TAU;
    }
    return in && l0 >= -SAMPLE_TAU;
}

// the lowest cell that contains x, or -1 (a coordinate that is not finite compares false)
template <int DIM>
HMG_HD int sample_find_cell(const SampleLocator &L, const double *x, double *xh)
{
    int bin = 0;
    for (int a = DIM - 1; a >= 0; --a) {
        if (!(x[a] >= L.lo[a] && x[a] <= L.hi[a])) return -1;
        bin = bin * L.nb[a] + sample_bin(L, a, x[a]);
    }
    const int q1 = L.bin_ptr[bin + 1];
    for (int q = L.bin_ptr[bin]; q < q1; ++q) {
        const int c = L.bin_cell[q];
        if (sample_in_cell<DIM>(L.geo + (size_t)c * (DIM + DIM * DIM), x, xh)) return c;
    }
    return -1;
}

template <int DIM>
HMG_HD int sample_slot(const SampleLevel &lv, const int *P)
{
    // lattice node of basis coordinates P: i = P_last, j = P_(last-1) - P_last, (k = P_0 - P_1)
    if (DIM == 2) {
        int cls;
        return rows_slot(lv.m, P[1], P[0] - P[1], lv.nei, lv.off_int, cls);
    }
    const int m1 = lv.m + 1, i = P[DIM - 1], j = P[DIM - 2] - P[DIM - 1], k = P[0] - P[1];
    return lv.slot_of[(k * m1 + j) * m1 + i];
}

// the fine element of the level that holds the point with reference coordinates xh (inside the cell up to the slack)
template <int DIM>
HMG_HD void sample_element(const SampleLevel &lv, const double *xh, SampleElement<DIM> &E)
{
#pragma clang fp contract(off)
    const double md = (double)lv.m;
    double Y[DIM], acc = 0.0;
    for (int a = 0; a < DIM; ++a) {
        acc += (xh[a] > 0.0 ? xh[a] : 0.0) * md;     // (m is a power of two: the product is exact)
        Y[DIM - 1 - a] = acc;
    }
    if (Y[0] > md) Y[0] = md;
    for (int a = 1; a < DIM; ++a)
        if (Y[a] > Y[a - 1]) Y[a] = Y[a - 1];
    int P[DIM];
    double f[DIM];
    for (int a = 0; a < DIM; ++a) {
        int p = (int)Y[a];
        if (p > lv.m - 1) p = lv.m - 1;
        P[a] = p;
        f[a] = Y[a] - (double)p;                     // exact
        E.perm[a] = a;
    }
    for (int i = 1; i < DIM; ++i)                    // stable insertion sort, f descending
        for (int j = i; j > 0 && f[E.perm[j]] > f[E.perm[j - 1]]; --j) {
            const int t = E.perm[j];
            E.perm[j] = E.perm[j - 1];
            E.perm[j - 1] = t;
        }
    E.w[0] = 1.0 - f[E.perm[0]];
    for (int q = 1; q < DIM; ++q) E.w[q] = f[E.perm[q - 1]] - f[E.perm[q]];
    E.w[DIM] = f[E.perm[DIM - 1]];
    for (int q = 0; q <= DIM; ++q) {
        E.slot[q] = sample_slot<DIM>(lv, P);
        if (q < DIM) P[E.perm[q]] += 1;
    }
}

// sum of w_k v_k over the vertices with a weight, then xi . x (xi may be null)
template <int DIM>
HMG_HD double sample_value(const SampleElement<DIM> &E, const double *v, const double *xi, const double *x)
{
    double acc = 0.0;
    for (int q = 0; q <= DIM; ++q)
        if (E.w[q] != 0.0) acc = __builtin_fma(E.w[q], v[q], acc);
    if (xi)
        for (int a = 0; a < DIM; ++a) acc = __builtin_fma(xi[a], x[a], acc);
    return acc;
}

// xi + gradient of the P1 interpolant with vertex values v on the element: the differences along the path are the derivatives
// along the basis, d/dt_a = sum of those over b <= DIM - 1 - a, and grad = m A^T d/dt
template <int DIM>
HMG_HD void sample_gradient(const SampleLevel &lv, const SampleElement<DIM> &E, const double *geo, const double *v, const double *xi,
                            double *grad)
{
#pragma clang fp contract(off)
    double gY[DIM], dt[DIM];
    for (int q = 0; q < DIM; ++q) gY[E.perm[q]] = v[q + 1] - v[q];
    double acc = 0.0;
    for (int b = 0; b < DIM; ++b) {
        acc += gY[b];
        dt[DIM - 1 - b] = acc * (double)lv.m;
    }
    const double *A = geo + DIM;
    for (int k = 0; k < DIM; ++k) {
        double s = A[k] * dt[0];
        for (int a = 1; a < DIM; ++a) s = __builtin_fma(A[a * DIM + k], dt[a], s);
        grad[k] = xi ? s + xi[k] : s;
    }
}

// ---- grids on a torus (hmg_grid_set_periodic_sampling) ----------------------------------------------------------------------
// The locator's box is [0, period[a]) per axis, fixed by the period alone; a cell's X0 is its first vertex reduced into that box
// and A comes from its unwrapped edges.  A point is reduced into the box for the bin lookup only; whether it lies in a cell is
// asked of the minimal image of x - X0, which is the only image that can: every point of a cell lies within half a period of the
// cell's first vertex on each axis.  A hit is therefore a hit on the torus, and the lists carry no image code.  xi . x is taken at
// the caller's point (sample_value is handed that one), so u = xi . x + v grows across periods while v repeats.

// x reduced into the box, x - P floor(x / P) per axis; false: a coordinate is not finite.  The rounding of x / P next to a whole
// number of periods can leave the difference just below 0: it gets one period more.  (A result that rounds to P stays; sample_bin
// clamps it into the last bin, whose lists hold the images that reach P.)
template <int DIM>
HMG_HD bool sample_wrap(const double *period, const double *x, double *xr)
{
#pragma clang fp contract(off)
    bool finite = true;
    for (int a = 0; a < DIM; ++a) {
        const double P = period[a];
        double r = x[a] - P * floor(x[a] / P);
        if (r < 0.0) r += P;
        xr[a] = r;
        finite = finite && r >= 0.0 && r <= P;       // (NaN and inf compare false)
    }
    return finite;
}

// sample_in_cell on a torus: x - X0 by the minimal image
template <int DIM>
HMG_HD bool sample_in_cell_torus(const double *geo, const double *period, const double *x, double *xh)
{
#pragma clang fp contract(off)
    double d[DIM];
    for (int a = 0; a < DIM; ++a) {
        d[a] = x[a] - geo[a];
        d[a] -= period[a] * rint(d[a] / period[a]);
    }
    const double *A = geo + DIM;
    double l0 = 1.0;
    bool in = true;
    for (int b = 0; b < DIM; ++b) {
        double v = A[b * DIM] * d[0];
        for (int a = 1; a < DIM; ++a) v = __builtin_fma(A[b * DIM + a], d[a], v);
        xh[b] = v;
        l0 -= v;
        in = in && v >= -SAMPLE_TAU;
    }
    return in && l0 >= -SAMPLE_TAU;
}

// the lowest cell that contains xr (a point of the box: sample_wrap) on the torus; -1 only where the lists fail the point
template <int DIM>
HMG_HD int sample_find_cell_torus(const SampleLocator &L, const double *period, const double *xr, double *xh)
{
    int bin = 0;
    for (int a = DIM - 1; a >= 0; --a) bin = bin * L.nb[a] + sample_bin(L, a, xr[a]);
    const int q1 = L.bin_ptr[bin + 1];
    for (int q = L.bin_ptr[bin]; q < q1; ++q) {
        const int c = L.bin_cell[q];
        if (sample_in_cell_torus<DIM>(L.geo + (size_t)c * (DIM + DIM * DIM), period, xr, xh)) return c;
    }
    return -1;
}

}  // namespace hmg
