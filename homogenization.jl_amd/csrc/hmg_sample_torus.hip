// k_sample_torus: k_sample (hmg_sample.hip) on a grid on a torus (hmg_grid_set_periodic_sampling), one thread per point.  Launch
// shape, raster tiles, the per-output null checks and the zero-weight rule are k_sample's.  What differs is the way to the cell
// (hmg_sample_device.hpp): the point is reduced into the box [0, period) for the bin lookup, and the inside test of a candidate
// takes x - X0 to its minimal image, one rint and one multiply-subtract per axis and candidate.  A finite point always has a
// cell.  xi . x is taken at the point as the caller gave it, so that a raster over several periods shows u = xi . x + v growing
// while v and the gradient repeat.  The period travels in the argument struct: scalar registers, no load.
// A kernel of its own, so that the four instantiations of k_sample keep their registers and their bits.
#include "hmg_sample.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

namespace {

// Eight waves per SIMD are asked for by name: like k_sample the kernel hides its dependent loads by occupancy alone, and without
// the bound the scheduler spreads the two double divisions per axis over 72 registers in the 3D raster form (7 waves); with it
// every form stays below 50, without scratch or spills (tests/test_sample_torus_kernel_resources.py).
template <int DIM, bool RASTER>
__global__ __launch_bounds__(SAMPLE_NT, 8) void k_sample_torus(const SampleTorusArgs t)
{
    const SampleArgs &a = t.s;
    int64_t p;
    double x[DIM];
    if (RASTER) {
        const int tw = 1 << a.tile_log2w, th = SAMPLE_NT >> a.tile_log2w;
        const int64_t ntx = (a.nu + tw - 1) / tw;
        const int64_t ta = ((int64_t)blockIdx.x % ntx) * tw + (threadIdx.x & (tw - 1));
        const int64_t tb = ((int64_t)blockIdx.x / ntx) * th + (threadIdx.x >> a.tile_log2w);
        if (ta >= a.nu || tb >= a.nv) return;
        p = tb * a.nu + ta;
        for (int c = 0; c < DIM; ++c) x[c] = __builtin_fma((double)tb, a.dv[c], __builtin_fma((double)ta, a.du[c], a.origin[c]));
    } else {
        p = (int64_t)blockIdx.x * SAMPLE_NT + threadIdx.x;
        if (p >= a.npoints) return;
        for (int c = 0; c < DIM; ++c) x[c] = a.points[p * DIM + c];
    }
    double xr[DIM], xh[DIM];
    const int cell = sample_wrap<DIM>(t.period, x, xr) ? sample_find_cell_torus<DIM>(a.loc, t.period, xr, xh) : -1;
    if (a.cell) a.cell[p] = cell;
    if (cell < 0) {
        const double nan = __builtin_nan("");
        if (a.values) a.values[p] = nan;
        if (a.gradients)
            for (int c = 0; c < DIM; ++c) a.gradients[p * DIM + c] = nan;
        return;
    }
    if (!a.values && !a.gradients) return;
    SampleElement<DIM> E;
    sample_element<DIM>(a.lev, xh, E);
    const double *col = a.column + (int64_t)cell * a.lev.ld;
    const bool all = a.gradients != nullptr;
    double v[DIM + 1];
    for (int q = 0; q <= DIM; ++q) v[q] = (all || E.w[q] != 0.0) ? col[E.slot[q]] : 0.0;
    const double *xi = a.has_xi ? a.xi : nullptr;
    if (a.values) a.values[p] = sample_value<DIM>(E, v, xi, x);          // (x: the caller's point, not the reduced one)
    if (a.gradients) {
        double g[DIM];
        sample_gradient<DIM>(a.lev, E, a.loc.geo + (size_t)cell * (DIM + DIM * DIM), v, xi, g);
        for (int c = 0; c < DIM; ++c) a.gradients[p * DIM + c] = g[c];
    }
}

template <int DIM, bool RASTER>
void launch(hipStream_t stream, SampleTorusArgs t)
{
    const int64_t grid = sample_launch_grid(RASTER, t.s);
    if (grid <= 0) return;
    if (grid * SAMPLE_NT > 0xffffffffll) throw std::runtime_error("k_sample_torus: the launch would exceed 2^32 - 1 threads");
    hipLaunchKernelGGL((k_sample_torus<DIM, RASTER>), dim3((unsigned)grid), dim3(SAMPLE_NT), 0, stream, t);
    check_launch();
}

}  // namespace

void launch_sample_torus(hipStream_t stream, int dim, bool raster, const SampleTorusArgs &t)
{
    if (dim == 3)
        raster ? launch<3, true>(stream, t) : launch<3, false>(stream, t);
    else
        raster ? launch<2, true>(stream, t) : launch<2, false>(stream, t);
}

}  // namespace hmg
