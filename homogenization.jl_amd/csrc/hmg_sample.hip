// k_sample: a level vector evaluated at points (hmg_sample) or on the pixels of a raster slice (hmg_sample_raster), one thread
// per point.  A thread forms or loads its point, looks up its bin and walks the bin's candidate cells in ascending order until
// one contains the point (on a raster the lanes of a wave mostly share bin and cell: the walk is close to wave-uniform and the
// geometry rows come from the cache), decomposes the reference coordinates into a fine element and its P1 weights
// (hmg_sample_device.hpp: the text the host runs in hmg_grid_locate), gathers the dim + 1 vertex values from
// column[cell * ld + slot] -- the vertices without a weight only when the gradient is wanted -- and stores value, gradient and
// cell, each only if wanted.  The cell's geometry row is read once per candidate and once more for the gradient, never per
// vertex.  No LDS, no atomics, no reductions: every point is independent and the results do not depend on the launch shape.
// Raster: a workgroup takes a tile of 16 x 16 pixels (a wave: 16 x 4), so that neighbouring lanes hit neighbouring fine nodes in
// both directions of the slice instead of a run of 256 pixels of one row; a raster thinner than 16 pixels takes thinner tiles.
#include "hmg_sample.hpp"
#include "hmg_stencil.hpp"

namespace hmg {

namespace {

template <int DIM, bool RASTER>
__global__ __launch_bounds__(SAMPLE_NT) void k_sample(const SampleArgs a)
{
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
    double xh[DIM];
    const int cell = sample_find_cell<DIM>(a.loc, x, xh);
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
    if (a.values) a.values[p] = sample_value<DIM>(E, v, xi, x);
    if (a.gradients) {
        double g[DIM];
        sample_gradient<DIM>(a.lev, E, a.loc.geo + (size_t)cell * (DIM + DIM * DIM), v, xi, g);
        for (int c = 0; c < DIM; ++c) a.gradients[p * DIM + c] = g[c];
    }
}

template <int DIM, bool RASTER>
void launch(hipStream_t stream, SampleArgs a)
{
    const int64_t grid = sample_launch_grid(RASTER, a);
    if (grid <= 0) return;
    if (grid * SAMPLE_NT > 0xffffffffll) throw std::runtime_error("k_sample: the launch would exceed 2^32 - 1 threads");
    hipLaunchKernelGGL((k_sample<DIM, RASTER>), dim3((unsigned)grid), dim3(SAMPLE_NT), 0, stream, a);
    check_launch();
}

}  // namespace

void launch_sample(hipStream_t stream, int dim, bool raster, const SampleArgs &a, const double *period)
{
    if (period) {                                // a grid on a torus: k_sample_torus (hmg_sample_torus.hip)
        SampleTorusArgs t{};
        t.s = a;
        for (int k = 0; k < dim; ++k) t.period[k] = period[k];
        launch_sample_torus(stream, dim, raster, t);
        return;
    }
    if (dim == 3)
        raster ? launch<3, true>(stream, a) : launch<3, false>(stream, a);
    else
        raster ? launch<2, true>(stream, a) : launch<2, false>(stream, a);
}

}  // namespace hmg
