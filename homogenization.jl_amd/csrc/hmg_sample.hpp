// Sampling a level vector at points and on raster slices (hmg_sample, hmg_sample_raster): what the host module (hmg_sample.cpp)
// and the kernel (hmg_sample.hip) share.  The evaluation itself is hmg_sample_device.hpp.
#pragma once
#include "hmg_sample_device.hpp"

namespace hmg {

constexpr int SAMPLE_NT = 256;     // threads per workgroup: a run of 256 points, or a tile of 16 x 16 raster pixels
constexpr int SAMPLE_TILE = 16;    // (a raster thinner than that one way: 2^k pixels that way, 256 / 2^k the other)

struct SampleArgs {
    SampleLocator loc;
    SampleLevel lev;
    const double *column;          // base of the level vector: ld doubles per cell
    double xi[3];
    int has_xi;
    int64_t npoints;               // points, or nu * nv
    const double *points;          // point-major, dim each (device); null on a raster
    double origin[3], du[3], dv[3];
    int64_t nu, nv;
    int tile_log2w;                // set by the launcher (raster): a workgroup's tile is 2^tile_log2w pixels wide, 256 / that high
    double *values;               // [npoints], each output may be null
    double *gradients;             // [npoints * dim]
    int32_t *cell;                 // [npoints]
};

// k_sample_torus (hmg_sample_torus.hip): the same, on a grid on a torus with box lengths period
struct SampleTorusArgs {
    SampleArgs s;
    double period[3];
};

// Launch shape of k_sample and k_sample_torus: the number of workgroups; on a raster it sets a.tile_log2w.
// 16 x 16 pixels per workgroup; a raster thinner than 16 pixels one way takes tiles as thin as it is (a line: 256 x 1): a raster of
// 2^31 - 1 pixels in one line stays a launch of 2^31 threads (square tiles would ask for 2^35), and whatever the shape a raster of
// that many pixels stays below 32 / 17 of them, inside what a launch accepts
inline int64_t sample_launch_grid(bool raster, SampleArgs &a)
{
    if (!raster) return (a.npoints + SAMPLE_NT - 1) / SAMPLE_NT;
    const auto log2_ceil = [](int64_t n) {         // smallest power of two >= n, as its exponent (1 <= n <= 16)
        int e = 0;
        while (((int64_t)1 << e) < n) ++e;
        return e;
    };
    a.tile_log2w = 4;
    if (a.nv < SAMPLE_TILE)
        a.tile_log2w = 8 - log2_ceil(a.nv);
    else if (a.nu < SAMPLE_TILE)
        a.tile_log2w = log2_ceil(a.nu);
    const int64_t tw = (int64_t)1 << a.tile_log2w, th = SAMPLE_NT / tw;
    return ((a.nu + tw - 1) / tw) * ((a.nv + th - 1) / th);
}

// one thread per point; raster = true: the points are formed on the device, a workgroup takes a tile of pixels.
// period != null: a grid on a torus (its box lengths), served by k_sample_torus
void launch_sample(hipStream_t stream, int dim, bool raster, const SampleArgs &a, const double *period);
void launch_sample_torus(hipStream_t stream, int dim, bool raster, const SampleTorusArgs &a);

}  // namespace hmg
