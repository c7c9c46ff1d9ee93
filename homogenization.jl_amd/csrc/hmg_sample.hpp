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

// one thread per point; raster = true: the points are formed on the device, a workgroup takes a tile of pixels
void launch_sample(hipStream_t stream, int dim, bool raster, const SampleArgs &a);

}  // namespace hmg
