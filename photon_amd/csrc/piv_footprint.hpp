// piv_footprint.hpp - where a voxel lands on a camera (include/parallel_ray_tracing.h, section 21): section 20a's coordinate
// pipeline -- the camera folded at the voxel's slice, the f64 Horner, the inside test -- and behind it four bilinear taps with
// their f32 weights.  The projection scatters with these weights and the update gathers with them: a matched pair.
// Host model: photon_amd/piv_mart.py, footprint.
#pragma once
#include "photon_internal.hpp"

namespace photon {
namespace piv_footprint {

// section 19a's bivariate cubic in its fixed Horner order (photon_piv_stereo.hip's, photon_piv_tomo.hip's)
static __device__ __forceinline__ double cubic(const double *k, double u, double v) {
    const double a0 = ((k[9] * v + k[5]) * v + k[2]) * v + k[0];
    const double a1 = (k[8] * v + k[4]) * v + k[1];
    const double a2 = k[7] * v + k[3];
    return ((k[6] * u + a2) * u + a1) * u + a0;
}

// tap t = 2 a + b is the pixel row[a] + col[b] with the weight w[t]: (y0, x0), (y0, x1), (y1, x0), (y1, x1)
struct Footprint {
    size_t row[2];      // y0 W, y1 W
    int col[2];         // x0, x1 = min(x0 + 1, W - 1)
    float w[4];         // wy wx, in f32, nothing fused
    __device__ __forceinline__ size_t pixel(int t) const { return row[t >> 1] + (size_t)col[t & 1]; }
};

// poly: the camera folded at this slice, f64[2][10]; grid: u0, du, v0, dv.  false: the camera does not see the voxel (a NaN is
// outside) and fp is not written.
static __device__ __forceinline__ bool footprint(const double *poly, const double *grid, int i, int j, int W, int H, Footprint &fp) {
    const double u = grid[0] + (double)j * grid[1], v = grid[2] + (double)i * grid[3];
    const double x = cubic(poly, u, v), y = cubic(poly + 10, u, v);
    if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1))) return false;
    // the absolute coordinate never enters a float: the fraction is taken in f64 and rounded once
    const double x0 = floor(x), y0 = floor(y);
    const float fx = (float)(x - x0), fy = (float)(y - y0);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const int ix = (int)x0, iy = (int)y0;
    fp.col[0] = ix, fp.col[1] = min(ix + 1, W - 1);
    fp.row[0] = (size_t)iy * W, fp.row[1] = (size_t)min(iy + 1, H - 1) * W;
    fp.w[0] = gy * gx, fp.w[1] = gy * fx, fp.w[2] = fy * gx, fp.w[3] = fy * fx;
    return true;
}

}  // namespace piv_footprint
}  // namespace photon
