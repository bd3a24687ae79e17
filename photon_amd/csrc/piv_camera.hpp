// piv_camera.hpp - what the camera-mapped PIV units share (include/parallel_ray_tracing.h, sections 19 to 21): where a grid
// node lands on a sensor, the voxel-per-thread launch shape, and the host-side argument rules.  Users: photon_piv_stereo.hip
// (dewarp_kernel), photon_piv_tomo.hip (los_kernel), photon_piv_mart.hip (mart_kernel): a line-of-sight slice is a dewarp and
// the update gathers where the projection scattered because the same function runs.  Host models: photon_amd/piv_stereo.py.
// The 16-tap B-spline sampler behind sensor_point is piv_warp.hpp's BsplineTaps, shared with section 7b's warp.
#pragma once
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_grid.hpp"
#include "piv_warp.hpp"

namespace photon {
namespace piv_camera {

constexpr int kMaxCameras = 8;
constexpr int kFrameChunk = 4;      // frames that share one coordinate evaluation per camera and node

// the bivariate cubic of section 19a in its fixed Horner order; k: 1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3
static __device__ __forceinline__ double cubic(const double *k, double u, double v) {
    const double a0 = ((k[9] * v + k[5]) * v + k[2]) * v + k[0];
    const double a1 = (k[8] * v + k[4]) * v + k[1];
    const double a2 = k[7] * v + k[3];
    return ((k[6] * u + a2) * u + a1) * u + a0;
}

struct SensorPoint { int ix, iy; float fx, fy; };       // floor(x), floor(y); x - floor(x), y - floor(y)

// Node (i, j) of a grid on a W x H sensor.  poly: the camera folded at the node's plane, f64[2][10] (kernel arguments or
// global memory alike); grid: u0, du, v0, dv.  false: the node is outside the sensor (a NaN is outside) and p is not written.
static __device__ __forceinline__ bool sensor_point(const double *poly, const double *grid, int i, int j, int W, int H, SensorPoint &p) {
    const double u = grid[0] + (double)j * grid[1], v = grid[2] + (double)i * grid[3];
    const double x = cubic(poly, u, v), y = cubic(poly + 10, u, v);
    if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1))) return false;
    // the absolute coordinate never enters a float: the fraction is taken in f64 and rounded once
    const double x0 = floor(x), y0 = floor(y);
    p.ix = (int)x0, p.iy = (int)y0;
    p.fx = (float)(x - x0), p.fy = (float)(y - y0);
    return true;
}

// tap t = 2 a + b is the pixel row[a] + col[b] with the weight w[t]: (y0, x0), (y0, x1), (y1, x0), (y1, x1).  The projection
// scatters with these weights and the update gathers with them: a matched pair.
struct Footprint {
    size_t row[2];      // y0 W, y1 W
    int col[2];         // x0, x1 = min(x0 + 1, W - 1)
    float w[4];         // wy wx, in f32, nothing fused
    __device__ __forceinline__ size_t pixel(int t) const { return row[t >> 1] + (size_t)col[t & 1]; }
};

// sensor_point's arguments and result; fp is not written where the camera does not see the node
static __device__ __forceinline__ bool footprint(const double *poly, const double *grid, int i, int j, int W, int H, Footprint &fp) {
    SensorPoint p;
    if (!sensor_point(poly, grid, i, j, W, H, p)) return false;
    const float gx = 1.0f - p.fx, gy = 1.0f - p.fy;
    fp.col[0] = p.ix, fp.col[1] = min(p.ix + 1, W - 1);
    fp.row[0] = (size_t)p.iy * W, fp.row[1] = (size_t)min(p.iy + 1, H - 1) * W;
    fp.w[0] = gy * gx, fp.w[1] = gy * p.fx, fp.w[2] = p.fy * gx, fp.w[3] = p.fy * p.fx;
    return true;
}

// the voxel-per-thread launch shape of los_kernel and mart_kernel
struct VoxelGrid {
    int nx, ny, nz, col_blocks, row_blocks;
    static VoxelGrid make(const photon_piv_volume_t &vol) {
        return {vol.nx, vol.ny, vol.nz, (vol.nx + piv_warp::kWarpX - 1) / piv_warp::kWarpX, (vol.ny + piv_warp::kWarpY - 1) / piv_warp::kWarpY};
    }
    // of kWarpX x kWarpY threads; below 2^31: nx ny nz <= INT_MAX, sides <= 2^22
    unsigned blocks() const { return (unsigned)((long long)col_blocks * row_blocks * nz); }
    // this thread's voxel (slice k, row i, column j) and its offset o in the volume; false: the thread is beyond the slice
    __device__ __forceinline__ bool voxel(int &i, int &j, int &k, size_t &o) const {
        const int cb = blockIdx.x % col_blocks, rest = blockIdx.x / col_blocks;
        const int rb = rest % row_blocks;
        k = rest / row_blocks;
        j = cb * piv_warp::kWarpX + threadIdx.x, i = rb * piv_warp::kWarpY + threadIdx.y;
        if (j >= nx || i >= ny) return false;
        o = ((size_t)k * ny + i) * nx + j;
        return true;
    }
};

// ---- host: the argument rules of sections 19 to 21
inline bool all_finite(const double *v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the bytes of n blocks of `stride` elements; a null pointer with n = 0 overlaps nothing
struct Range { const char *lo; size_t bytes; };
inline Range range_of(const void *p, size_t element, long long stride, int n) { return {reinterpret_cast<const char *>(p), element * (size_t)stride * (size_t)n}; }
inline bool overlap(const Range &a, const Range &b) { return a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes; }

// What sections 20a, 21a and 21b share, in pieces: each entry point tests them in its own order between its own rules, so a
// job that breaks two rules gets the message it always got.  Behind cameras_error every c < n_cameras is a camera.
inline const char *cameras_error(int n_cameras) { return n_cameras < 2 || n_cameras > kMaxCameras ? "n_cameras must be within [2, 8]" : nullptr; }
inline const char *frames_error(int n_frames) { return n_frames < 1 ? "n_frames must be >= 1" : nullptr; }
// stride_below: the message in the entry point's own name for the stride, "out_stride is below nx ny nz"
inline const char *volume_error(const photon_piv_volume_t &vol, long long stride, const char *stride_below) {
    const char *bad = piv_grid::side_error(vol.nx, vol.ny);
    if (!bad) bad = piv_grid::side_error(vol.nz, vol.nz);
    if (bad) return bad;
    if ((long long)vol.nx * vol.ny * vol.nz > INT_MAX) return "nx ny nz is above INT_MAX";
    return stride < (long long)vol.nx * vol.ny * vol.nz ? stride_below : nullptr;
}
inline const char *grid_values_error(const double *grid) { return all_finite(grid, 4) ? nullptr : "a grid value is not finite"; }

inline bool camera_ok(const photon_piv_camera_t &c) {
    return all_finite(c.centre, 3) && all_finite(c.scale, 3) && all_finite(c.cx, 19) && all_finite(c.cy, 19) && c.scale[0] != 0.0 &&
           c.scale[1] != 0.0 && c.scale[2] != 0.0;
}

// section 19b's and 19c's plane and camera pair
inline const char *plane_cameras_error(const photon_piv_plane_t &pl, const photon_piv_camera_t &camera1, const photon_piv_camera_t &camera2) {
    if (!(std::isfinite(pl.x0) && std::isfinite(pl.y0) && std::isfinite(pl.z) && std::isfinite(pl.pitch))) return "a plane value is not finite";
    if (!(pl.pitch > 0.0)) return "pitch must be > 0";
    if (!camera_ok(camera1) || !camera_ok(camera2)) return "a camera value is not finite, or a scale is 0";
    return nullptr;
}

}  // namespace piv_camera
}  // namespace photon
