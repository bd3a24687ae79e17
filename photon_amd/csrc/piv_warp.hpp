// piv_warp.hpp - the warp of section 7b, shared by the two units that launch it: photon_piv_deform.hip (the displacement
// interpolated from the window grid) and photon_optflow.hip (the displacement read per pixel).  One kernel template over
// where the displacement D of a pixel comes from; everything after D -- the clamp, the taps, the weights, the order of
// the sums -- is the same code, so both forms return the same bits for the same D.
// BsplineTaps, the same taps as a struct, samples for piv_camera.hpp's users (dewarp, line of sight), which reuse them per frame.
#pragma once
#include <cmath>

#include "photon_internal.hpp"

namespace photon {
namespace piv_warp {

// whole-sample mirror of any index into [0, n): ... 2 1 | 0 1 2 ... n-2 n-1 | n-2 n-3 ...
// An index within n - 1 of the image needs one reflection; the division is kept out of line for the others, so that the
// compiler cannot flatten it into the common path (it was 2/3 of the warp's instructions).
static __device__ __noinline__ int mirror_far(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}
static __device__ __forceinline__ int mirror(int i, int n) {
    int m = i < 0 ? -i : i;
    m = m >= n ? 2 * (n - 1) - m : m;
    if (__builtin_expect((unsigned)m >= (unsigned)n, 0)) m = mirror_far(i, n);
    return m;
}

constexpr int kWarpX = 64, kWarpY = 4;
constexpr float kMaxShift = 16777216.f;     // |scale D| is clamped to 2^24 pixels (section 7b)

// node index and weight of the bilinear grid interpolation at a point that lies num / den nodes behind node 0, from the
// exact integers num and den = 2 step: f = clamp(num / den, 0, n - 1), i0 = floor(f) (at most n - 2 when n > 1), w = f - i0.
// The quotient comes from one f32 multiply by inv_den = 1 / den and is corrected by the exact remainder (num < 2^24).
static __device__ __forceinline__ void grid_weight_num(int num, int den, float inv_den, int n, int &i0, int &i1, float &w) {
    if (num <= 0 || n == 1) {
        i0 = i1 = 0;
        w = 0.f;
    } else if ((long long)num >= (long long)(n - 1) * den) {
        i0 = i1 = n - 1;
        w = 0.f;
    } else {
        int q = (int)((float)num * inv_den), r = num - q * den;
        if (r < 0) {
            q--;
            r += den;
        } else if (r >= den) {
            q++;
            r -= den;
        }
        i0 = q;
        i1 = q + 1;
        w = (float)r * inv_den;
    }
}

// at pixel p: (p - (win-1)/2) / step, num = 2p - (win-1)
static __device__ __forceinline__ void grid_weight(int p, int win, int step, float inv_den, int n, int &i0, int &i1, float &w) {
    grid_weight_num(2 * p - (win - 1), 2 * step, inv_den, n, i0, i1, w);
}

// at the centre of window k of another grid (to_win, to_step) on the same image: the half-pixel centres cancel,
// num = (to_win - win) + 2 k to_step (section 16)
static __device__ __forceinline__ void grid_weight_centre(int k, int to_win, int to_step, int win, int step, float inv_den, int n, int &i0,
                                                          int &i1, float &w) {
    grid_weight_num((to_win - win) + 2 * k * to_step, 2 * step, inv_den, n, i0, i1, w);
}

static __device__ __forceinline__ void node(const float *__restrict__ field, int stride, int k, float &dx, float &dy) {
    dx = field[(size_t)k * stride];
    dy = field[(size_t)k * stride + 1];
    if (!(isfinite(dx) && isfinite(dy))) dx = dy = 0.f;
}

// D from the window grid: bilinear in the window-centre coordinates, a vector that is not finite reads as (0, 0)
struct GridField {
    const float *field;
    int stride, n_rows, n_cols, win, step;
    float inv_den;                          // 1 / (2 step)
    // the two-stage interpolation between the nodes (i0, i1) x (j0, j1)
    __device__ __forceinline__ void lerp(int i0, int i1, float wy, int j0, int j1, float wx, float &dx, float &dy) const {
        float ax, ay, bx, by, cx, cy, ex, ey;
        node(field, stride, i0 * n_cols + j0, ax, ay);
        node(field, stride, i0 * n_cols + j1, bx, by);
        node(field, stride, i1 * n_cols + j0, cx, cy);
        node(field, stride, i1 * n_cols + j1, ex, ey);
        const float tx = ax + wx * (bx - ax), ty = ay + wx * (by - ay);    // along the row of nodes i0, then i1, then between
        const float ux = cx + wx * (ex - cx), uy = cy + wx * (ey - cy);
        dx = tx + wy * (ux - tx);
        dy = ty + wy * (uy - ty);
    }
    __device__ __forceinline__ void operator()(int r, int q, int, float &dx, float &dy) const {
        int i0, i1, j0, j1;
        float wy, wx;
        grid_weight(r, win, step, inv_den, n_rows, i0, i1, wy);
        grid_weight(q, win, step, inv_den, n_cols, j0, j1, wx);
        lerp(i0, i1, wy, j0, j1, wx, dx, dy);
    }
    // D at the centre of window (i, j) of the grid (to_win, to_step)
    __device__ __forceinline__ void at_centre(int i, int j, int to_win, int to_step, float &dx, float &dy) const {
        int i0, i1, j0, j1;
        float wy, wx;
        grid_weight_centre(i, to_win, to_step, win, step, inv_den, n_rows, i0, i1, wy);
        grid_weight_centre(j, to_win, to_step, win, step, inv_den, n_cols, j0, j1, wx);
        lerp(i0, i1, wy, j0, j1, wx, dx, dy);
    }
};

// D read per pixel: f32[H W][2]
struct DenseField {
    const float *dense;
    __device__ __forceinline__ void operator()(int r, int q, int W, float &dx, float &dy) const {
        const float2 d = reinterpret_cast<const float2 *>(dense)[(size_t)r * W + q];
        dx = d.x;
        dy = d.y;
    }
};

// cubic B-spline weights of the 4 taps floor(x) - 1 .. floor(x) + 2 at the fraction t
static __device__ __forceinline__ void bspline_weights(float t, float w[4]) {
    const float u = 1.f - t, t2 = t * t, u2 = u * u;
    w[0] = u2 * u * (1.f / 6.f);
    w[1] = (4.f - 3.f * t2 * (2.f - t)) * (1.f / 6.f);
    w[2] = (4.f - 3.f * u2 * (2.f - u)) * (1.f / 6.f);
    w[3] = t2 * t * (1.f / 6.f);
}

// the 16 taps of a cubic B-spline sample around the base pixel (ix, iy): weights and mirrored indices, good for every W x H image
struct BsplineTaps {
    float wx[4], wy[4];
    int xi[4];          // mirrored columns ix - 1 .. ix + 2
    size_t yo[4];       // mirrored rows iy - 1 .. iy + 2, times W
    __device__ __forceinline__ BsplineTaps(int ix, int iy, float fx, float fy, int W, int H) {
        bspline_weights(fx, wx);
        bspline_weights(fy, wy);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            xi[t] = mirror(ix - 1 + t, W);
            yo[t] = (size_t)mirror(iy - 1 + t, H) * W;
        }
    }
    __device__ __forceinline__ float sample(const float *coef) const {
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const float *row = coef + yo[t];
            const float s = ((wx[0] * row[xi[0]] + wx[1] * row[xi[1]]) + wx[2] * row[xi[2]]) + wx[3] * row[xi[3]];
            acc = acc + wy[t] * s;
        }
        return acc;
    }
};

// one thread per output pixel: D, 16 coefficient taps gathered from global memory, one coalesced store
template <typename Field>
__global__ __launch_bounds__(kWarpX *kWarpY) void deform_kernel(const float *__restrict__ coef, int W, int H, Field D, float scale,
                                                                float *__restrict__ out) {
    const int q = blockIdx.x * kWarpX + threadIdx.x, r = blockIdx.y * kWarpY + threadIdx.y;
    if (q >= W || r >= H) return;
    float dx, dy;
    D(r, q, W, dx, dy);
    const float sx = fminf(fmaxf(scale * dx, -kMaxShift), kMaxShift);
    const float sy = fminf(fmaxf(scale * dy, -kMaxShift), kMaxShift);
    // the pixel index never enters a float: the fraction comes from the shift alone
    const float fx = floorf(sx), fy = floorf(sy);
    // BsplineTaps' operations in this kernel's own schedule, a row's mirror between the rows' loads: measured 1 to 2 % faster here
    float wxs[4], wys[4];
    bspline_weights(sx - fx, wxs);
    bspline_weights(sy - fy, wys);
    const int bx0 = q + (int)fx - 1, by0 = r + (int)fy - 1;
    int xi[4];
#pragma unroll
    for (int t = 0; t < 4; t++) xi[t] = mirror(bx0 + t, W);
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const float *row = coef + (size_t)mirror(by0 + u, H) * W;
        const float s = ((wxs[0] * row[xi[0]] + wxs[1] * row[xi[1]]) + wxs[2] * row[xi[2]]) + wxs[3] * row[xi[3]];
        acc = acc + wys[u] * s;
    }
    out[(size_t)r * W + q] = acc;
}

inline dim3 warp_grid(int width, int height) {
    return dim3((unsigned)((width + kWarpX - 1) / kWarpX), (unsigned)((height + kWarpY - 1) / kWarpY));
}

}  // namespace piv_warp
}  // namespace photon
