// photon_optflow.hip - dense optical flow on an image pair (Horn & Schunck 1981, warped as in Brox et al. 2004): one
// displacement vector per pixel, refined from a predictor that a correlation supplies.  Definition:
// include/parallel_ray_tracing.h, section 12; host model: photon_amd/optical_flow.py.
//
//   field_to_pixels_kernel        one thread per pixel: section 7b's dense displacement of a window grid (GridField of
//                                 piv_warp.hpp, the function the grid warp calls), one 8-byte store
//   deform_kernel<DenseField>     section 7b's warp (piv_warp.hpp) with the displacement read per pixel
//   terms_kernel                  one thread per pixel: the 4th-order derivatives of the pair's mean along the row and the
//                                 column (mirrored), the temporal difference, and the two numbers a sweep needs, one
//                                 16-byte store
//   sweep_kernel<N>               N Jacobi sweeps in one launch.  One workgroup per tile (32 x 32): the tile and a halo of N
//                                 pixels of the field in LDS (ping-pong), the terms of the pixels a thread owns (one
//                                 column, every R-th row) in registers; sweep s updates the staged region shrunk by s
//                                 pixels a side, the last one writes the tile.  Neighbours clamp by image coordinates, so the recomputed halo holds the
//                                 bits N global sweeps would have produced.
// No kernel writes what another workgroup of the same launch reads, and there is no sum whose order could vary: two calls
// on the same inputs return the same bits.
#include <cmath>

#include "photon_internal.hpp"
#include "piv_grid.hpp"
#include "piv_warp.hpp"

using namespace photon;
using namespace photon::piv_warp;

namespace {

__global__ __launch_bounds__(kWarpX *kWarpY) void field_to_pixels_kernel(GridField D, int W, int H, float2 *__restrict__ dense) {
    const int q = blockIdx.x * kWarpX + threadIdx.x, r = blockIdx.y * kWarpY + threadIdx.y;
    if (q >= W || r >= H) return;
    float dx, dy;
    D(r, q, W, dx, dy);
    dense[(size_t)r * W + q] = make_float2(dx, dy);
}

// =============================================================================================
// c. data terms
// =============================================================================================
// (m(-2) - m(+2) + 8 (m(+1) - m(-1))) / 12 of the pair's mean m = (a + b) / 2 along one axis
__device__ __forceinline__ float mean_at(const float *__restrict__ w1, const float *__restrict__ w2, size_t k, float gain) {
    return (gain * w1[k] + gain * w2[k]) * 0.5f;
}
__device__ __forceinline__ float derivative(float m2m, float m1m, float m1p, float m2p) {
    return ((m2m - m2p) + 8.f * (m1p - m1m)) / 12.f;
}

__global__ __launch_bounds__(kWarpX *kWarpY) void terms_kernel(const float *__restrict__ w1, const float *__restrict__ w2, int W, int H,
                                                               const float2 *__restrict__ u0, float gain, float alpha2,
                                                               float4 *__restrict__ terms) {
    const int q = blockIdx.x * kWarpX + threadIdx.x, r = blockIdx.y * kWarpY + threadIdx.y;
    if (q >= W || r >= H) return;
    const size_t row = (size_t)r * W, k = row + q;
    const float ix = derivative(mean_at(w1, w2, row + mirror(q - 2, W), gain), mean_at(w1, w2, row + mirror(q - 1, W), gain),
                                mean_at(w1, w2, row + mirror(q + 1, W), gain), mean_at(w1, w2, row + mirror(q + 2, W), gain));
    const float iy = derivative(mean_at(w1, w2, (size_t)mirror(r - 2, H) * W + q, gain), mean_at(w1, w2, (size_t)mirror(r - 1, H) * W + q, gain),
                                mean_at(w1, w2, (size_t)mirror(r + 1, H) * W + q, gain), mean_at(w1, w2, (size_t)mirror(r + 2, H) * W + q, gain));
    const float it = gain * w2[k] - gain * w1[k];
    const float2 u = u0 ? u0[k] : make_float2(0.f, 0.f);
    const float c = (it - ix * u.x) - iy * u.y;
    const float w = 1.f / ((alpha2 + ix * ix) + iy * iy);
    terms[k] = make_float4(ix, iy, c, w);
}

// =============================================================================================
// d. relaxation
// =============================================================================================
// tile shape and workgroup size: measured choices; the macros exist for the A/B builds of that table
#ifndef PHOTON_OPTFLOW_TILE_X
#define PHOTON_OPTFLOW_TILE_X 32
#endif
#ifndef PHOTON_OPTFLOW_TILE_Y
#define PHOTON_OPTFLOW_TILE_Y 32
#endif
#ifndef PHOTON_OPTFLOW_THREADS
#define PHOTON_OPTFLOW_THREADS 512
#endif
constexpr int kTileX = PHOTON_OPTFLOW_TILE_X, kTileY = PHOTON_OPTFLOW_TILE_Y;      // a workgroup's output tile, pixels
constexpr int kFlowThreads = PHOTON_OPTFLOW_THREADS;
constexpr int kMaxFuse = 8;                 // the most sweeps one launch performs (sweep_kernel<1 .. kMaxFuse>)

// Thread (tx, ty) of the SX x R arrangement owns the staged pixels (tx, ty + k R), k < K: its column, its clamps to the
// left and right and which of its pixels lie in the image are decided once, and a pixel's LDS index is one constant away
// from the last one's.  (Deciding them per pixel from a linear index made the kernel VALU-bound at 40 instructions a pixel.)
template <int N>
__global__ __launch_bounds__(kFlowThreads) void sweep_kernel(const float4 *__restrict__ terms, const float2 *__restrict__ u, int W, int H,
                                                             float2 *__restrict__ out) {
    constexpr int SX = kTileX + 2 * N, SY = kTileY + 2 * N, P = SX * SY;     // the staged rectangle: the tile and its halo
    constexpr int R = kFlowThreads / SX, K = (SY + R - 1) / R;              // rows of threads (the last kFlowThreads - SX R idle), rows per thread
    static_assert(R >= 1 && K <= 32, "the tile is too wide for the workgroup, or too tall for the mask of live rows");
    __shared__ float2 s_u[2][P];            // the staged field: sweep s reads [(s - 1) & 1] and writes [s & 1]
    const int tid = threadIdx.x, ty = tid / SX, tx = tid - ty * SX;
    const int gx = (int)blockIdx.x * kTileX - N + tx, gy0 = (int)blockIdx.y * kTileY - N + ty;
    const bool column_in = ty < R && gx >= 0 && gx < W;
    const int left = gx > 0 ? -1 : 0, right = gx < W - 1 ? 1 : 0;          // neighbours clamp by image coordinates
    float4 t[K];                            // (Ix, Iy, c, w) of the thread's pixels
    unsigned live = 0;                      // bit k: pixel k is staged and inside the image
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int ly = ty + k * R, gy = gy0 + k * R;
        t[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (column_in && ly < SY && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            live |= 1u << k;
            s_u[0][ly * SX + tx] = u[g];
            t[k] = terms[g];
        }
    }
    __syncthreads();
    // LDS byte addresses of the thread's first pixel and of its four neighbours' columns: a pixel's own part (buffer, row
    // k R) is a compile-time constant that the ds instructions carry as their offset
    char *lds = reinterpret_cast<char *>(&s_u[0][0]);
    constexpr int kPix = (int)sizeof(float2);
    const int self = (ty * SX + tx) * kPix;
    const char *at_left = lds + self + left * kPix, *at_right = lds + self + right * kPix;
    const char *at_self = lds + self, *at_up = lds + self - SX * kPix, *at_down = lds + self + SX * kPix;
#pragma unroll
    for (int s = 1; s <= N; s++) {
        constexpr int kBuf = P * kPix;
        const int rd = ((s - 1) & 1) * kBuf, wr = (s & 1) * kBuf;
        const bool column_ok = tx >= s && tx < SX - s;                     // the region of sweep s: s pixels less a side
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int ly = ty + k * R, gy = gy0 + k * R, off = k * R * SX * kPix;
            if (column_ok && (live >> k & 1u) && ly >= s && ly < SY - s) {
                const float2 a = *reinterpret_cast<const float2 *>(at_left + (rd + off)), b = *reinterpret_cast<const float2 *>(at_right + (rd + off));
                const float2 c = *reinterpret_cast<const float2 *>((gy > 0 ? at_up : at_self) + (rd + off));
                const float2 d = *reinterpret_cast<const float2 *>((gy < H - 1 ? at_down : at_self) + (rd + off));
                const float ub = ((a.x + b.x) + (c.x + d.x)) * 0.25f, vb = ((a.y + b.y) + (c.y + d.y)) * 0.25f;
                const float rho = ((t[k].x * ub + t[k].y * vb) + t[k].z) * t[k].w;
                const float2 res = make_float2(ub - t[k].x * rho, vb - t[k].y * rho);
                if (s == N) out[(size_t)gy * W + gx] = res;
                else *reinterpret_cast<float2 *>(lds + self + (wr + off)) = res;
            }
        }
        if (s < N) __syncthreads();
    }
}

template <int N>
void launch_sweeps(const float4 *terms, const float2 *u, int W, int H, float2 *out, hipStream_t stream) {
    const dim3 grid((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((H + kTileY - 1) / kTileY));
    hipLaunchKernelGGL(sweep_kernel<N>, grid, dim3(kFlowThreads), 0, stream, terms, u, W, H, out);
}

void launch_sweeps(int n, const float4 *terms, const float2 *u, int W, int H, float2 *out, hipStream_t stream) {
    switch (n) {
        case 1: return launch_sweeps<1>(terms, u, W, H, out, stream);
        case 2: return launch_sweeps<2>(terms, u, W, H, out, stream);
        case 3: return launch_sweeps<3>(terms, u, W, H, out, stream);
        case 4: return launch_sweeps<4>(terms, u, W, H, out, stream);
        case 5: return launch_sweeps<5>(terms, u, W, H, out, stream);
        case 6: return launch_sweeps<6>(terms, u, W, H, out, stream);
        case 7: return launch_sweeps<7>(terms, u, W, H, out, stream);
        default: return launch_sweeps<kMaxFuse>(terms, u, W, H, out, stream);
    }
}

constexpr int kDefaultFuse = 8;             // measured: DESIGN.md section 4.3i

// T: PHOTON_OPTFLOW_SWEEPS (1 .. kMaxFuse; measurements), else kDefaultFuse.  Read per call, so that one process can time several.
int sweeps_per_launch() {
    const char *e = getenv("PHOTON_OPTFLOW_SWEEPS");
    const int v = e ? atoi(e) : 0;
    return v >= 1 && v <= kMaxFuse ? v : kDefaultFuse;
}

}  // namespace

extern "C" int photon_piv_field_to_pixels(const float *d_field, int field_stride, int n_rows, int n_cols, int win, int step, int width,
                                          int height, float *d_dense, void *stream_p) {
    const char *bad = piv_grid::grid_error(width, height, win, step, n_rows, n_cols);
    if (!bad) {
        if (field_stride != 2 && field_stride != 4) bad = "field_stride must be 2 or 4";
        else if (width > (1 << 22) || height > (1 << 22)) bad = "the image is larger than 2^22 pixels a side";
        else if (!d_field || !d_dense) bad = "null d_field or d_dense";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_field_to_pixels: %s (win %d, step %d, %d x %d image, %d x %d grid, stride %d)\n", bad, win, step,
                width, height, n_rows, n_cols, field_stride);
        return 1;
    }
    const GridField D{d_field, field_stride, n_rows, n_cols, win, step, 1.f / (float)(2 * step)};
    hipLaunchKernelGGL(field_to_pixels_kernel, warp_grid(width, height), dim3(kWarpX, kWarpY), 0, (hipStream_t)stream_p, D, width, height,
                       reinterpret_cast<float2 *>(d_dense));
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_deform_dense(const float *d_coef, int width, int height, const float *d_dense, float scale, float *d_out,
                                       void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (width > (1 << 22) || height > (1 << 22)) bad = "the image is larger than 2^22 pixels a side";
    else if (!std::isfinite(scale)) bad = "scale must be finite";
    else if (!d_coef || !d_dense || !d_out) bad = "null d_coef, d_dense or d_out";
    else if (d_coef == d_out) bad = "d_out must not be d_coef";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_deform_dense: %s (%d x %d image, scale %g)\n", bad, width, height, (double)scale);
        return 1;
    }
    hipLaunchKernelGGL(deform_kernel<DenseField>, warp_grid(width, height), dim3(kWarpX, kWarpY), 0, (hipStream_t)stream_p, d_coef, width, height,
                       DenseField{d_dense}, scale, d_out);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_optflow_terms(const float *d_w1, const float *d_w2, int width, int height, const float *d_u0, float gain, float alpha2,
                                    float *d_terms, void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (!std::isfinite(gain) || !(gain > 0.f)) bad = "gain must be finite and > 0";
    else if (!std::isfinite(alpha2) || !(alpha2 > 0.f)) bad = "alpha2 must be finite and > 0";
    else if (!d_w1 || !d_w2 || !d_terms) bad = "null d_w1, d_w2 or d_terms";
    if (bad) {
        fprintf(stderr, "photon: photon_optflow_terms: %s (%d x %d image, gain %g, alpha2 %g)\n", bad, width, height, (double)gain,
                (double)alpha2);
        return 1;
    }
    hipLaunchKernelGGL(terms_kernel, warp_grid(width, height), dim3(kWarpX, kWarpY), 0, (hipStream_t)stream_p, d_w1, d_w2, width, height,
                       reinterpret_cast<const float2 *>(d_u0), gain, alpha2, reinterpret_cast<float4 *>(d_terms));
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_optflow_iterations_per_launch(void) { return sweeps_per_launch(); }

extern "C" int photon_optflow_iterate(const float *d_terms, const float *d_u, int width, int height, int iterations, float *d_out,
                                      float *d_tmp, void *stream_p) {
    const int T = sweeps_per_launch();
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (iterations < 0) bad = "iterations must be >= 0";
    else if (!d_terms || !d_u || !d_out) bad = "null d_terms, d_u or d_out";
    else if (d_out == d_u) bad = "d_out must not be d_u";
    else if (d_tmp && (d_tmp == d_u || d_tmp == d_out)) bad = "d_tmp must be neither d_u nor d_out";
    else if (!d_tmp && iterations > T) bad = "more iterations than one launch performs need d_tmp";
    if (bad) {
        fprintf(stderr, "photon: photon_optflow_iterate: %s (%d x %d field, %d iterations, %d per launch)\n", bad, width, height, iterations, T);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    if (iterations == 0) {
        PH_CHECK(hipMemcpyAsync(d_out, d_u, (size_t)width * height * 2 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return 0;
    }
    // launches of T sweeps and one of the remainder; they alternate between d_tmp and d_out so that the last one writes d_out
    const int launches = (iterations + T - 1) / T;
    const float2 *src = reinterpret_cast<const float2 *>(d_u);
    for (int l = 0, left = iterations; l < launches; l++) {
        float2 *dst = reinterpret_cast<float2 *>((launches - 1 - l) % 2 == 0 ? d_out : d_tmp);
        const int n = left < T ? left : T;
        launch_sweeps(n, reinterpret_cast<const float4 *>(d_terms), src, width, height, dst, stream);
        PH_CHECK(hipGetLastError());
        src = dst;
        left -= n;
    }
    return 0;
}
