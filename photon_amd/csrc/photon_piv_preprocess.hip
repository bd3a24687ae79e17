// photon_piv_preprocess.hip - what a PIV / BOS time series gets before it is correlated: the background of a stack of frames
// (per-pixel minimum or mean), and per frame the chain subtract -> clamp -> min-max filter (Westerweel 1993) in one launch.
// Definition: include/parallel_ray_tracing.h, section 15; host models: photon_amd/piv_preprocess.py.
//
// Background: bandwidth-bound.  A lane owns 4 consecutive pixels (one 16-byte load per frame) where the base pointers and the
// frame stride allow it, one pixel otherwise, and folds the frames in ascending order in a plain loop: the compiler's own
// schedule of that loop measured faster than explicit batches of 2 to 16 loads issued together.
// Both forms fold every pixel in the same order: the same bits.
//
// Chain at radius R > 0: one workgroup per 32 x 32 tile.  d is staged on the tile plus 2R around it with the image's edge
// replicated (the minimum over a clipped neighbourhood is the minimum over the replicated one), then four separable passes in
// LDS -- min / max along rows, along columns (0 outside the image: a +0 term changes no sum), box sums along rows, along
// columns -- between two buffers; a lane makes 4 consecutive results of a pass from one run of 2R + 4 values in registers.
// R is a template argument so that those runs are registers; the four d of a lane's own pixels wait in registers too.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "photon_internal.hpp"
#include "piv_grid.hpp"

using namespace photon;

namespace {

constexpr int kThreads = 256;

template <int W>
struct alignas(4 * W) Pack {
    float v[W];
};

// ---- background ------------------------------------------------------------------------------------------------------------
constexpr unsigned kMaxBlocks = 16384;  // the rest by grid stride

// one pixel's value over the frames, in ascending frame order from frame 0's
template <bool MEAN>
struct Fold {
    using T = std::conditional_t<MEAN, double, float>;
    static __device__ T first(float v) { return (T)v; }
    static __device__ T next(T m, float v) {
        if constexpr (MEAN) return m + (double)v;
        else return v < m ? v : m;
    }
    static __device__ float last(T m, int n) {
        if constexpr (MEAN) return (float)(m / (double)n);
        else return m;
    }
};

template <bool MEAN, int W>
__device__ void fold_frames(const float *__restrict__ px, size_t stride, int n, float *__restrict__ out) {
    using F = Fold<MEAN>;
    using V = Pack<W>;
    typename F::T m[W];
    for (int k = 0; k < n; k++) {
        const V u = *reinterpret_cast<const V *>(px + (size_t)k * stride);
#pragma unroll
        for (int c = 0; c < W; c++) m[c] = k == 0 ? F::first(u.v[c]) : F::next(m[c], u.v[c]);
    }
    V r;
#pragma unroll
    for (int c = 0; c < W; c++) r.v[c] = F::last(m[c], n);
    *reinterpret_cast<V *>(out) = r;
}

// VEC: items 0 .. npx/4 - 1 are runs of 4 pixels, the npx mod 4 items after them single pixels; else every item is a pixel
template <bool MEAN, bool VEC>
__global__ __launch_bounds__(kThreads) void piv_background_kernel(const float *__restrict__ frames, long long stride, int n, size_t npx,
                                                                  float *__restrict__ out) {
    const size_t quads = VEC ? npx / 4 : 0, items = quads + (npx - 4 * quads);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (size_t)gridDim.x * kThreads) {
        if (VEC && i < quads) {
            fold_frames<MEAN, 4>(frames + 4 * i, (size_t)stride, n, out + 4 * i);
        } else {
            const size_t p = 4 * quads + (i - quads);
            fold_frames<MEAN, 1>(frames + p, (size_t)stride, n, out + p);
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

bool background_vector_path(const float *d_frames, long long frame_stride, const float *d_out) {
    return aligned16(d_frames) && aligned16(d_out) && frame_stride % 4 == 0;
}

// [a, a + na) and [b, b + nb) floats share an address
bool overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 4 * nb && b0 < a0 + 4 * na;
}

size_t span(long long stride, int n, size_t npx) { return (size_t)(n - 1) * (size_t)stride + npx; }

// ---- the chain -------------------------------------------------------------------------------------------------------------
// max(im - bg, 0) as one subtraction and one select
__device__ float subtracted(float im, float bg) {
    const float x = im - bg;
    return x > 0.f ? x : 0.f;
}

__global__ __launch_bounds__(kThreads) void piv_subtract_kernel(const float *frames, long long stride, int n, size_t npx, const float *__restrict__ bg,
                                                               float *out, long long out_stride) {
    // in place is allowed (frames == out at equal strides): every lane reads its pixel before it writes it
    for (int k = blockIdx.y; k < n; k += gridDim.y)
        for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < npx; p += (size_t)gridDim.x * kThreads)
            out[(size_t)k * (size_t)out_stride + p] = subtracted(frames[(size_t)k * (size_t)stride + p], bg[p]);
}

constexpr int up4(int x) { return (x + 3) / 4 * 4; }

template <int R>
struct Chain {
    static constexpr int T = 32;                        // tile side; T * T / 4 = kThreads: one run of 4 results per lane at the end
    static constexpr int NV = up4(2 * R + 4);           // values a run of 4 results reads, in whole 16-byte loads
    static constexpr int W1 = T + 2 * R;                // side of the tile plus R around it
    // A: d on the tile plus 2R around it.  Pass 1's last run starts at column up4(W1) - 4 and reads NV values.
    static constexpr int a_rows = T + 4 * R, a_cols = T + 4 * R, a_pitch = up4(W1) - 4 + NV;
    static constexpr int a_rounds = (a_rows * a_cols + kThreads - 1) / kThreads;      // pixels a lane stages
    // B: min | max along rows, a_rows x W1 in use; pass 2's last run starts at row up4(W1) - 4 and reads NV rows (the rows
    // past a_rows are never written and feed only rows of C that nobody reads)
    static constexpr int b_rows = up4(W1) - 4 + NV, b_pitch = up4(W1);
    // C: min | max over the square, W1 x W1 in use, 0 outside the image; pass 3's last run starts at column T - 4
    static constexpr int c_rows = up4(W1), c_pitch = T - 4 + NV;
    // D: box sums along rows, W1 x T in use; pass 4's last run starts at row T - 4
    static constexpr int d_rows = T - 4 + NV, d_pitch = T;
    static constexpr int a_size = a_rows * a_pitch, b_size = b_rows * b_pitch, c_size = c_rows * c_pitch, d_size = d_rows * d_pitch;
    static constexpr int P = a_size > 2 * c_size ? a_size : 2 * c_size;         // A, then C
    static constexpr int Q = 2 * (b_size > d_size ? b_size : d_size);           // B, then D
    static constexpr int lds_floats = P + Q;
    static_assert(a_pitch >= a_cols && c_pitch >= W1 && d_rows >= W1 && T * T / 4 == kThreads, "layout");
};

struct Min {
    __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct Max {
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// out[j] = op over a[j .. j + 2R], j < 4: the values all four share once, then three more each (min and max are exact in
// any order)
template <int R, typename Op>
__device__ void run_extreme(const float *a, float *out, Op op) {
    if constexpr (R >= 2) {
        float core = a[3];
#pragma unroll
        for (int i = 4; i <= 2 * R; i++) core = op(core, a[i]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float m = core;
#pragma unroll
            for (int i = j; i < 3; i++) m = op(m, a[i]);
#pragma unroll
            for (int i = 2 * R + 1; i <= 2 * R + j; i++) m = op(m, a[i]);
            out[j] = m;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) out[j] = op(op(a[j], a[j + 1]), a[j + 2]);
    }
}

// out[j] = ((0 + a[j]) + a[j + 1]) + ... + a[j + 2R]: the contract's order, no term shared
template <int R>
__device__ void run_sum(const float *a, float *out) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i <= 2 * R; i++) s = s + a[j + i];
        out[j] = s;
    }
}

template <int NV>
__device__ void load_row(const float *p, float *a) {            // NV floats from a 16-byte aligned LDS address
#pragma unroll
    for (int q = 0; q < NV / 4; q++) {
        const Pack<4> v = reinterpret_cast<const Pack<4> *>(p)[q];
#pragma unroll
        for (int c = 0; c < 4; c++) a[4 * q + c] = v.v[c];
    }
}

template <int NV>
__device__ void load_column(const float *p, int pitch, float *a) {
#pragma unroll
    for (int i = 0; i < NV; i++) a[i] = p[i * pitch];
}

template <int R>
__global__ __launch_bounds__(kThreads) void piv_minmax_kernel(const float *__restrict__ frames, long long stride, int n, int w, int h,
                                                             const float *__restrict__ bg, float floor_, float *__restrict__ out,
                                                             long long out_stride) {
    using L = Chain<R>;
    constexpr int T = L::T, NV = L::NV, W1 = L::W1;
    __shared__ __attribute__((aligned(16))) float lds[L::lds_floats];
    float *const A = lds, *const C = lds;               // C replaces A after pass 1
    float *const B = lds + L::P, *const D = lds + L::P; // D replaces B after pass 2
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * T;
    const int own_x = tid % T, own_y = tid / T * 4;     // the lane's own pixels: column own_x, rows own_y .. own_y + 3 of the tile

    for (int frame = blockIdx.z; frame < n; frame += gridDim.z) {
        const float *im = frames + (size_t)frame * (size_t)stride;
        float *res = out + (size_t)frame * (size_t)out_stride;
        for (int ty0 = blockIdx.y * T; ty0 < h; ty0 += gridDim.y * T) {
            __syncthreads();                            // the tile before has been read
            // every load of the lane before the first use: one round trip to memory per tile, not a_count / kThreads of them.
            // The lanes past the region's end in the last round take its last pixel again (the same value to the same place).
            float v[L::a_rounds], b[L::a_rounds];
#pragma unroll
            for (int q = 0; q < L::a_rounds; q++) {
                const int i = min(tid + q * kThreads, L::a_rows * L::a_cols - 1);
                const int row = i / L::a_cols, col = i % L::a_cols;
                const int gy = min(max(ty0 - 2 * R + row, 0), h - 1), gx = min(max(tx0 - 2 * R + col, 0), w - 1);
                v[q] = im[(size_t)gy * w + gx];
                b[q] = bg ? bg[(size_t)gy * w + gx] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < L::a_rounds; q++) {
                const int i = min(tid + q * kThreads, L::a_rows * L::a_cols - 1);
                A[i / L::a_cols * L::a_pitch + i % L::a_cols] = bg ? subtracted(v[q], b[q]) : v[q];
            }
            __syncthreads();

            float own[4];
#pragma unroll
            for (int j = 0; j < 4; j++) own[j] = A[(2 * R + own_y + j) * L::a_pitch + 2 * R + own_x];
            // pass 1: min, max along rows; B's origin is (ty0 - 2R, tx0 - R)
            for (int t = tid; t < L::a_rows * (L::b_pitch / 4); t += kThreads) {
                const int row = t / (L::b_pitch / 4), x0 = t % (L::b_pitch / 4) * 4;
                float a[NV];
                Pack<4> mn, mx;
                load_row<NV>(A + row * L::a_pitch + x0, a);
                run_extreme<R>(a, mn.v, Min());
                run_extreme<R>(a, mx.v, Max());
                *reinterpret_cast<Pack<4> *>(B + row * L::b_pitch + x0) = mn;
                *reinterpret_cast<Pack<4> *>(B + L::b_size + row * L::b_pitch + x0) = mx;
            }
            __syncthreads();

            // pass 2: along columns; C's origin is (ty0 - R, tx0 - R), 0 outside the image
            for (int t = tid; t < (L::c_rows / 4) * W1; t += kThreads) {
                const int y0 = t / W1 * 4, x = t % W1;
                const int gx = tx0 - R + x;
                float a[NV], m[4];
#pragma unroll
                for (int plane = 0; plane < 2; plane++) {
                    load_column<NV>(B + plane * L::b_size + y0 * L::b_pitch + x, L::b_pitch, a);
                    if (plane == 0) run_extreme<R>(a, m, Min());
                    else run_extreme<R>(a, m, Max());
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int gy = ty0 - R + y0 + j;
                        C[plane * L::c_size + (y0 + j) * L::c_pitch + x] = gy >= 0 && gy < h && gx >= 0 && gx < w ? m[j] : 0.f;
                    }
                }
            }
            __syncthreads();

            // pass 3: box sums along rows; D's origin is (ty0 - R, tx0)
            for (int t = tid; t < 2 * W1 * (T / 4); t += kThreads) {
                const int plane = t / (W1 * (T / 4)), row = t / (T / 4) % W1, x0 = t % (T / 4) * 4;
                float a[NV];
                Pack<4> s;
                load_row<NV>(C + plane * L::c_size + row * L::c_pitch + x0, a);
                run_sum<R>(a, s.v);
                *reinterpret_cast<Pack<4> *>(D + plane * L::d_size + row * L::d_pitch + x0) = s;
            }
            __syncthreads();

            // pass 4: box sums along columns, the means, the lane's four pixels
            float a[NV], lo[4], hi[4];
            load_column<NV>(D + own_y * L::d_pitch + own_x, L::d_pitch, a);
            run_sum<R>(a, lo);
            load_column<NV>(D + L::d_size + own_y * L::d_pitch + own_x, L::d_pitch, a);
            run_sum<R>(a, hi);
            const int gx = tx0 + own_x;
            if (gx < w) {
                const int cols_in = min(gx + R, w - 1) - max(gx - R, 0) + 1;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int gy = ty0 + own_y + j;
                    if (gy < h) {
                        const float cnt = (float)((min(gy + R, h - 1) - max(gy - R, 0) + 1) * cols_in);
                        const float l = lo[j] / cnt, u = hi[j] / cnt;
                        const float num = own[j] - l, range = u - l;
                        res[(size_t)gy * w + gx] = (num > 0.f ? num : 0.f) / (range > floor_ ? range : floor_);
                    }
                }
            }
        }
    }
}

template <int R>
int launch_minmax(const float *frames, long long stride, int n, int w, int h, const float *bg, float floor_, float *out, long long out_stride,
                  hipStream_t stream) {
    constexpr int T = Chain<R>::T;
    const dim3 grid((unsigned)((w + T - 1) / T), (unsigned)std::min((h + T - 1) / T, 65535), (unsigned)std::min(n, 65535));
    hipLaunchKernelGGL(piv_minmax_kernel<R>, grid, dim3(kThreads), 0, stream, frames, stride, n, w, h, bg, floor_, out, out_stride);
    PH_CHECK(hipGetLastError());
    return 0;
}

unsigned blocks_for(size_t items) { return (unsigned)std::min<size_t>((items + kThreads - 1) / kThreads, kMaxBlocks); }

}  // namespace

extern "C" int photon_piv_background_path(const float *d_frames, long long frame_stride, const float *d_out) {
    return background_vector_path(d_frames, frame_stride, d_out) ? 1 : 0;
}

extern "C" int photon_piv_background(const float *d_frames, long long frame_stride, int n_frames, int width, int height, int mode, float *d_out,
                                     void *stream_p) {
    const char *bad = piv_grid::side_error(width, height);
    const size_t npx = bad ? 0 : (size_t)width * (size_t)height;
    if (!bad && (!d_frames || !d_out)) bad = "null pointer";
    if (!bad && n_frames < 1) bad = "n_frames must be >= 1";
    if (!bad && frame_stride < (long long)npx) bad = "frame_stride is smaller than one image";
    if (!bad && mode != 0 && mode != 1) bad = "mode must be 0 (minimum) or 1 (mean)";
    if (!bad && overlap(d_out, npx, d_frames, span(frame_stride, n_frames, npx))) bad = "d_out lies inside the span of the frames";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_background: %s (mode %d, %d x %d image, %d frames %lld apart)\n", bad, mode, width, height, n_frames,
                frame_stride);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const bool vec = background_vector_path(d_frames, frame_stride, d_out);
    const size_t items = vec ? npx / 4 + npx % 4 : npx;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks_for(items)), dim3(kThreads), 0, stream, d_frames, frame_stride, n_frames, npx, d_out);
    };
    if (mode == 0) {
        if (vec) launch(piv_background_kernel<false, true>);
        else launch(piv_background_kernel<false, false>);
    } else {
        if (vec) launch(piv_background_kernel<true, true>);
        else launch(piv_background_kernel<true, false>);
    }
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_preprocess(const float *d_frames, long long frame_stride, int n_frames, int width, int height,
                                     const float *d_background, int radius, float floor, float *d_out, long long out_stride, void *stream_p) {
    const char *bad = piv_grid::side_error(width, height);
    const size_t npx = bad ? 0 : (size_t)width * (size_t)height;
    if (!bad && (!d_frames || !d_out)) bad = "null pointer";
    if (!bad && n_frames < 1) bad = "n_frames must be >= 1";
    if (!bad && (frame_stride < (long long)npx || out_stride < (long long)npx)) bad = "a stride is smaller than one image";
    if (!bad && (radius < 0 || radius > 8)) bad = "radius must lie in [0, 8]";
    if (!bad && radius > 0 && !(std::isfinite(floor) && floor > 0.f)) bad = "floor must be finite and > 0 with radius > 0";
    if (!bad && radius == 0 && !d_background) bad = "radius 0 without a background: nothing to do";
    if (!bad) {
        const size_t in_span = span(frame_stride, n_frames, npx), out_span = span(out_stride, n_frames, npx);
        const bool in_place = radius == 0 && d_out == d_frames && out_stride == frame_stride;
        if (!in_place && overlap(d_out, out_span, d_frames, in_span))
            bad = "d_out overlaps the frames (allowed at radius 0 with d_out == d_frames at equal strides)";
        else if (d_background && overlap(d_out, out_span, d_background, npx))
            bad = "d_out overlaps the background";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_preprocess: %s (radius %d, floor %g, %d x %d image, %d frames %lld apart, out %lld apart)\n", bad,
                radius, (double)floor, width, height, n_frames, frame_stride, out_stride);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    auto minmax = [&](auto R) {
        return launch_minmax<R()>(d_frames, frame_stride, n_frames, width, height, d_background, floor, d_out, out_stride, stream);
    };
    switch (radius) {
    case 0:
        hipLaunchKernelGGL(piv_subtract_kernel, dim3(blocks_for(npx), (unsigned)std::min(n_frames, 65535)), dim3(kThreads), 0, stream, d_frames,
                           frame_stride, n_frames, npx, d_background, d_out, out_stride);
        PH_CHECK(hipGetLastError());
        return 0;
    case 1: return minmax(std::integral_constant<int, 1>());
    case 2: return minmax(std::integral_constant<int, 2>());
    case 3: return minmax(std::integral_constant<int, 3>());
    case 4: return minmax(std::integral_constant<int, 4>());
    case 5: return minmax(std::integral_constant<int, 5>());
    case 6: return minmax(std::integral_constant<int, 6>());
    case 7: return minmax(std::integral_constant<int, 7>());
    default: return minmax(std::integral_constant<int, 8>());
    }
}
