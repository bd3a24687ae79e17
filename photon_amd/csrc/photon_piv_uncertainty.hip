// photon_piv_uncertainty.hip - a posteriori uncertainty of a displacement vector from correlation statistics (Wieneke
// 2015): one windowed reduction per vector over the matched (mutually warped) image pair.
// Definition: include/parallel_ray_tracing.h, section 11; host model: photon_amd/piv_uncertainty.py (uncertainty_model).
//
// One workgroup of 256 threads (4 waves) per window, all arithmetic in f64 on the f32 pixels.  The two raw tiles sit in
// LDS as f32; A = a - mean a and B = b - mean b are formed on the fly.  d_x and d_y are staged as f64 tiles with KP zero
// columns on either side (KP = K rounded up to even) and K zero rows below, so that a read at p + Delta needs no bounds
// test and the cells outside the pixel set P (the last column of d_x, the last row of d_y) contribute 0: the sums over
// "p and p + Delta both in P" become sums over every pixel.  Since
//   V = S(0) + 2 sum_H S(Delta) = sum_p d(p) (d(p) + 2 sum_H d(p + Delta)),
// a pixel costs |H_K| adds and two multiply-adds per axis.  A thread owns two pixels side by side (an even column and the
// next) and reads, per row offset, the K + 1 (K odd: K + 2) aligned 16-byte pairs that cover both pixels' neighbours:
// ds_read_b128 at constant offsets from one address (K is a template parameter), 3 reads instead of 10 per row at K = 2.
// The pairs are read as 16-byte vectors on purpose: left to itself the compiler fuses scalar f64 reads of neighbouring
// columns into ds_read_b128 / ds_read2_b64 at addresses that are only 8-byte aligned, which the LDS replays.
// LDS banks (ds_read_b128: four groups of 16 lanes, 64 banks of 4 bytes): a wave walks whole rows of pairs (win 64: two
// rows, win 32: four, win 16: eight).  32 contiguous pairs are conflict-free at any pitch (win 64: pitch win + 2 KP).
// At win 32 a group of 16 lanes spans two rows: conflict-free when the pitch is 0 (mod 32) f64 -- 64; at win 16 four
// rows: conflict-free when the pitch is 16 (mod 32) f64 -- 48.
// (Derived from the bank rule of the lane groups; not confirmed with a counter run.)
// Every sum has a fixed order (per thread in pixel order, a butterfly inside each wave, the wave totals in wave order):
// two calls on the same inputs return the same bits.  No atomics, no device scratch.
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_grid.hpp"

using namespace photon;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRedDoubles = 4 * kWaves;     // block-reduction scratch: at most 4 values per wave (block_reduce asserts it)
constexpr int kMaxReach = 4;

typedef double v2d __attribute__((ext_vector_type(2)));

struct SumOp {
    __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
struct MinOp {
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct MaxOp {
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};

// Fixed-order block reduction of N values: a butterfly inside each wave (every lane ends with the same bits), then the
// wave totals in wave order.  Every thread returns with the block's values.
template <int N, typename Op>
__device__ __forceinline__ void block_reduce(double (&v)[N], double *red, Op op) {
    static_assert(N * kWaves <= kRedDoubles, "the reduction scratch holds kRedDoubles values");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int n = 0; n < N; n++) v[n] = op(v[n], __shfl_xor(v[n], o, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int n = 0; n < N; n++) red[w * N + n] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) {
        double t = red[n];
        for (int i = 1; i < kWaves; i++) t = op(t, red[i * N + n]);
        v[n] = t;
    }
}

template <int WIN, int K>
struct Layout {
    static constexpr int kPad = (K + 1) / 2 * 2;                     // zero columns left and right of the pixels: K, rounded up to even
    static constexpr int kPitch = WIN == 16 ? 48 : WIN == 32 ? 64 : WIN + 2 * kPad;      // f64 per row (the banks: see the head of the file)
    static constexpr int kRows = WIN + K;
    static constexpr int kCells = kRows * kPitch;
    static constexpr size_t kBytes = sizeof(double) * (2 * kCells + kRedDoubles) + sizeof(float) * 2 * WIN * WIN;
};

// sigma of one axis from its four sums (section 11); raises bits 16 and 32 in `flag`
__device__ __forceinline__ float sigma_of(double C0, double C1, double S00, double V, int &flag) {
    if (!(V >= 0.0)) {
        V = S00;
        flag |= 32;
    }
    const double s = sqrt(V), lo = C1 - s / 2.0, hi = C1 + s / 2.0;
    double num, den;
    if (lo > 0.0 && C0 > 0.0) {
        const double llo = log(lo), lhi = log(hi);
        num = lhi - llo;
        den = (4.0 * log(C0) - 2.0 * llo) - 2.0 * lhi;
    } else {
        num = hi - lo;
        den = 4.0 * (C0 - C1);
    }
    if (den > 0.0) return (float)(num / den);
    flag |= 16;
    return __builtin_nanf("");
}

// LDS (bytes, in this order): d_x [kRows][kPitch] f64 | d_y the same | reduction scratch f64 | a [WIN][WIN] f32 | b the same.
// Pixel (r, q) of a d tile sits at row r, column q + kPad: an even column at a 16-byte boundary.
template <int WIN, int K>
__global__ __launch_bounds__(kThreads) void piv_uncertainty_kernel(const float *__restrict__ im1, const float *__restrict__ im2, int W,
                                                                   int step, int n_cols, float *__restrict__ sigma,
                                                                   int *__restrict__ flags, double *__restrict__ stats) {
    using L = Layout<WIN, K>;
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    double *sdx = lds64;
    double *sdy = sdx + L::kCells;
    double *red = sdy + L::kCells;
    float *sa = reinterpret_cast<float *>(red + kRedDoubles);
    float *sb = sa + WIN * WIN;

    const int win_id = blockIdx.x, tid = threadIdx.x;
    const size_t wy0 = (size_t)(win_id / n_cols) * step, wx0 = (size_t)(win_id % n_cols) * step;

    // ---- the raw tiles, their sums, their smallest and largest pixel
    double sums[2] = {0.0, 0.0}, mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int i = tid; i < WIN * WIN; i += kThreads) {
        const size_t g = (wy0 + i / WIN) * W + wx0 + i % WIN;
        const float va = im1[g], vb = im2[g];
        sa[i] = va;
        sb[i] = vb;
        sums[0] += (double)va;
        sums[1] += (double)vb;
        mn[0] = fmin(mn[0], (double)va);
        mx[0] = fmax(mx[0], (double)va);
        mn[1] = fmin(mn[1], (double)vb);
        mx[1] = fmax(mx[1], (double)vb);
    }
    block_reduce(sums, red, SumOp());
    block_reduce(mn, red, MinOp());
    block_reduce(mx, red, MaxOp());           // (the barriers also publish sa and sb)

    if (mn[0] == mx[0] || mn[1] == mx[1]) {     // flat (block-uniform): all pixels of a equal, or all of b
        if (tid == 0) {
            sigma[2 * (size_t)win_id + 0] = __builtin_nanf("");
            sigma[2 * (size_t)win_id + 1] = __builtin_nanf("");
            flags[win_id] = 2;
        }
        if (stats && tid < 8) stats[8 * (size_t)win_id + tid] = __builtin_nan("");
        return;
    }
    const double ma = sums[0] / (double)(WIN * WIN), mb = sums[1] / (double)(WIN * WIN);

    // ---- d_x, d_y over the padded tiles (0 off their pixel sets) and the four correlation sums
    double c[4] = {0.0, 0.0, 0.0, 0.0};         // 2 C0x, 2 C1x, 2 C0y, 2 C1y
    for (int i = tid; i < L::kCells; i += kThreads) {
        const int r = i / L::kPitch, q = i % L::kPitch - L::kPad;
        double dx = 0.0, dy = 0.0;
        if (r < WIN && q >= 0 && q < WIN) {
            const int p = r * WIN + q;
            const double A = (double)sa[p] - ma, B = (double)sb[p] - mb;
            if (q < WIN - 1) {
                const double Ae = (double)sa[p + 1] - ma, Be = (double)sb[p + 1] - mb;
                const double u = A * Be, v = Ae * B;
                dx = u - v;
                c[0] += A * B + Ae * Be;
                c[1] += u + v;
            }
            if (r < WIN - 1) {
                const double Ae = (double)sa[p + WIN] - ma, Be = (double)sb[p + WIN] - mb;
                const double u = A * Be, v = Ae * B;
                dy = u - v;
                c[2] += A * B + Ae * Be;
                c[3] += u + v;
            }
        }
        sdx[i] = dx;
        sdy[i] = dy;
    }
    block_reduce(c, red, SumOp());             // (the barriers also publish the d tiles)

    // ---- S(0) and V per axis: sum_p d(p) d(p), sum_p d(p) (d(p) + 2 sum_H d(p + Delta)); two pixels (r, q) and (r, q + 1) per step
    double s[4] = {0.0, 0.0, 0.0, 0.0};         // S00x, Vx, S00y, Vy
    constexpr int KP = L::kPad, NV = 2 * KP + 2;        // v[m] is column q - KP + m: the two pixels at m = KP, KP + 1
    for (int i = tid; i < WIN * WIN / 2; i += kThreads) {
        const int at = (i / (WIN / 2)) * L::kPitch + 2 * (i % (WIN / 2));          // v[0]: KP columns left of pixel (r, q), q = 2 (i % (WIN / 2))
        double e[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, n[2][2] = {{0.0, 0.0}, {0.0, 0.0}};      // [axis][pixel]
#pragma unroll
        for (int axis = 0; axis < 2; axis++) {
            const double *base = (axis == 0 ? sdx : sdy) + at;
#pragma unroll
            for (int dr = 0; dr <= K; dr++) {
                double v[NV];
#pragma unroll
                for (int m = 0; m < NV; m += 2) {
                    // a pair no neighbour of this row offset needs is not read
                    const bool used = dr > 0 ? (m + 1 >= KP - K && m <= KP + 1 + K) : (m + 1 >= KP && m <= KP + 1 + K);
                    const v2d t = used ? *reinterpret_cast<const v2d *>(base + dr * L::kPitch + m) : v2d{0.0, 0.0};
                    v[m] = t.x;
                    v[m + 1] = t.y;
                }
                if (dr == 0) {
                    e[axis][0] = v[KP];
                    e[axis][1] = v[KP + 1];
                }
#pragma unroll
                for (int dq = -K; dq <= K; dq++)
                    if (dr > 0 || dq > 0) {
                        n[axis][0] += v[KP + dq];
                        n[axis][1] += v[KP + 1 + dq];
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            s[0] += e[0][j] * e[0][j];
            s[1] += e[0][j] * (e[0][j] + 2.0 * n[0][j]);
            s[2] += e[1][j] * e[1][j];
            s[3] += e[1][j] * (e[1][j] + 2.0 * n[1][j]);
        }
    }
    block_reduce(s, red, SumOp());

    if (tid == 0) {
        const double C0x = 0.5 * c[0], C1x = 0.5 * c[1], C0y = 0.5 * c[2], C1y = 0.5 * c[3];
        int f = 0;
        sigma[2 * (size_t)win_id + 0] = sigma_of(C0x, C1x, s[0], s[1], f);
        sigma[2 * (size_t)win_id + 1] = sigma_of(C0y, C1y, s[2], s[3], f);
        flags[win_id] = f;
        if (stats) {
            double *o = stats + 8 * (size_t)win_id;
            o[0] = C0x, o[1] = C1x, o[2] = s[0], o[3] = s[1];
            o[4] = C0y, o[5] = C1y, o[6] = s[2], o[7] = s[3];
        }
    }
}

template <int WIN, int K>
int launch(const float *im1, const float *im2, int W, int step, int n_rows, int n_cols, float *sigma, int *flags, double *stats,
           hipStream_t stream) {
    constexpr size_t bytes = Layout<WIN, K>::kBytes;
    PH_TRY(piv_grid::reserve_lds(piv_uncertainty_kernel<WIN, K>, bytes, "photon_piv_uncertainty", WIN, "reach", K));
    hipLaunchKernelGGL((piv_uncertainty_kernel<WIN, K>), dim3((unsigned)(n_rows * n_cols)), dim3(kThreads), bytes, stream, im1, im2, W, step,
                       n_cols, sigma, flags, stats);
    PH_CHECK(hipGetLastError());
    return 0;
}

template <int WIN>
int launch_reach(int reach, const float *im1, const float *im2, int W, int step, int n_rows, int n_cols, float *sigma, int *flags,
                 double *stats, hipStream_t stream) {
    switch (reach) {
    case 0: return launch<WIN, 0>(im1, im2, W, step, n_rows, n_cols, sigma, flags, stats, stream);
    case 1: return launch<WIN, 1>(im1, im2, W, step, n_rows, n_cols, sigma, flags, stats, stream);
    case 2: return launch<WIN, 2>(im1, im2, W, step, n_rows, n_cols, sigma, flags, stats, stream);
    case 3: return launch<WIN, 3>(im1, im2, W, step, n_rows, n_cols, sigma, flags, stats, stream);
    default: return launch<WIN, 4>(im1, im2, W, step, n_rows, n_cols, sigma, flags, stats, stream);
    }
}

}  // namespace

extern "C" int photon_piv_uncertainty(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int reach,
                                      float *d_sigma, int *d_flags, double *d_stats, int *n_rows, int *n_cols, void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (reach < 0 || reach > kMaxReach)) bad = "reach must lie in [0, 4]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && d_sigma && !d_flags) bad = "d_sigma without d_flags";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_uncertainty: %s (win %d, step %d, reach %d, %d x %d image)\n", bad, win, step, reach, width, height);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_uncertainty", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_sigma) return 0;                     // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto WIN) {
        return launch_reach<WIN()>(reach, d_im1, d_im2, width, step, rows, cols, d_sigma, d_flags, d_stats, stream);
    });
}
