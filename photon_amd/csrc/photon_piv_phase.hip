// photon_piv_phase.hip - windowed FFT correlation of an image pair on the device: circular cross-correlation (mode 0) and
// robust phase correlation (mode 1).  Definition: include/parallel_ray_tracing.h, section 13; host models:
// photon_amd/piv_phase.py (correlate_phase_model_f32 is this file operation by operation).
//
// One workgroup per window.  z = a' + i b' (both windows, mean-subtracted and weighted) sits in LDS as complex f32 with a row
// pitch of win + 1 elements.  One 2-D transform serves both frames: radix-2 decimation in frequency along the rows, then
// along the columns (natural order in, bit-reversed out, no permutation pass), the spectra separated by symmetry and
// multiplied in place at the bit-reversed positions, then radix-2 decimation in time back (bit-reversed in, natural out).
// In every stage a lane owns one line (a row in the row passes, a column in the column passes) and the waves split the
// butterflies, so the twiddle of an access is the same for all lines and the lanes of an access lie one pitch (rows) or one
// element (columns) apart: with the odd pitch neither walk meets a bank twice.
// Every butterfly is four multiplies and six adds, each rounded on its own (-ffp-contract=off); butterflies of one stage are
// independent, so their schedule does not show in the bits.  The plane stays in LDS for the argmax, the ratio and the fit.
#include <cfloat>
#include <climits>
#include <cmath>

#include "../../include/photon_det_math.h"
#include "photon_internal.hpp"
#include "piv_grid.hpp"
#include "piv_peak.hpp"

using namespace photon;

namespace {

constexpr int kMaxWin = 64;

// The tables of one call, by value in the kernel's arguments (768 bytes): nothing to allocate, nothing to keep alive.
struct PhaseTables {
    float twiddles[kMaxWin];        // [win/2][2] = (cos, -sin)(2 pi k / win)
    float window[kMaxWin];          // g(p)
    float filter[kMaxWin];          // w(k)
};

// f64 values rounded once to f32; the quarter turns exact
void fill_tables(int win, float window_sigma, float diameter, float *twiddles, float *window, float *filter) {
    const double s = (double)window_sigma, d = (double)diameter;
    for (int k = 0; k < win / 2; k++) {
        double sn, cs;
        photon_det_sincos(2.0 * PHOTON_PI * k / win, &sn, &cs);
        twiddles[2 * k] = (float)cs;
        twiddles[2 * k + 1] = (float)(-sn);
    }
    twiddles[0] = 1.f;
    twiddles[1] = 0.f;
    twiddles[2 * (win / 4)] = 0.f;
    twiddles[2 * (win / 4) + 1] = -1.f;
    for (int p = 0; p < win; p++) {
        const double c = p - (win - 1) / 2.0;
        window[p] = s > 0.0 ? (float)photon_det_exp(-(c * c) / (2.0 * s * s)) : 1.f;
        const double f = p < win / 2 ? p : p - win;
        const double u = 2.0 * PHOTON_PI * f / win;
        filter[p] = (float)photon_det_exp(-(d * d / 16.0) * (u * u));
    }
}

// how many of the win pixels from `first` on lie in [0, size)
__device__ __forceinline__ int count_inside(long long first, int win, int size) {
    const long long lo = first < 0 ? -first : 0, hi = (long long)size - first < win ? (long long)size - first : win;
    return hi > lo ? (int)(hi - lo) : 0;
}

// One radix-2 stage of half-size 1 << S over all N lines.  Work item = (line, butterfly), the line in the lane.
template <int N, int B, bool INVERSE, bool COLUMNS>
__device__ __forceinline__ void fft_stage(float2 *z, const float2 *tw, int S, int tid) {
    constexpr int PITCH = N + 1;
    const int h = 1 << S;
    for (int item = tid; item < N * N / 2; item += B) {
        const int line = item % N, q = item / N;
        const int j = q & (h - 1);
        const int i0 = ((q - j) << 1) + j, i1 = i0 + h;
        const float2 t = tw[j * ((N / 2) >> S)];
        const float wr = t.x, wi = INVERSE ? -t.y : t.y;
        const int e0 = COLUMNS ? i0 * PITCH + line : line * PITCH + i0;
        const int e1 = COLUMNS ? i1 * PITCH + line : line * PITCH + i1;
        const float2 u = z[e0], v = z[e1];
        if (INVERSE) {          // decimation in time: (u, v) -> (u + v w, u - v w)
            const float tr = v.x * wr - v.y * wi, ti = v.x * wi + v.y * wr;
            z[e0] = make_float2(u.x + tr, u.y + ti);
            z[e1] = make_float2(u.x - tr, u.y - ti);
        } else {                // decimation in frequency: (u, v) -> (u + v, (u - v) w)
            const float dr = u.x - v.x, di = u.y - v.y;
            z[e0] = make_float2(u.x + v.x, u.y + v.y);
            z[e1] = make_float2(dr * wr - di * wi, dr * wi + di * wr);
        }
    }
    __syncthreads();
}

template <int N, int B>
__global__ __launch_bounds__(B) void piv_phase_kernel(const float *__restrict__ im1, const float *__restrict__ im2, int W, int H, int step,
                                                      int R, int n_cols, const int *__restrict__ offset, int mode, double inv_filter_sum,
                                                      const PhaseTables tab, float *__restrict__ vectors, int *__restrict__ flags,
                                                      float *__restrict__ planes) {
    static_assert(N == 16 || N == 32 || N == 64, "win");
    static_assert(B % 64 == 0 && B >= N && B <= 1024, "whole waves, and a lane per row for the sums");
    constexpr int LOG = N == 16 ? 4 : N == 32 ? 5 : 6, PITCH = N + 1;
    __shared__ float2 z[N * PITCH];
    __shared__ float2 stw[N / 2];
    __shared__ float sg[N], sw[N];
    __shared__ float red[68];           // 0..63: the block reductions (4 floats a wave at most); 64..67: the two sums, the two energies
    __shared__ int redi[16];

    const int win_id = blockIdx.x, tid = threadIdx.x;
    const int wy0 = (win_id / n_cols) * step, wx0 = (win_id % n_cols) * step;
    const int ox = offset ? offset[2 * win_id] : 0, oy = offset ? offset[2 * win_id + 1] : 0;
    const int nS = 2 * R + 1;

    for (int i = tid; i < N / 2; i += B) stw[i] = make_float2(tab.twiddles[2 * i], tab.twiddles[2 * i + 1]);
    for (int i = tid; i < N; i += B) {
        sg[i] = tab.window[i];
        sw[i] = tab.filter[i];
    }

    // ---- the pixels: (a, b) at their natural places, b = 0 outside the image; the extremes decide flatness
    float ext[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};       // max a, max -a, max b, max -b
    for (int i = tid; i < N * N; i += B) {
        const int y = i / N, x = i % N;
        const float a = im1[(size_t)(wy0 + y) * W + (wx0 + x)];
        const int gy = wy0 + oy + y, gx = wx0 + ox + x;
        float b = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            b = im2[(size_t)gy * W + gx];
            ext[2] = fmaxf(ext[2], b);
            ext[3] = fmaxf(ext[3], -b);
        }
        ext[0] = fmaxf(ext[0], a);
        ext[1] = fmaxf(ext[1], -a);
        z[y * PITCH + x] = make_float2(a, b);
    }
    block_reduce(ext, red, B / 64, MaxF32());           // (its barriers also publish z and the tables)
    const int rows_in = count_inside((long long)wy0 + oy, N, H), cols_in = count_inside((long long)wx0 + ox, N, W);
    const float cnt = (float)(rows_in * cols_in);
    const bool outside = rows_in < N || cols_in < N;
    const bool all_equal = ext[0] == -ext[1] || cnt == 0.f || ext[2] == -ext[3];

    // ---- the sums: lane r walks row r from its first column on, then the rows by halving (row i + row i + h)
    float sum_a = 0.f, sum_b = 0.f;
    if (tid < N)
        for (int x = 0; x < N; x++) {
            const float2 v = z[tid * PITCH + x];
            sum_a = sum_a + v.x;
            sum_b = sum_b + v.y;
        }
#pragma unroll
    for (int o = N / 2; o > 0; o >>= 1) {
        sum_a += __shfl_xor(sum_a, o, 64);
        sum_b += __shfl_xor(sum_b, o, 64);
    }
    if (tid == 0) {
        red[64] = sum_a;
        red[65] = sum_b;
    }
    __syncthreads();
    const float mean_a = red[64] / (float)(N * N);
    const float mean_b = cnt > 0.f ? red[65] / cnt : 0.f;

    // ---- mean off, weights on, in place; the two energies in the order of the sums
    float ea = 0.f, eb = 0.f;
    if (tid < N) {
        const float gr = sg[tid];
        const int gy = wy0 + oy + tid;
        const bool row_in = gy >= 0 && gy < H;
        for (int x = 0; x < N; x++) {
            const float2 v = z[tid * PITCH + x];
            const int gx = wx0 + ox + x;
            const float gc = sg[x];
            const float a = ((v.x - mean_a) * gr) * gc;
            const float b = ((row_in && gx >= 0 && gx < W ? v.y - mean_b : 0.f) * gr) * gc;
            ea = ea + a * a;
            eb = eb + b * b;
            z[tid * PITCH + x] = make_float2(a, b);
        }
    }
#pragma unroll
    for (int o = N / 2; o > 0; o >>= 1) {
        ea += __shfl_xor(ea, o, 64);
        eb += __shfl_xor(eb, o, 64);
    }
    if (tid == 0) {
        red[66] = ea;
        red[67] = eb;
    }
    __syncthreads();                    // (also publishes the weighted z)
    ea = red[66];
    eb = red[67];

    // flat window (block-uniform): by its pixels, or a contrast too small for the f32 energies
    if (all_equal || !(ea > 0.f) || !(eb > 0.f)) {
        write_flat(win_id, nS * nS, outside, vectors, flags, planes);
        return;
    }

    // ---- Z = DFT(a' + i b'): rows, then columns
    for (int S = LOG - 1; S >= 0; S--) fft_stage<N, B, false, false>(z, stw, S, tid);
    for (int S = LOG - 1; S >= 0; S--) fft_stage<N, B, false, true>(z, stw, S, tid);

    // ---- 2 A = Z(k) + conj Z(-k), 2 B = -i (Z(k) - conj Z(-k)), T = conj(A) B or its filtered phase.  Place p holds bin
    //      k = bitrev(p); T(-k) = conj T(k) bit for bit, so the lower place of each pair computes and writes both.
    for (int p = tid; p < N * N; p += B) {
        const int py = p / N, px = p % N;
        const int ky = (int)(__brev((unsigned)py) >> (32 - LOG)), kx = (int)(__brev((unsigned)px) >> (32 - LOG));
        const int qy = (int)(__brev((unsigned)((N - ky) & (N - 1))) >> (32 - LOG));
        const int qx = (int)(__brev((unsigned)((N - kx) & (N - 1))) >> (32 - LOG));
        if (qy * N + qx < p) continue;
        const float2 zk = z[py * PITCH + px], zm = z[qy * PITCH + qx];
        const float ar = zk.x + zm.x, ai = zk.y - zm.y, br = zk.y + zm.y, bi = zm.x - zk.x;
        float tr = ar * br + ai * bi, ti = ar * bi - ai * br;
        if (mode == 1) {
            const float mag = sqrtf(tr * tr + ti * ti);
            if (mag > 0.f && p != 0) {          // p = 0: the bin of the means holds rounding only
                const float q = (sw[ky] * sw[kx]) / mag;
                tr = tr * q;
                ti = ti * q;
            } else {
                tr = 0.f;
                ti = 0.f;
            }
        }
        z[py * PITCH + px] = make_float2(tr, ti);
        if (qy * N + qx != p) z[qy * PITCH + qx] = make_float2(tr, -ti);
    }
    __syncthreads();

    // ---- back: columns, then rows; the plane is the real part, shift s at index s mod N
    for (int S = 0; S < LOG; S++) fft_stage<N, B, true, true>(z, stw, S, tid);
    for (int S = 0; S < LOG; S++) fft_stage<N, B, true, false>(z, stw, S, tid);
    auto plane_at = [&](int sy, int sx) { return z[((sy - R) & (N - 1)) * PITCH + ((sx - R) & (N - 1))].x; };

    const double inv = mode == 1 ? inv_filter_sum : 1.0 / ((double)(4 * N * N) * sqrt((double)ea * (double)eb));
    peak_tail(plane_at, plane_at, nS, R, ox, oy, inv, outside, win_id, vectors, flags, planes, red, redi);
}

template <int N, int B>
int launch(const float *im1, const float *im2, int W, int H, int step, int R, int n_rows, int n_cols, const int *offset, int mode,
           float window_sigma, float diameter, float *vectors, int *flags, float *planes, hipStream_t stream) {
    PhaseTables tab = {};
    fill_tables(N, window_sigma, diameter, tab.twiddles, tab.window, tab.filter);
    double s = 0.0;
    for (int k = 0; k < N; k++) s += (double)tab.filter[k];
    const double inv_filter_sum = 1.0 / (s * s - 1.0);          // the bin of the means never contributes
    hipLaunchKernelGGL((piv_phase_kernel<N, B>), dim3((unsigned)(n_rows * n_cols)), dim3(B), 0, stream, im1, im2, W, H, step, R, n_cols,
                       offset, mode, inv_filter_sum, tab, vectors, flags, planes);
    PH_CHECK(hipGetLastError());
    return 0;
}

const char *weights_error(float window_sigma, float diameter) {
    if (!(std::isfinite(window_sigma) && window_sigma >= 0.f)) return "window_sigma must be finite and >= 0";
    if (!(std::isfinite(diameter) && diameter >= 0.f)) return "diameter must be finite and >= 0";
    return nullptr;
}

}  // namespace

extern "C" int photon_piv_phase_tables(int win, float window_sigma, float diameter, float *twiddles, float *window, float *filter) {
    const char *bad = piv_grid::win_error(win);
    if (!bad) bad = weights_error(window_sigma, diameter);
    if (!bad && (!twiddles || !window || !filter)) bad = "null table pointer";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_phase_tables: %s (win %d, window_sigma %g, diameter %g)\n", bad, win, (double)window_sigma,
                (double)diameter);
        return 1;
    }
    fill_tables(win, window_sigma, diameter, twiddles, window, filter);
    return 0;
}

extern "C" int photon_piv_correlate_phase(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int radius,
                                          const int *d_offset, int mode, float window_sigma, float diameter, float *d_vectors, int *d_flags,
                                          float *d_planes, int *n_rows, int *n_cols, void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (radius < 1 || radius > win / 2 - 1)) bad = "radius must lie in [1, win / 2 - 1]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && mode != 0 && mode != 1) bad = "mode must be 0 or 1";
    if (!bad) bad = weights_error(window_sigma, diameter);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && d_vectors && !d_flags) bad = "d_vectors without d_flags";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate_phase: %s (win %d, step %d, radius %d, mode %d, window_sigma %g, diameter %g, %d x %d image)\n",
                bad, win, step, radius, mode, (double)window_sigma, (double)diameter, width, height);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate_phase", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_vectors) return 0;                   // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto N) {            // 64 threads at win 16, 256 above
        return launch<N(), N() == 16 ? 64 : 256>(d_im1, d_im2, width, height, step, radius, rows, cols, d_offset, mode, window_sigma, diameter,
                                                 d_vectors, d_flags, d_planes, stream);
    });
}
