// photon_dots.hip - dot tracking on an image pair (BOS / PTV): find the dots of an image, locate each to a fraction of a
// pixel, pair the dots of two frames and average the pairs' shifts onto section 5's window grid.  Definition:
// include/parallel_ray_tracing.h, section 8; host model: photon_amd/dot_tracking.py.
//
//   image_max_kernel        grid-stride maximum of the finite pixels, folded per wave and workgroup, one atomicMax per
//                           workgroup on the bits of a non-negative float (a maximum does not depend on the order)
//   detect_mask_kernel      every wave takes 16 consecutive pieces of 64 pixels in row-major order: the peak test per
//                           lane (threshold first: the eight neighbours are read by the few lanes that pass it), one
//                           ballot per piece -> the piece's 64-bit mask and its popcount
//   scan_kernel             exclusive scan of an int array by ONE workgroup: a contiguous segment per thread, a wave
//                           and workgroup scan of the segment sums, the segment again.  Used for the pieces of detect
//                           and the cells of match.
//   detect_write_kernel     one thread per piece: its set bits, in increasing order, from the piece's scanned offset
//   fit_kernel              16 lanes per dot, 16 dots per workgroup: lane l holds row l of the box in registers and the
//                           exponentials of row l and column l; column weights travel by __shfl inside the group, the
//                           sums fold by __shfl_xor 8, 4, 2, 1 (a + b on both partners: every lane ends with the same bits)
//   match_*                 targets and cell counts (integer atomics), scan, fill, a 3 x 3-cell search in both
//                           directions that orders candidates by (d2, index) -- the order in which the fill's atomics
//                           land changes the lists' order in scratch and nothing else --, and the pairing
//   window_means_kernel     one wave per window: 64 dots per step, a ballot of the members, their shifts added in f64
//                           in increasing dot index by every lane alike
// Device scratch comes from the caller (photon_dots_*_scratch_bytes): the entry points are asynchronous and allocate
// nothing, so nothing has to outlive them.
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_peak.hpp"

using namespace photon;

namespace {

constexpr int kWave = 64;

// =============================================================================================
// exclusive scan by one workgroup
// =============================================================================================
constexpr int kScanThreads = 1024;

// Array b = blockIdx.x starts at data + b * stride and has n + 1 entries: [0, n) are replaced by their exclusive prefix
// sums, entry n receives the total.  total_out (or NULL) receives array 0's total.
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int *__restrict__ data, int n, size_t stride, int *__restrict__ total_out) {
    __shared__ int s_wave[kScanThreads / kWave];
    int *a = data + (size_t)blockIdx.x * stride;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long seg = ((long long)n + kScanThreads - 1) / kScanThreads;
    const long long lo = min((long long)tid * seg, (long long)n), hi = min(lo + seg, (long long)n);
    int sum = 0;
    for (long long i = lo; i < hi; i++) sum += a[i];
    int inc = sum;                                                          // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kScanThreads / kWave; w++) {
        before += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    int run = before + inc - sum;
    for (long long i = lo; i < hi; i++) {
        const int c = a[i];
        a[i] = run;
        run += c;
    }
    if (tid == 0) {
        a[n] = total;
        if (total_out && blockIdx.x == 0) *total_out = total;
    }
}

// =============================================================================================
// image maximum
// =============================================================================================
constexpr int kMaxThreads = 256, kMaxBlocks = 256;

__global__ __launch_bounds__(kMaxThreads) void image_max_kernel(const float *__restrict__ im, long long n, unsigned *__restrict__ out_bits) {
    __shared__ float s_wave[kMaxThreads / kWave];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * kMaxThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kMaxThreads) {
        const float v = im[i];
        if (isfinite(v) && v > m) m = v;
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kMaxThreads / kWave; w++) m = fmaxf(m, s_wave[w]);
        // one atomic per workgroup; m >= +0: the bit patterns of non-negative floats order as unsigned integers
        if (m > 0.f) atomicMax(out_bits, __float_as_uint(m));
    }
}

// =============================================================================================
// a. detect
// =============================================================================================
constexpr int kDetThreads = 256, kDetPieces = 16;                           // pieces of 64 pixels per wave
constexpr int kDetRun = kDetThreads * kDetPieces;                           // pixels per workgroup

// section 8a's test at pixel index p < W H.  The threshold comes first: in a dot image few pixels pass it, and only
// those pay for the division and the eight neighbours.
__device__ __forceinline__ bool is_peak(const float *__restrict__ im, int W, int H, int p, float thr) {
    const float v = im[p];
    if (!(v > thr) || !isfinite(v)) return false;
    const int r = p / W, q = p - r * W;
    if (r < 1 || r > H - 2 || q < 1 || q > W - 2) return false;
    const float *up = im + (p - W), *dn = im + (p + W);
    // v is finite: v <= n is false for a smaller or a NaN neighbour, v < n likewise
    if (v <= up[-1] || v <= up[0] || v <= up[1] || v <= im[p - 1]) return false;
    if (v < im[p + 1] || v < dn[-1] || v < dn[0] || v < dn[1]) return false;
    return true;
}

__global__ __launch_bounds__(kDetThreads) void detect_mask_kernel(const float *__restrict__ im, int W, int H, float threshold,
                                                                  const float *__restrict__ scale, unsigned long long *__restrict__ masks,
                                                                  int *__restrict__ counts) {
    const long long n = (long long)W * H;
    const float thr = scale ? threshold * *scale : threshold;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long piece0 = ((long long)blockIdx.x * (kDetThreads / kWave) + wave) * kDetPieces;
    for (int k = 0; k < kDetPieces; k++) {
        const long long p = (piece0 + k) * kWave + lane;
        const bool pk = p < n && is_peak(im, W, H, (int)p, thr);
        const unsigned long long m = __ballot(pk);
        if (lane == 0) {
            masks[piece0 + k] = m;
            counts[piece0 + k] = __popcll(m);
        }
    }
}

__global__ __launch_bounds__(256) void detect_write_kernel(const unsigned long long *__restrict__ masks, const int *__restrict__ offsets,
                                                           int n_pieces, int max_dots, int *__restrict__ peaks) {
    const int piece = blockIdx.x * 256 + threadIdx.x;
    if (piece >= n_pieces) return;
    unsigned long long m = masks[piece];
    int at = offsets[piece];
    while (m && at < max_dots) {
        const int bit = __ffsll((long long)m) - 1;
        peaks[at++] = piece * kWave + bit;
        m &= m - 1;
    }
}

// =============================================================================================
// b. fit
// =============================================================================================
constexpr int kFitLanes = 16, kFitThreads = 256, kFitBox = 15;             // box_radius <= 7

__device__ __forceinline__ double fold16(double v) {
#pragma unroll
    for (int d = kFitLanes / 2; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kFitLanes);
    return v;
}

__global__ __launch_bounds__(kFitThreads) void fit_kernel(const float *__restrict__ im, int W, int H, const int *__restrict__ peaks,
                                                          const int *__restrict__ count, int max_dots, int R, double sigma_w,
                                                          int iterations, double background, float *__restrict__ dots,
                                                          int *__restrict__ status) {
    const int n = min(max(*count, 0), max_dots);
    if (blockIdx.x * (kFitThreads / kFitLanes) >= n) return;          // the whole workgroup: the capacity is several times the count
    const int k = blockIdx.x * (kFitThreads / kFitLanes) + threadIdx.x / kFitLanes, l = threadIdx.x & (kFitLanes - 1);
    // a group without a dot runs along on an empty box (every lane of the wave takes every shuffle) and stores nothing
    const bool live = k < n;
    const int p = live ? peaks[k] : -1;
    const bool pixel = p >= 0 && (long long)p < (long long)W * H;
    const int r = pixel ? p / W : -(kFitBox + 1), q = pixel ? p - r * W : -(kFitBox + 1);
    const int nb = 2 * R + 1;
    const int row = r + l - R;
    const bool row_in = l < nb && row >= 0 && row < H;

    double I[kFitBox], i_left = 0.0, i_mid = 0.0, i_right = 0.0;
#pragma unroll
    for (int c = 0; c < kFitBox; c++) {
        const int col = q + c - R;
        double v = 0.0;
        if (row_in && c < nb && col >= 0 && col < W) {
            const float f = im[(size_t)row * W + col];
            if (isfinite(f)) v = fmax((double)f - background, 0.0);
        }
        I[c] = v;
        i_left = c == R - 1 ? v : i_left;
        i_mid = c == R ? v : i_mid;
        i_right = c == R + 1 ? v : i_right;
    }
    // the 3-point start through the peak pixel: row R holds the x neighbours, column R of rows R - 1, R + 1 the y neighbours
    const double i0 = __shfl(i_mid, R, kFitLanes);
    double dx = subpixel(__shfl(i_left, R, kFitLanes), i0, __shfl(i_right, R, kFitLanes));
    double dy = subpixel(__shfl(i_mid, R - 1, kFitLanes), i0, __shfl(i_mid, R + 1, kFitLanes));
    int st = 0;
    if (q - R < 0 || q + R > W - 1 || r - R < 0 || r + R > H - 1) st |= 1;

    const double two_s2 = 2.0 * (sigma_w * sigma_w), o = (double)(l - R);
    double diameter = __builtin_nan("");
    for (int it = 0; it <= iterations; it++) {
        // lane l: the weight of column l and of row l at the current position
        const double ax = o - dx, ay = o - dy;
        const double ex = l < nb ? exp(-(ax * ax) / two_s2) : 0.0, ey = l < nb ? exp(-(ay * ay) / two_s2) : 0.0;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int c = 0; c < kFitBox; c++) {
            const double e = __shfl(ex, c, kFitLanes);             // 0 beyond the box (c >= nb)
            const double w = I[c] * e, oc = (double)(c - R);
            s0 = s0 + w;
            s1 = s1 + w * oc;
            s2 = s2 + w * ((oc - dx) * (oc - dx));
        }
        const double sw = fold16(ey * s0);
        if (it == iterations) {                                     // the variance at the final position (iterations > 0)
            if (iterations > 0 && sw > 0.0) {
                const double v = fold16(ey * s2 + (ey * s0) * (ay * ay)) / (2.0 * sw);
                const double sg2 = sigma_w * sigma_w, var = v * sg2 / (sg2 - v) - 1.0 / 12.0;
                if (var > 0.0 && isfinite(var)) diameter = 4.0 * sqrt(var);
            }
            break;
        }
        const double sx = fold16(ey * s1), sy = fold16((ey * s0) * o);
        if (sw > 0.0) {
            dx = sx / sw;
            dy = sy / sw;
        } else {
            st |= 4;
        }
    }
    if (fabs(dx) > 1.0 || fabs(dy) > 1.0) st |= 2;
    if (live && l == 0) {
        float4 out;
        if (pixel) out = make_float4((float)((double)q + dx), (float)((double)r + dy), (float)i0, (float)diameter);
        else {
            const float qn = __builtin_nanf("");
            out = make_float4(qn, qn, qn, qn);
            st = 8;
        }
        reinterpret_cast<float4 *>(dots)[k] = out;
        status[k] = st;
    }
}

// =============================================================================================
// c. match
// =============================================================================================
constexpr int kMatchThreads = 256;

struct CellGrid {
    double cell;                            // cell side in pixels, >= 1.001 radius
    int nx, ny;
};

__device__ __forceinline__ int cell_coord(float x, double cell, int n) {
    const double c = floor((double)x / cell);
    return c <= 0.0 ? 0 : (c >= (double)(n - 1) ? n - 1 : (int)c);
}

struct Predictor {
    const float *field;                     // NULL: none
    int stride, n_rows, n_cols, win, step;
};

// section 7b's bilinear rule at a continuous coordinate, every step one f32 operation
__device__ __forceinline__ void grid_weight_at(float p, int win, int step, int n, int &i0, int &i1, float &w) {
    const float c = (float)(win - 1) * 0.5f;
    float f = __fdiv_rn(__fsub_rn(p, c), (float)step);
    f = fminf(fmaxf(f, 0.f), (float)(n - 1));
    i0 = min((int)floorf(f), max(n - 2, 0));
    i1 = min(i0 + 1, n - 1);
    w = __fsub_rn(f, (float)i0);
}

__device__ __forceinline__ void field_node(const Predictor &P, int k, float &dx, float &dy) {
    dx = P.field[(size_t)k * P.stride];
    dy = P.field[(size_t)k * P.stride + 1];
    if (!(isfinite(dx) && isfinite(dy))) dx = dy = 0.f;
}

__device__ __forceinline__ float lerp_rn(float a, float b, float w) { return __fadd_rn(a, __fmul_rn(w, __fsub_rn(b, a))); }

__device__ __forceinline__ bool takes_part(const float *__restrict__ dots, const int *__restrict__ status, int mask, int k, float &x, float &y) {
    x = dots[4 * (size_t)k];
    y = dots[4 * (size_t)k + 1];
    return isfinite(x) && isfinite(y) && !(status && (status[k] & mask));
}

struct MatchArgs {
    const float *dots1, *dots2;
    const int *status1, *status2, *count1, *count2;
    int max1, max2, reject;
    Predictor pred;
    CellGrid grid;
    float r2;
    float *tgt;                             // [max1][2], NaN for a dot that takes no part
    int *start1, *start2;                   // [cells + 1]: counts, then exclusive offsets
    int *cur1, *cur2;                       // [cells] fill cursors
    int *list1, *list2;                     // dot indices by cell
    int *jstar, *istar;
};

__global__ __launch_bounds__(kMatchThreads) void match_count_kernel(MatchArgs a) {
    const int k = blockIdx.x * kMatchThreads + threadIdx.x;
    const int n1 = min(max(*a.count1, 0), a.max1), n2 = min(max(*a.count2, 0), a.max2);
    float x, y;
    if (k < n1) {
        float tx = __builtin_nanf(""), ty = tx;
        if (takes_part(a.dots1, a.status1, a.reject, k, x, y)) {
            float px = 0.f, py = 0.f;
            if (a.pred.field) {
                int i0, i1, j0, j1;
                float wy, wx, ax, ay, bx, by, cx, cy, ex, ey;
                grid_weight_at(y, a.pred.win, a.pred.step, a.pred.n_rows, i0, i1, wy);
                grid_weight_at(x, a.pred.win, a.pred.step, a.pred.n_cols, j0, j1, wx);
                field_node(a.pred, i0 * a.pred.n_cols + j0, ax, ay);
                field_node(a.pred, i0 * a.pred.n_cols + j1, bx, by);
                field_node(a.pred, i1 * a.pred.n_cols + j0, cx, cy);
                field_node(a.pred, i1 * a.pred.n_cols + j1, ex, ey);
                px = lerp_rn(lerp_rn(ax, bx, wx), lerp_rn(cx, ex, wx), wy);
                py = lerp_rn(lerp_rn(ay, by, wx), lerp_rn(cy, ey, wx), wy);
            }
            tx = __fadd_rn(x, px);
            ty = __fadd_rn(y, py);
            if (isfinite(tx) && isfinite(ty))
                atomicAdd(a.start1 + cell_coord(ty, a.grid.cell, a.grid.ny) * a.grid.nx + cell_coord(tx, a.grid.cell, a.grid.nx), 1);
            else tx = ty = __builtin_nanf("");
        }
        a.tgt[2 * (size_t)k] = tx;
        a.tgt[2 * (size_t)k + 1] = ty;
    }
    if (k < n2 && takes_part(a.dots2, a.status2, a.reject, k, x, y))
        atomicAdd(a.start2 + cell_coord(y, a.grid.cell, a.grid.ny) * a.grid.nx + cell_coord(x, a.grid.cell, a.grid.nx), 1);
}

__global__ __launch_bounds__(kMatchThreads) void match_fill_kernel(MatchArgs a) {
    const int k = blockIdx.x * kMatchThreads + threadIdx.x;
    const int n1 = min(max(*a.count1, 0), a.max1), n2 = min(max(*a.count2, 0), a.max2);
    float x, y;
    if (k < n1) {
        x = a.tgt[2 * (size_t)k];
        y = a.tgt[2 * (size_t)k + 1];
        if (x == x) {
            const int c = cell_coord(y, a.grid.cell, a.grid.ny) * a.grid.nx + cell_coord(x, a.grid.cell, a.grid.nx);
            const int at = a.start1[c] + atomicAdd(a.cur1 + c, 1);
            if (at < a.max1) a.list1[at] = k;
        }
    }
    if (k < n2 && takes_part(a.dots2, a.status2, a.reject, k, x, y)) {
        const int c = cell_coord(y, a.grid.cell, a.grid.ny) * a.grid.nx + cell_coord(x, a.grid.cell, a.grid.nx);
        const int at = a.start2[c] + atomicAdd(a.cur2 + c, 1);
        if (at < a.max2) a.list2[at] = k;
    }
}

// The nearest of the listed points to (x, y) within r2, ties to the smallest index.  `frame2`: the points are the dots
// of frame 2 and (x, y) a target; otherwise the points are the targets and (x, y) a dot of frame 2.  Either way
// d2 = (x2 - tx)^2 + (y2 - ty)^2 from the same operands in the same order: both directions see the same bits.
template <bool frame2>
__device__ __forceinline__ int nearest(const MatchArgs &a, float x, float y, int cap) {
    const int *start = frame2 ? a.start2 : a.start1, *list = frame2 ? a.list2 : a.list1;
    const int cx = cell_coord(x, a.grid.cell, a.grid.nx), cy = cell_coord(y, a.grid.cell, a.grid.ny);
    int best = -1;
    float best_d2 = 0.f;
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, a.grid.ny - 1); yy++)
        for (int xx = max(cx - 1, 0); xx <= min(cx + 1, a.grid.nx - 1); xx++) {
            const int c = yy * a.grid.nx + xx;
            const int lo = start[c], hi = min(start[c + 1], cap);
            for (int s = lo; s < hi; s++) {
                const int m = list[s];
                float ex, ey;
                if (frame2) {
                    ex = __fsub_rn(a.dots2[4 * (size_t)m], x);
                    ey = __fsub_rn(a.dots2[4 * (size_t)m + 1], y);
                } else {
                    ex = __fsub_rn(x, a.tgt[2 * (size_t)m]);
                    ey = __fsub_rn(y, a.tgt[2 * (size_t)m + 1]);
                }
                const float d2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                if (d2 <= a.r2 && (best < 0 || d2 < best_d2 || (d2 == best_d2 && m < best))) {
                    best = m;
                    best_d2 = d2;
                }
            }
        }
    return best;
}

__global__ __launch_bounds__(kMatchThreads) void match_search_kernel(MatchArgs a) {
    const int k = blockIdx.x * kMatchThreads + threadIdx.x;
    const int n1 = min(max(*a.count1, 0), a.max1), n2 = min(max(*a.count2, 0), a.max2);
    float x, y;
    if (k < n1) {
        x = a.tgt[2 * (size_t)k];
        y = a.tgt[2 * (size_t)k + 1];
        a.jstar[k] = x == x ? nearest<true>(a, x, y, a.max2) : -1;
    }
    if (k < n2) a.istar[k] = takes_part(a.dots2, a.status2, a.reject, k, x, y) ? nearest<false>(a, x, y, a.max1) : -1;
}

__global__ __launch_bounds__(kMatchThreads) void match_pair_kernel(MatchArgs a, int *__restrict__ pair, float *__restrict__ shift,
                                                                   int *__restrict__ npaired) {
    const int k = blockIdx.x * kMatchThreads + threadIdx.x;
    const int n1 = min(max(*a.count1, 0), a.max1);
    bool paired = false;
    if (k < n1) {
        const int j = a.jstar[k];
        paired = j >= 0 && a.istar[j] == k;
        const float qn = __builtin_nanf("");
        float4 out = make_float4(qn, qn, qn, qn);
        if (paired) {
            const float x1 = a.dots1[4 * (size_t)k], y1 = a.dots1[4 * (size_t)k + 1];
            const float dx = __fsub_rn(a.dots2[4 * (size_t)j], x1), dy = __fsub_rn(a.dots2[4 * (size_t)j + 1], y1);
            out = make_float4(__fadd_rn(x1, __fmul_rn(dx, 0.5f)), __fadd_rn(y1, __fmul_rn(dy, 0.5f)), dx, dy);
        }
        pair[k] = paired ? j : -1;
        reinterpret_cast<float4 *>(shift)[k] = out;
    }
    // an integer count: the sum does not depend on the order of the atomics
    const unsigned long long m = __ballot(paired);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(npaired, __popcll(m));
}

// =============================================================================================
// d. window means
// =============================================================================================
constexpr int kMeanThreads = 256;

__global__ __launch_bounds__(kMeanThreads) void window_means_kernel(const float *__restrict__ dots1, const int *__restrict__ pair,
                                                                    const float *__restrict__ shift, const int *__restrict__ count,
                                                                    int max1, int n_rows, int n_cols, int win, int step,
                                                                    int min_count, int anchor, float *__restrict__ vectors,
                                                                    int *__restrict__ flags) {
    const int n = min(max(*count, 0), max1);
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * (kMeanThreads / kWave) + threadIdx.x / kWave;
    if (w >= n_rows * n_cols) return;                               // a whole wave: no barrier follows
    const int wi = w / n_cols, wj = w - wi * n_cols;
    const double r0 = (double)wi * step, c0 = (double)wj * step;
    double sx = 0.0, sy = 0.0, mx = 0.0, my = 0.0, q = 0.0;
    int cnt = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int base = 0; base < n; base += kWave) {
            const int k = base + lane;
            bool member = false;
            float dx = 0.f, dy = 0.f;
            if (k < n && pair[k] >= 0) {
                const float4 s = reinterpret_cast<const float4 *>(shift)[k];
                const float ax = anchor ? s.x : dots1[4 * (size_t)k], ay = anchor ? s.y : dots1[4 * (size_t)k + 1];
                dx = s.z;
                dy = s.w;
                const double col = floor((double)ax + 0.5), row = floor((double)ay + 0.5);
                member = isfinite(dx) && isfinite(dy) && col >= c0 && col < c0 + win && row >= r0 && row < r0 + win;
            }
            unsigned long long m = __ballot(member);
            while (m) {                                             // wave-uniform: every lane adds the same values in the same order
                const int b = __ffsll((long long)m) - 1;
                const double vx = (double)__shfl(dx, b), vy = (double)__shfl(dy, b);
                if (pass == 0) {
                    sx = sx + vx;
                    sy = sy + vy;
                    cnt++;
                } else {
                    const double ex = vx - mx, ey = vy - my;
                    q = q + (ex * ex + ey * ey);
                }
                m &= m - 1;
            }
        }
        if (pass == 0) {
            if (cnt == 0) break;
            mx = sx / (double)cnt;
            my = sy / (double)cnt;
        }
    }
    if (lane == 0) {
        const bool ok = cnt >= min_count;
        const float qn = __builtin_nanf("");
        reinterpret_cast<float4 *>(vectors)[w] =
            ok ? make_float4((float)mx, (float)my, (float)cnt, (float)sqrt(q / (double)cnt)) : make_float4(qn, qn, (float)cnt, qn);
        flags[w] = ok ? 0 : 2;
    }
}

long long detect_pieces(int width, int height) {
    const long long n = (long long)width * height, runs = (n + kDetRun - 1) / kDetRun;
    return runs * (kDetRun / kWave);
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// the cell grid of photon_dots_match: cells of max(1.001 radius, 8, max(width, height) / 2048) pixels
CellGrid match_grid(int width, int height, float radius) {
    CellGrid g;
    g.cell = std::fmax(std::fmax(1.001 * (double)radius, 8.0), (double)std::max(width, height) / 2048.0);
    g.nx = (int)std::ceil((double)width / g.cell) + 1;
    g.ny = (int)std::ceil((double)height / g.cell) + 1;
    return g;
}

}  // namespace

extern "C" size_t photon_dots_detect_scratch_bytes(int width, int height) {
    if (width < 1 || height < 1 || (long long)width * height > INT_MAX) return 0;
    const size_t pieces = (size_t)detect_pieces(width, height);
    return align16(pieces * sizeof(unsigned long long)) + align16((pieces + 1) * sizeof(int));
}

extern "C" size_t photon_dots_match_scratch_bytes(int width, int height, float radius, int max1, int max2) {
    if (width < 1 || height < 1 || !(radius > 0.f) || !std::isfinite(radius) || max1 < 1 || max2 < 1) return 0;
    const CellGrid g = match_grid(width, height, radius);
    const size_t cells = (size_t)g.nx * g.ny;
    return align16(2 * (size_t)max1 * sizeof(float)) + align16((4 * cells + 2) * sizeof(int)) + 2 * align16((size_t)max1 * sizeof(int)) +
           2 * align16((size_t)max2 * sizeof(int));
}

extern "C" int photon_dots_image_max(const float *d_im, int width, int height, float *d_max, void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (!d_im || !d_max) bad = "null pointer";
    if (bad) {
        fprintf(stderr, "photon: photon_dots_image_max: %s (%d x %d image)\n", bad, width, height);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const long long n = (long long)width * height;
    PH_CHECK(hipMemsetAsync(d_max, 0, sizeof(float), stream));
    const unsigned blocks = (unsigned)std::min<long long>((n + kMaxThreads - 1) / kMaxThreads, kMaxBlocks);
    hipLaunchKernelGGL(image_max_kernel, dim3(blocks), dim3(kMaxThreads), 0, stream, d_im, n, reinterpret_cast<unsigned *>(d_max));
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_dots_detect(const float *d_im, int width, int height, float threshold, const float *d_scale, int max_dots,
                                  int *d_peaks, int *d_count, void *d_scratch, size_t scratch_bytes, void *stream_p) {
    const char *bad = nullptr;
    if (width < 3 || height < 3) bad = "the image is smaller than 3 x 3";
    else if ((long long)width * height > INT_MAX) bad = "more than INT_MAX pixels";
    else if (max_dots < 1) bad = "max_dots must be >= 1";
    else if (!std::isfinite(threshold)) bad = "threshold must be finite";
    else if (!d_im || !d_peaks || !d_count || !d_scratch) bad = "null d_im, d_peaks, d_count or d_scratch";
    else if (scratch_bytes < photon_dots_detect_scratch_bytes(width, height)) bad = "d_scratch is smaller than photon_dots_detect_scratch_bytes";
    if (bad) {
        fprintf(stderr, "photon: photon_dots_detect: %s (%d x %d image, max_dots %d, threshold %g)\n", bad, width, height, max_dots,
                (double)threshold);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const long long pieces = detect_pieces(width, height);
    unsigned long long *masks = static_cast<unsigned long long *>(d_scratch);
    int *counts = reinterpret_cast<int *>(static_cast<char *>(d_scratch) + align16((size_t)pieces * sizeof(unsigned long long)));
    hipLaunchKernelGGL(detect_mask_kernel, dim3((unsigned)(pieces / (kDetRun / kWave))), dim3(kDetThreads), 0, stream, d_im, width, height,
                       threshold, d_scale, masks, counts);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, counts, (int)pieces, (size_t)0, d_count);
    hipLaunchKernelGGL(detect_write_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, masks, counts, (int)pieces, max_dots,
                       d_peaks);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_dots_fit(const float *d_im, int width, int height, const int *d_peaks, const int *d_count, int max_dots,
                               int box_radius, double sigma_w, int iterations, double background, float *d_dots, int *d_status,
                               void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if ((long long)width * height > INT_MAX) bad = "more than INT_MAX pixels";
    else if (max_dots < 1) bad = "max_dots must be >= 1";
    else if (box_radius < 1 || box_radius > 7) bad = "box_radius must lie in [1, 7]";
    else if (iterations < 0 || iterations > 16) bad = "iterations must lie in [0, 16]";
    else if (!std::isfinite(sigma_w) || !(sigma_w > 0.0)) bad = "sigma_w must be finite and > 0";
    else if (!std::isfinite(background)) bad = "background must be finite";
    else if (!d_im || !d_peaks || !d_count || !d_dots || !d_status) bad = "null d_im, d_peaks, d_count, d_dots or d_status";
    if (bad) {
        fprintf(stderr, "photon: photon_dots_fit: %s (%d x %d image, max_dots %d, box_radius %d, sigma_w %g, iterations %d, background %g)\n",
                bad, width, height, max_dots, box_radius, sigma_w, iterations, background);
        return 1;
    }
    const int per_block = kFitThreads / kFitLanes;
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)((max_dots + per_block - 1) / per_block)), dim3(kFitThreads), 0, (hipStream_t)stream_p, d_im,
                       width, height, d_peaks, d_count, max_dots, box_radius, sigma_w, iterations, background, d_dots, d_status);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_dots_match(const float *d_dots1, const int *d_status1, const int *d_count1, int max1, const float *d_dots2,
                                 const int *d_status2, const int *d_count2, int max2, int reject_mask, const float *d_field,
                                 int field_stride, int n_rows, int n_cols, int win, int step, float radius, int width, int height,
                                 int *d_pair, float *d_shift, int *d_npaired, void *d_scratch, size_t scratch_bytes, void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (max1 < 1 || max2 < 1) bad = "max1 and max2 must be >= 1";
    else if (!std::isfinite(radius) || !(radius > 0.f)) bad = "radius must be finite and > 0";
    else if (!d_dots1 || !d_dots2 || !d_count1 || !d_count2 || !d_pair || !d_shift || !d_npaired || !d_scratch)
        bad = "null d_dots, d_count, d_pair, d_shift, d_npaired or d_scratch";
    else if (d_field && field_stride != 2 && field_stride != 4) bad = "field_stride must be 2 or 4";
    else if (d_field && (win < 1 || step < 1 || width < win || height < win)) bad = "win and step must be >= 1 and the image at least one window";
    else if (d_field && (n_rows != (height - win) / step + 1 || n_cols != (width - win) / step + 1))
        bad = "n_rows x n_cols is not the window grid of section 5";
    else if (scratch_bytes < photon_dots_match_scratch_bytes(width, height, radius, max1, max2))
        bad = "d_scratch is smaller than photon_dots_match_scratch_bytes";
    if (bad) {
        fprintf(stderr, "photon: photon_dots_match: %s (%d x %d image, max %d / %d, radius %g, %d x %d grid, win %d, step %d, stride %d)\n", bad,
                width, height, max1, max2, (double)radius, n_rows, n_cols, win, step, field_stride);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_p;
    MatchArgs a;
    a.dots1 = d_dots1, a.dots2 = d_dots2, a.status1 = d_status1, a.status2 = d_status2, a.count1 = d_count1, a.count2 = d_count2;
    a.max1 = max1, a.max2 = max2, a.reject = reject_mask;
    a.pred = Predictor{d_field, field_stride, n_rows, n_cols, win, step};
    a.grid = match_grid(width, height, radius);
    a.r2 = radius * radius;
    const size_t cells = (size_t)a.grid.nx * a.grid.ny;
    char *p = static_cast<char *>(d_scratch);
    a.tgt = reinterpret_cast<float *>(p);
    p += align16(2 * (size_t)max1 * sizeof(float));
    int *ints = reinterpret_cast<int *>(p);                          // start1 | start2 | cur1 | cur2: zeroed together
    a.start1 = ints, a.start2 = ints + (cells + 1), a.cur1 = ints + 2 * (cells + 1), a.cur2 = a.cur1 + cells;
    p += align16((4 * cells + 2) * sizeof(int));
    a.list1 = reinterpret_cast<int *>(p);
    p += align16((size_t)max1 * sizeof(int));
    a.jstar = reinterpret_cast<int *>(p);
    p += align16((size_t)max1 * sizeof(int));
    a.list2 = reinterpret_cast<int *>(p);
    p += align16((size_t)max2 * sizeof(int));
    a.istar = reinterpret_cast<int *>(p);
    PH_CHECK(hipMemsetAsync(ints, 0, (4 * cells + 2) * sizeof(int), stream));
    PH_CHECK(hipMemsetAsync(d_npaired, 0, sizeof(int), stream));
    const unsigned blocks = (unsigned)((std::max(max1, max2) + kMatchThreads - 1) / kMatchThreads);
    hipLaunchKernelGGL(match_count_kernel, dim3(blocks), dim3(kMatchThreads), 0, stream, a);
    hipLaunchKernelGGL(scan_kernel, dim3(2), dim3(kScanThreads), 0, stream, a.start1, (int)cells, cells + 1, (int *)nullptr);
    hipLaunchKernelGGL(match_fill_kernel, dim3(blocks), dim3(kMatchThreads), 0, stream, a);
    hipLaunchKernelGGL(match_search_kernel, dim3(blocks), dim3(kMatchThreads), 0, stream, a);
    hipLaunchKernelGGL(match_pair_kernel, dim3((unsigned)((max1 + kMatchThreads - 1) / kMatchThreads)), dim3(kMatchThreads), 0, stream, a,
                       d_pair, d_shift, d_npaired);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_dots_window_means(const float *d_dots1, const int *d_pair, const float *d_shift, const int *d_count1, int max1,
                                        int width, int height, int win, int step, int min_count, int anchor, float *d_vectors,
                                        int *d_flags, void *stream_p) {
    const char *bad = nullptr;
    if (win < 1 || step < 1) bad = "win and step must be >= 1";
    else if (width < win || height < win) bad = "the image is smaller than one window";
    else if (max1 < 1) bad = "max1 must be >= 1";
    else if (min_count < 1) bad = "min_count must be >= 1";
    else if (anchor != 0 && anchor != 1) bad = "anchor must be 0 or 1";
    else if ((long long)((height - win) / step + 1) * ((width - win) / step + 1) > INT_MAX) bad = "more than INT_MAX windows";
    else if (!d_dots1 || !d_pair || !d_shift || !d_count1 || !d_vectors || !d_flags) bad = "null pointer";
    if (bad) {
        fprintf(stderr, "photon: photon_dots_window_means: %s (%d x %d image, win %d, step %d, max1 %d, min_count %d, anchor %d)\n", bad, width,
                height, win, step, max1, min_count, anchor);
        return 1;
    }
    const int n_rows = (height - win) / step + 1, n_cols = (width - win) / step + 1;
    const int per_block = kMeanThreads / kWave;
    hipLaunchKernelGGL(window_means_kernel, dim3((unsigned)(((long long)n_rows * n_cols + per_block - 1) / per_block)), dim3(kMeanThreads), 0,
                       (hipStream_t)stream_p, d_dots1, d_pair, d_shift, d_count1, max1, n_rows, n_cols, win, step, min_count, anchor, d_vectors,
                       d_flags);
    PH_CHECK(hipGetLastError());
    return 0;
}
