// photon_piv_weighted.hip - section 5's direct correlation with a weight per window pixel: a Gaussian (or any other
// non-negative) window in place of the top hat, whose frequency response turns negative below the window size.
// Definition: include/parallel_ray_tracing.h, section 18; host model: photon_amd/piv_weighting.py
// (correlate_weighted_model); DESIGN.md section 4.3q.
//
// One workgroup per window, section 5's plan (piv_direct::plan_for), tile loop and peak tail; no LDS beyond section 5's.
// The weight rides on frame 1's window: sa holds W (a - mean a) in place, so the tile loop sums W (a - mean a)(b - mean b)
// as it stands.  The table (win^2 floats, shared by all windows, resident in L2) is read from global memory in the first
// pass and in the staging of b.  The staging passes are section 5's lane for lane with W as one more factor:
// fmaf(1, v, s) is s + v and 1 d is d, so a table of ones returns section 5's bits.  They are a copy, not a shared function: sharing the staging pass
// changed section 5's code generation.  The one thing that moved is the exact flatness count:
// its reference pixels depend on the table (the first pixel under a weight > 0), so they are fetched behind the first pass
// and the count rides with the energies in the second reduction; the decision is taken after that one in section 5 too.
// The loops that read global memory ask for the loads of kBatch trips together (addresses clamped, no load behind a
// branch) and use the values in section 5's order: the same sums, a quarter of the waits.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_direct.hpp"
#include "piv_grid.hpp"
#include "piv_peak.hpp"

using namespace photon;

namespace {

using namespace piv_direct;

constexpr int kBatch = 4;           // trips of a staging loop whose loads are in flight together

// the weight the kernel reads: negative and NaN entries count as 0
__device__ __forceinline__ float live_weight(float w) { return w > 0.f ? w : 0.f; }

// The first entry > 0 of the table inside the box of rh x rw window pixels at (y0, x0), in row-major order, as its index
// in the table; -1 when there is none.  Every wave scans for itself, 64 entries a step, so the answer is block-uniform
// without a barrier.  The whole window's scan takes its first 64 entries from a load the caller made earlier (`head`:
// entry `lane` of the table), so that any table with a positive weight among them costs no wait here.
template <int WIN>
__device__ __forceinline__ int first_live(const float *__restrict__ weight, int y0, int x0, int rh, int rw, bool whole = false, float head = 0.f) {
    const int lane = threadIdx.x & 63, n = rh * rw;
    if (whole) {
        const unsigned long long found = __ballot(head > 0.f);
        if (found) return __ffsll((long long)found) - 1;
    }
    for (int base = whole ? 64 : 0; base < n; base += 64) {
        const int j = base + lane;
        bool live = false;
        int idx = 0;
        if (j < n) {
            idx = (y0 + j / rw) * WIN + (x0 + j % rw);
            live = weight[idx] > 0.f;
        }
        const unsigned long long found = __ballot(live);
        if (found) return __shfl(idx, __ffsll((long long)found) - 1, 64);
    }
    return -1;
}

// LDS layout (floats): a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | K partial planes [nSyp][nSxp] | reduction scratch.
template <int WIN>
__global__ __launch_bounds__(kMaxThreads) void piv_correlate_weighted_kernel(const float *__restrict__ im1, const float *__restrict__ im2,
                                                                             const float *__restrict__ weight, int W, int H, int step, int R,
                                                                             int n_cols, const int *__restrict__ offset, int K, int nSxp,
                                                                             int nSyp, float *__restrict__ vectors, int *__restrict__ flags,
                                                                             float *__restrict__ planes) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nS = 2 * R + 1, nS2 = nS * nS;
    const int pitch = WIN + nSxp, rows = WIN + nSyp - 1, P = nSyp * nSxp;
    float *sa = lds;
    float *sb = sa + WIN * WIN;
    float *sp = sb + rows * pitch;
    float *red = sp + K * P;
    int *redi = reinterpret_cast<int *>(red + 32);

    const int win_id = blockIdx.x;
    const int wy0 = (win_id / n_cols) * step, wx0 = (win_id % n_cols) * step;
    const int ox = offset ? offset[2 * win_id] : 0, oy = offset ? offset[2 * win_id + 1] : 0;
    const int tid = threadIdx.x, B = blockDim.x;
    const float head = weight[tid & 63];        // for first_live below: asked for now, looked at behind the first pass

    // ---- weighted sums for the means: a over the window; b over the in-image pixels of the zero-shift window (outside
    //      pixels read as that mean).  The weight of pixel i waits in sb[i], idle until the second pass, for the thread that
    //      put it there: the second pass over a then reads LDS alone, as section 5's does (a global load per trip there cost
    //      9 us a launch at 1024^2).  Both passes and the b staging walk i = tid, tid + B, ...: a thread meets only its own
    //      residue class of sb, so its weights are still there when it reads them, whatever the other threads have staged.
    //      The loads of kBatch trips are asked for together, with addresses clamped into the image and the table so that
    //      none of them hangs on a branch, and their values are used in the order of i: the pass waits for memory once per
    //      batch, where a trip-by-trip loop waits once per trip (and twice where b's load follows a's behind a branch).
    float sum_a = 0.f, sum_b = 0.f, sw_a = 0.f, sw_b = 0.f;
    for (int i0 = tid; i0 < WIN * WIN; i0 += kBatch * B) {
        float v[kBatch], u[kBatch], w[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int i = min(i0 + k * B, WIN * WIN - 1);
            const int y = i / WIN, x = i % WIN;
            const int gy = min(max(wy0 + oy + y, 0), H - 1), gx = min(max(wx0 + ox + x, 0), W - 1);
            v[k] = im1[(size_t)(wy0 + y) * W + (wx0 + x)];
            u[k] = im2[(size_t)gy * W + gx];
            w[k] = weight[i];
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int i = i0 + k * B;
            if (i < WIN * WIN) {
                const int gy = wy0 + oy + i / WIN, gx = wx0 + ox + i % WIN;
                const float wk = live_weight(w[k]);
                sa[i] = v[k];
                sb[i] = wk;
                sum_a = fmaf(wk, v[k], sum_a);
                sw_a += wk;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    sum_b = fmaf(wk, u[k], sum_b);
                    sw_b += wk;
                }
            }
        }
    }

    // ---- the pixels flatness is read against: the first of a under a weight > 0, and the first of b at zero shift that
    //      lies in the image under a weight > 0 (the in-image part of the zero-shift window is a box).  With a table of ones
    //      these are section 5's two reference pixels.  Asked for here, behind the loop that pulled both windows into the
    //      cache, and first used after the reduction: nothing waits for them.
    const int by0 = max(0, -(wy0 + oy)), by1 = min(WIN, H - (wy0 + oy));
    const int bx0 = max(0, -(wx0 + ox)), bx1 = min(WIN, W - (wx0 + ox));
    const int bh = max(0, by1 - by0), bw = max(0, bx1 - bx0);
    const int ia = first_live<WIN>(weight, 0, 0, WIN, WIN, true, head);
    const int ib = bh == WIN && bw == WIN ? ia : first_live<WIN>(weight, by0, bx0, bh, bw);
    const float ref_a = ia >= 0 ? im1[(size_t)(wy0 + ia / WIN) * W + (wx0 + ia % WIN)] : 0.f;
    const float ref_b = ib >= 0 ? im2[(size_t)(wy0 + oy + ib / WIN) * W + (wx0 + ox + ib % WIN)] : 0.f;

    const int n_waves = B >> 6;
    float tot[4] = {sum_a, sum_b, sw_a, sw_b};
    block_reduce(tot, red, n_waves, Sum());
    const float mean_a = tot[0] / tot[2];
    const float mean_b = tot[3] > 0.f ? tot[1] / tot[3] : 0.f;

    // ---- W (a - mean a) in place; the b region with zero padding; the two weighted energies (b at zero shift); and how
    //      many pixels of a, and of b at zero shift in the image, lie under a weight > 0 and differ from their reference,
    //      which decides flatness exactly (counts up to win^2 are exact in f32; (w a) / w need not return a)
    float e[4] = {0.f, 0.f, 0.f, 0.f};          // energy a, energy b, differing pixels of a, of b
    for (int i = tid; i < WIN * WIN; i += B) {
        const float w = sb[i];
        const float u = sa[i], v = u - mean_a;
        const float wv = w * v;
        sa[i] = wv;
        e[0] = fmaf(wv, v, e[0]);
        e[2] += w > 0.f && u != ref_a ? 1.f : 0.f;
    }
    const int span = WIN + 2 * R, n_b = rows * pitch;
    for (int i0 = tid; i0 < n_b; i0 += kBatch * B) {            // batched as the first pass
        float u[kBatch], w[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int i = min(i0 + k * B, n_b - 1);
            const int ry = i / pitch, rx = i % pitch;
            const int gy = min(max(wy0 + oy - R + ry, 0), H - 1), gx = min(max(wx0 + ox - R + rx, 0), W - 1);
            const bool zero_shift = ry >= R && ry < R + WIN && rx >= R && rx < R + WIN;
            u[k] = im2[(size_t)gy * W + gx];
            w[k] = weight[zero_shift ? (ry - R) * WIN + (rx - R) : 0];
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int i = i0 + k * B;
            if (i < n_b) {
                const int ry = i / pitch, rx = i % pitch;
                float v = 0.f;
                if (ry < span && rx < span) {
                    const int gy = wy0 + oy - R + ry, gx = wx0 + ox - R + rx;
                    const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    if (inside) v = u[k] - mean_b;
                    if (ry >= R && ry < R + WIN && rx >= R && rx < R + WIN) {
                        const float wk = live_weight(w[k]);
                        e[1] = fmaf(wk * v, v, e[1]);
                        e[3] += inside && wk > 0.f && u[k] != ref_b ? 1.f : 0.f;
                    }
                }
                sb[i] = v;
            }
        }
    }
    block_reduce(e, red, n_waves, Sum());       // (its barriers also publish sa and sb)
    const float ea = e[0], eb = e[1];
    // all pixels of a under a weight equal (or no weight above 0 at all), or all (or none) of b at zero shift
    const bool all_equal = e[2] == 0.f || e[3] == 0.f;

    const bool outside = wy0 + oy - R < 0 || wx0 + ox - R < 0 || wy0 + oy + WIN - 1 + R >= H || wx0 + ox + WIN - 1 + R >= W;
    // flat window (block-uniform): by its pixels, or a contrast too small for the f32 energies (1 / sqrt(0) below)
    if (all_equal || !(ea > 0.f) || !(eb > 0.f)) {
        write_flat(win_id, nS2, outside, vectors, flags, planes);
        return;
    }

    // ---- the correlation: every lane's tile into its slice's partial plane
    correlate_tiles<WIN>(sa, sb, sp, K, P, pitch, nSxp, nSyp);
    __syncthreads();

    // ---- the plane (slices summed in order, into slice 0, as the tail's first pass meets each shift) and the peak read-out
    const double inv = 1.0 / sqrt((double)ea * (double)eb);
    auto sum_slices = [&](int sy, int sx) {
        const int j = sy * nSxp + sx;
        float c = sp[j];
        for (int k = 1; k < K; k++) c += sp[k * P + j];
        sp[j] = c;
        return c;
    };
    auto plane_at = [&](int sy, int sx) { return sp[sy * nSxp + sx]; };
    peak_tail(sum_slices, plane_at, nS, R, ox, oy, inv, outside, win_id, vectors, flags, planes, red, redi);
}

template <int WIN>
int launch(const float *im1, const float *im2, const float *weight, int W, int H, int step, int R, int n_rows, int n_cols, const int *offset,
           float *vectors, int *flags, float *planes, hipStream_t stream) {
    int lds_limit = 0;
    PH_TRY(piv_grid::lds_limit(&lds_limit));
    const Plan p = plan_for(WIN, R, (size_t)lds_limit);         // section 5's plan: a table of ones returns its bits
    if (p.K == 0) return piv_grid::lds_refused("photon_piv_correlate_weighted", WIN, "radius", R, lds_limit);
    PH_TRY(piv_grid::raise_lds(piv_correlate_weighted_kernel<WIN>, p.lds_bytes));
    hipLaunchKernelGGL(piv_correlate_weighted_kernel<WIN>, dim3((unsigned)(n_rows * n_cols)), dim3(p.threads), p.lds_bytes, stream, im1, im2,
                       weight, W, H, step, R, n_cols, offset, p.K, p.nSxp, p.nSyp, vectors, flags, planes);
    PH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int photon_piv_correlate_weighted(const float *d_im1, const float *d_im2, const float *d_weight, int width, int height, int win,
                                             int step, int radius, const int *d_offset, float *d_vectors, int *d_flags, float *d_planes,
                                             int *n_rows, int *n_cols, void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (radius < 1 || radius > win / 2)) bad = "radius must lie in [1, win / 2]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && !d_weight) bad = "null weight table";
    if (!bad && d_vectors && !d_flags) bad = "d_vectors without d_flags";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate_weighted: %s (win %d, step %d, radius %d, %d x %d image)\n", bad, win, step, radius, width,
                height);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate_weighted", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_vectors) return 0;                   // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto WIN) {
        return launch<WIN()>(d_im1, d_im2, d_weight, width, height, step, radius, rows, cols, d_offset, d_vectors, d_flags, d_planes, stream);
    });
}

extern "C" int photon_piv_window_weights(int win, int kind, float param, float *weights) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && kind != 0 && kind != 1) bad = "kind must be 0 (uniform) or 1 (Gaussian)";
    if (!bad && kind == 1 && !(std::isfinite(param) && param > 0.f)) bad = "sigma must be finite and > 0";
    if (!bad && !weights) bad = "null table pointer";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_window_weights: %s (win %d, kind %d, param %g)\n", bad, win, kind, (double)param);
        return 1;
    }
    const double centre = (win - 1) / 2.0, sigma = (double)param;
    for (int y = 0; y < win; y++)
        for (int x = 0; x < win; x++) {
            const double cy = y - centre, cx = x - centre;
            weights[y * win + x] = kind == 0 ? 1.f : (float)exp(-(cy * cy + cx * cx) / (2.0 * sigma * sigma));
        }
    return 0;
}
