// photon_piv_masked.hip - section 5's direct correlation with excluded pixels (a model, a wall, the region outside the
// laser sheet): two u8 masks in image coordinates, one per frame.  Definition: include/parallel_ray_tracing.h, section 17;
// host model: photon_amd/piv_mask.py (correlate_masked_model); DESIGN.md section 4.3p.
//
// One workgroup per window, section 5's plan (piv_direct::plan_for), tile loop and peak tail.  A window no mask touches
// runs section 5's arithmetic operation by operation and returns its bits.  A window a mask touches correlates twice: the
// pixels (invalid ones staged as 0 after the mean), then the two 0/1 validity planes, restaged into the a / b areas once
// the K partial planes of C are summed into plane 0; the pair counts N(s) are small integers, exact in f32 in any order,
// and land in the planes behind plane 0.  The peak tail's first pass divides as it meets each shift.  The path is chosen
// from block-wide totals, so it is uniform over the workgroup.  The value under a mask is never loaded.
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

constexpr int kMaskedOut = 16, kPartial = 32;

// the planes a launch keeps in LDS: section 5's K for C, and room for one plane of N behind plane 0 when K is 1
inline int planes_for(int K) { return std::max(K, 2); }

// LDS layout (floats): a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | max(K, 2) planes [nSyp][nSxp] | reduction scratch.
template <int WIN>
__global__ __launch_bounds__(kMaxThreads) void piv_correlate_masked_kernel(const float *__restrict__ im1, const float *__restrict__ im2,
                                                                           const unsigned char *__restrict__ m1,
                                                                           const unsigned char *__restrict__ m2, int W, int H, int step, int R,
                                                                           int n_cols, const int *__restrict__ offset, int K, int nSxp,
                                                                           int nSyp, int min_valid, float *__restrict__ vectors,
                                                                           int *__restrict__ flags, int *__restrict__ valid,
                                                                           float *__restrict__ planes) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nS = 2 * R + 1, nS2 = nS * nS;
    const int pitch = WIN + nSxp, rows = WIN + nSyp - 1, P = nSyp * nSxp;
    float *sa = lds;
    float *sb = sa + WIN * WIN;
    float *sp = sb + rows * pitch;
    float *red = sp + (K > 2 ? K : 2) * P;
    int *redi = reinterpret_cast<int *>(red + 32);

    const int win_id = blockIdx.x;
    const int wy0 = (win_id / n_cols) * step, wx0 = (win_id % n_cols) * step;
    const int ox = offset ? offset[2 * win_id] : 0, oy = offset ? offset[2 * win_id + 1] : 0;
    const int tid = threadIdx.x, B = blockDim.x;
    const int span = WIN + 2 * R;

    // ---- sums, counts and extremes over the valid pixels: a over the window, b over the zero-shift window; and how many
    //      masked pixels b's search region holds inside the image (a's are win^2 - n_a)
    float sum_a = 0.f, sum_b = 0.f, cnt_a = 0.f, cnt_b = 0.f, hid_b = 0.f;
    float ext[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};      // max a, -min a, max b, -min b
    for (int i = tid; i < WIN * WIN; i += B) {
        const int y = i / WIN, x = i % WIN;
        const size_t p = (size_t)(wy0 + y) * W + (wx0 + x);
        float v = 0.f;
        if (!m1 || m1[p] == 0) {
            v = im1[p];
            sum_a += v;
            cnt_a += 1.f;
            ext[0] = fmaxf(ext[0], v);
            ext[1] = fmaxf(ext[1], -v);
        }
        sa[i] = v;
        const int gy = wy0 + oy + y, gx = wx0 + ox + x;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t q = (size_t)gy * W + gx;
            if (!m2 || m2[q] == 0) {
                const float u = im2[q];
                sum_b += u;
                cnt_b += 1.f;
                ext[2] = fmaxf(ext[2], u);
                ext[3] = fmaxf(ext[3], -u);
            }
        }
    }
    if (m2)
        for (int i = tid; i < span * span; i += B) {
            const int gy = wy0 + oy - R + i / span, gx = wx0 + ox - R + i % span;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W && m2[(size_t)gy * W + gx] != 0) hid_b += 1.f;
        }
    const int n_waves = B >> 6;
    float tot[5] = {sum_a, sum_b, cnt_a, cnt_b, hid_b};        // counts up to (win + 2R)^2 are exact in f32
    block_reduce(tot, red, n_waves, Sum());
    block_reduce(ext, red, n_waves, MaxF32());
    const float na = tot[2], nb = tot[3];
    const bool hid_a = na < (float)(WIN * WIN), hid_any = hid_a || tot[4] > 0.f;
    const bool outside = wy0 + oy - R < 0 || wx0 + ox - R < 0 || wy0 + oy + WIN - 1 + R >= H || wx0 + ox + WIN - 1 + R >= W;
    if (valid && tid == 0) {
        valid[2 * (size_t)win_id + 0] = (int)na;
        valid[2 * (size_t)win_id + 1] = (int)nb;
    }
    // masked out (block-uniform): too few valid pixels in either window
    if (na < (float)min_valid || nb < (float)min_valid) {
        write_flat(win_id, nS2, outside, vectors, flags, planes);
        if (tid == 0) flags[win_id] = kMaskedOut | (outside ? 4 : 0);
        return;
    }
    const int touched = hid_any ? kPartial : 0;
    const bool all_equal = ext[0] == -ext[1] || ext[2] == -ext[3];  // the valid pixels of a, or of b at zero shift, all equal
    const float mean_a = tot[0] / na;
    const float mean_b = tot[1] / nb;

    // ---- mean-subtracted a in place; the b region with zero padding; the two energies (b at zero shift).  A mask is read
    //      again only where the window saw one of its pixels.
    const unsigned char *ma = hid_a ? m1 : nullptr, *mb = tot[4] > 0.f ? m2 : nullptr;
    float e[2] = {0.f, 0.f};            // a, b
    for (int i = tid; i < WIN * WIN; i += B) {
        float v = sa[i] - mean_a;
        if (ma && ma[(size_t)(wy0 + i / WIN) * W + (wx0 + i % WIN)] != 0) v = 0.f;
        sa[i] = v;
        e[0] = fmaf(v, v, e[0]);
    }
    for (int i = tid; i < rows * pitch; i += B) {
        const int ry = i / pitch, rx = i % pitch;
        float v = 0.f;
        if (ry < span && rx < span) {
            const int gy = wy0 + oy - R + ry, gx = wx0 + ox - R + rx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t q = (size_t)gy * W + gx;
                if (!mb || mb[q] == 0) v = im2[q] - mean_b;
            }
            if (ry >= R && ry < R + WIN && rx >= R && rx < R + WIN) e[1] = fmaf(v, v, e[1]);
        }
        sb[i] = v;
    }
    block_reduce(e, red, n_waves, Sum());       // (its barriers also publish sa and sb)
    const float ea = e[0], eb = e[1];

    // flat window (block-uniform): by its valid pixels, or a contrast too small for the f32 energies
    if (all_equal || !(ea > 0.f) || !(eb > 0.f)) {
        write_flat(win_id, nS2, outside, vectors, flags, planes);
        if (touched && tid == 0) flags[win_id] |= touched;
        return;
    }

    // ---- the correlation of the pixels: every lane's tile into its slice's partial plane
    correlate_tiles<WIN>(sa, sb, sp, K, P, pitch, nSxp, nSyp);
    __syncthreads();
    const double inv = 1.0 / sqrt((double)ea * (double)eb);
    auto plane_at = [&](int sy, int sx) { return sp[sy * nSxp + sx]; };

    if (!touched) {         // section 5 from here on, operation by operation
        auto sum_slices = [&](int sy, int sx) {
            const int j = sy * nSxp + sx;
            float c = sp[j];
            for (int k = 1; k < K; k++) c += sp[k * P + j];
            sp[j] = c;
            return c;
        };
        peak_tail(sum_slices, plane_at, nS, R, ox, oy, inv, outside, win_id, vectors, flags, planes, red, redi);
        return;
    }

    // ---- C into plane 0 (the slices in section 5's order); the validity planes into the a / b areas; N behind plane 0
    for (int j = tid; j < P; j += B) {
        float c = sp[j];
        for (int k = 1; k < K; k++) c += sp[k * P + j];
        sp[j] = c;
    }
    for (int i = tid; i < WIN * WIN; i += B) sa[i] = ma && ma[(size_t)(wy0 + i / WIN) * W + (wx0 + i % WIN)] != 0 ? 0.f : 1.f;
    for (int i = tid; i < rows * pitch; i += B) {
        const int ry = i / pitch, rx = i % pitch;
        float v = 0.f;
        if (ry < span && rx < span) {
            const int gy = wy0 + oy - R + ry, gx = wx0 + ox - R + rx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W && (!mb || mb[(size_t)gy * W + gx] == 0)) v = 1.f;
        }
        sb[i] = v;
    }
    __syncthreads();
    float *sn = sp + P;
    const int Kn = K > 2 ? K - 1 : 1;
    correlate_tiles<WIN>(sa, sb, sn, Kn, P, pitch, nSxp, nSyp);
    __syncthreads();

    // ---- C' = C n_a / N where at least half of a's valid pixels keep a partner, 0 elsewhere; the peak read-out
    auto normalise = [&](int sy, int sx) {
        const int j = sy * nSxp + sx;
        float n = sn[j];
        for (int k = 1; k < Kn; k++) n += sn[k * P + j];
        const float c = 2.f * n >= na ? (float)((double)sp[j] * (double)na / (double)n) : 0.f;
        sp[j] = c;
        return c;
    };
    peak_tail(normalise, plane_at, nS, R, ox, oy, inv, outside, win_id, vectors, flags, planes, red, redi);
    if (tid == 0) flags[win_id] |= touched;
}

template <int WIN>
int launch(const float *im1, const float *im2, const unsigned char *m1, const unsigned char *m2, int W, int H, int step, int R, int n_rows,
           int n_cols, int min_valid, const int *offset, float *vectors, int *flags, int *valid, float *planes, hipStream_t stream) {
    int lds_limit = 0;
    PH_TRY(piv_grid::lds_limit(&lds_limit));
    const Plan p = plan_for(WIN, R, (size_t)lds_limit);         // section 5's plan: the untouched windows return its bits
    if (p.K == 0) return piv_grid::lds_refused("photon_piv_correlate_masked", WIN, "radius", R, lds_limit);
    const size_t lds_bytes = p.lds_bytes + 4 * (size_t)(planes_for(p.K) - p.K) * p.nSxp * p.nSyp;
    if (lds_bytes > (size_t)lds_limit) return piv_grid::lds_refused("photon_piv_correlate_masked", WIN, "radius", R, lds_limit);
    PH_TRY(piv_grid::raise_lds(piv_correlate_masked_kernel<WIN>, lds_bytes));
    hipLaunchKernelGGL(piv_correlate_masked_kernel<WIN>, dim3((unsigned)(n_rows * n_cols)), dim3(p.threads), lds_bytes, stream, im1, im2, m1,
                       m2, W, H, step, R, n_cols, offset, p.K, p.nSxp, p.nSyp, min_valid, vectors, flags, valid, planes);
    PH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int photon_piv_correlate_masked(const float *d_im1, const float *d_im2, const unsigned char *d_mask1, const unsigned char *d_mask2,
                                           int width, int height, int win, int step, int radius, int min_valid, const int *d_offset,
                                           float *d_vectors, int *d_flags, int *d_valid, float *d_planes, int *n_rows, int *n_cols,
                                           void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (radius < 1 || radius > win / 2)) bad = "radius must lie in [1, win / 2]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && d_vectors && !d_flags) bad = "d_vectors without d_flags";
    if (!bad && (min_valid < 1 || min_valid > win * win)) bad = "min_valid must lie in [1, win^2]";
    if (!bad && d_valid && !d_vectors) bad = "d_valid without d_vectors";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate_masked: %s (win %d, step %d, radius %d, min_valid %d, %d x %d image)\n", bad, win, step,
                radius, min_valid, width, height);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate_masked", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_vectors) return 0;                   // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto WIN) {
        return launch<WIN()>(d_im1, d_im2, d_mask1, d_mask2, width, height, step, radius, rows, cols, min_valid, d_offset, d_vectors, d_flags,
                             d_valid, d_planes, stream);
    });
}
