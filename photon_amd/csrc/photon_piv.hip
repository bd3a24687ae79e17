// photon_piv.hip - windowed direct cross-correlation of an image pair on the device (PIV / BOS displacement fields):
// the measurement step of a synthetic-image error study, run on the two f32 images while they are still in HBM.
// Definition: include/parallel_ray_tracing.h, section 5; host model: photon_amd/piv_correlation.py (correlate_model).
//
// One workgroup per window.  The mean-subtracted window of im1 (win^2) and of the search region of im2 ((win + 2R)^2,
// b - mean(b), pixels outside the image 0) are staged in LDS.  The (2R+1)^2 shifts are cut into tiles of 4 (x) x 4 (y);
// a lane owns one tile and one of K contiguous slices of the window's rows, walks its rows 4 columns at a time with
// ds_read_b128, and keeps a sliding 8-value strip of each of its 4 im2 rows in registers: per 4 columns 1 + 4 LDS reads
// for 64 FMAs.  The K partial planes are summed in a fixed order; every sum in the kernel has a fixed order, so two calls
// on the same inputs return the same bits.  The plane stays in LDS for the argmax, the ratio and the subpixel fit.
// f32 FMA on the VALU: gfx950's f32 MFMA runs at the VALU's f32 rate and the GEMM form of a correlation doubles the work.
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

// LDS layout (floats): a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | K partial planes [nSyp][nSxp] | reduction scratch.
// nSxp, nSyp: 2R + 1 rounded up to the tile; the shifts past 2R read zero padding and are dropped.
template <int WIN>
__global__ __launch_bounds__(kMaxThreads) void piv_correlate_kernel(const float *__restrict__ im1, const float *__restrict__ im2, int W, int H,
                                                                    int step, int R, int n_cols, const int *__restrict__ offset, int K,
                                                                    int nSxp, int nSyp, float *__restrict__ vectors,
                                                                    int *__restrict__ flags, float *__restrict__ planes) {
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

    // ---- means: a over the window; b over the in-image pixels of the zero-shift window (outside pixels read as that mean);
    //      and how many pixels of each differ from its first one, which decides flatness exactly: an f32 mean of equal
    //      pixels need not reproduce them (counts up to win^2 are exact in f32)
    const float ref_a = im1[(size_t)wy0 * W + wx0];
    const float ref_b = im2[(size_t)min(max(wy0 + oy, 0), H - 1) * W + min(max(wx0 + ox, 0), W - 1)];     // in the window if any pixel is
    float sum_a = 0.f, sum_b = 0.f, cnt_b = 0.f, dif_a = 0.f, dif_b = 0.f;
    for (int i = tid; i < WIN * WIN; i += B) {
        const int y = i / WIN, x = i % WIN;
        const float v = im1[(size_t)(wy0 + y) * W + (wx0 + x)];
        sa[i] = v;
        sum_a += v;
        dif_a += v != ref_a ? 1.f : 0.f;
        const int gy = wy0 + oy + y, gx = wx0 + ox + x;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float u = im2[(size_t)gy * W + gx];
            sum_b += u;
            cnt_b += 1.f;
            dif_b += u != ref_b ? 1.f : 0.f;
        }
    }
    const int n_waves = B >> 6;
    float tot[5] = {sum_a, sum_b, cnt_b, dif_a, dif_b};
    block_reduce(tot, red, n_waves, Sum());                   // 5 x 8 words: reaches into the argmax's index words, idle until the tail
    const float cnt = tot[2];
    const bool all_equal = tot[3] == 0.f || tot[4] == 0.f;  // all pixels of a equal, or all (or none) of b at zero shift
    const float mean_a = tot[0] / (float)(WIN * WIN);
    const float mean_b = cnt > 0.f ? tot[1] / cnt : 0.f;

    // ---- mean-subtracted a in place; the b region with zero padding; the two energies (b at zero shift)
    float e[2] = {0.f, 0.f};            // a, b
    for (int i = tid; i < WIN * WIN; i += B) {
        const float v = sa[i] - mean_a;
        sa[i] = v;
        e[0] = fmaf(v, v, e[0]);
    }
    const int span = WIN + 2 * R;
    for (int i = tid; i < rows * pitch; i += B) {
        const int ry = i / pitch, rx = i % pitch;
        float v = 0.f;
        if (ry < span && rx < span) {
            const int gy = wy0 + oy - R + ry, gx = wx0 + ox - R + rx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = im2[(size_t)gy * W + gx] - mean_b;
            if (ry >= R && ry < R + WIN && rx >= R && rx < R + WIN) e[1] = fmaf(v, v, e[1]);
        }
        sb[i] = v;
    }
    block_reduce(e, red, n_waves, Sum());       // (its barriers also publish sa and sb)
    const float ea = e[0], eb = e[1];

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
int launch(const float *im1, const float *im2, int W, int H, int step, int R, int n_rows, int n_cols, const int *offset,
           float *vectors, int *flags, float *planes, hipStream_t stream) {
    int lds_limit = 0;
    PH_TRY(piv_grid::lds_limit(&lds_limit));
    const Plan p = plan_for(WIN, R, (size_t)lds_limit);
    if (p.K == 0) return piv_grid::lds_refused("photon_piv_correlate", WIN, "radius", R, lds_limit);
    PH_TRY(piv_grid::raise_lds(piv_correlate_kernel<WIN>, p.lds_bytes));
    hipLaunchKernelGGL(piv_correlate_kernel<WIN>, dim3((unsigned)(n_rows * n_cols)), dim3(p.threads), p.lds_bytes, stream, im1, im2, W, H,
                       step, R, n_cols, offset, p.K, p.nSxp, p.nSyp, vectors, flags, planes);
    PH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int photon_piv_correlate(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int radius,
                                    const int *d_offset, float *d_vectors, int *d_flags, float *d_planes, int *n_rows, int *n_cols,
                                    void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (radius < 1 || radius > win / 2)) bad = "radius must lie in [1, win / 2]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && d_vectors && !d_flags) bad = "d_vectors without d_flags";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate: %s (win %d, step %d, radius %d, %d x %d image)\n", bad, win, step, radius, width, height);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_vectors) return 0;                   // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto WIN) {
        return launch<WIN()>(d_im1, d_im2, width, height, step, radius, rows, cols, d_offset, d_vectors, d_flags, d_planes, stream);
    });
}
