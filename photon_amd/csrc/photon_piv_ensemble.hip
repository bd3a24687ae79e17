// photon_piv_ensemble.hip - ensemble (sum-of-correlation) form of the windowed direct cross-correlation: the planes and the
// energies of many image pairs are summed per window before the peak is read, so that pairs too sparse for a peak of their
// own still give one field (steady or periodic flow, a static BOS object, micro-PIV seeding).
// Definition: include/parallel_ray_tracing.h, section 14; host model: photon_amd/piv_ensemble.py (correlate_ensemble_model).
//
// One workgroup per window, looping over the pairs.  A pair is staged and correlated exactly as photon_piv.hip does it (the
// plan and the tile loop are piv_direct.hpp's, the staging pass is repeated below operation for operation), so one pair
// returns section 5's bits.  The running total needs no LDS of its own: it lives in slice 0 of the K partial planes.  The
// lanes of slice 0 sum their tile from zero in registers and store total + tile (the first contributing pair: tile alone),
// the other slices are stored as they are, and after the barrier slices 1 .. K-1 are added into slice 0 in slice order:
// per shift T_k = ((T_(k-1) + S_0) + S_1) + ... + S_(K-1).  Every sum has a fixed order.  A flat pair is block-uniform and
// is skipped whole, barriers included.  After the last pair the peak tail reads slice 0.
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

// LDS layout (floats): photon_piv.hip's -- a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | K partial planes | scratch.
template <int WIN>
__global__ __launch_bounds__(kMaxThreads, 4) void piv_ensemble_kernel(const float *__restrict__ im1_0, const float *__restrict__ im2_0,
                                                                   long long pair_stride, int n_pairs, int W, int H, int step, int R,
                                                                   int n_cols, const int *__restrict__ offset, int K, int nSxp, int nSyp,
                                                                   float *__restrict__ vectors, int *__restrict__ flags,
                                                                   int *__restrict__ count, float *__restrict__ planes) {
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
    const int n_waves = B >> 6;
    const int span = WIN + 2 * R;
    const bool outside = wy0 + oy - R < 0 || wx0 + ox - R < 0 || wy0 + oy + WIN - 1 + R >= H || wx0 + ox + WIN - 1 + R >= W;

    int n_used = 0;                     // contributing pairs so far (block-uniform)
    float Ea = 0.f, Eb = 0.f;           // their energies, summed in pair order from the first one's
    for (int pair = 0; pair < n_pairs; pair++) {
        const float *im1 = im1_0 + (size_t)pair * (size_t)pair_stride;
        const float *im2 = im2_0 + (size_t)pair * (size_t)pair_stride;

        // ---- this pair's window, as photon_piv.hip stages it: the means and the exact flatness counts ...
        const float ref_a = im1[(size_t)wy0 * W + wx0];
        const float ref_b = im2[(size_t)min(max(wy0 + oy, 0), H - 1) * W + min(max(wx0 + ox, 0), W - 1)];
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
        float tot[5] = {sum_a, sum_b, cnt_b, dif_a, dif_b};
        block_reduce(tot, red, n_waves, Sum());     // (its first barrier is also behind every read of the pair before)
        const float cnt = tot[2];
        const bool all_equal = tot[3] == 0.f || tot[4] == 0.f;
        const float mean_a = tot[0] / (float)(WIN * WIN);
        const float mean_b = cnt > 0.f ? tot[1] / cnt : 0.f;

        // ---- ... the mean-subtracted a, the b region with zero padding, the two energies
        float e[2] = {0.f, 0.f};
        for (int i = tid; i < WIN * WIN; i += B) {
            const float v = sa[i] - mean_a;
            sa[i] = v;
            e[0] = fmaf(v, v, e[0]);
        }
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
        if (all_equal || !(ea > 0.f) || !(eb > 0.f)) continue;      // a flat pair (block-uniform) contributes nothing

        // ---- its correlation: slice 0 takes the running total along, the other slices are the pair's own
        const bool first = n_used == 0;
        correlate_tiles<WIN, true>(sa, sb, sp, K, P, pitch, nSxp, nSyp, !first);      // total + tile, never 0 + tile
        __syncthreads();
        // slices 1 .. K-1 into slice 0, in slice order, by the thread that owns the shift in the tail's first pass
        if (K > 1)
            for (int i = tid; i < nS2; i += B) {
                const int j = (i / nS) * nSxp + i % nS;
                float c = sp[j];
                for (int k = 1; k < K; k++) c += sp[k * P + j];
                sp[j] = c;
            }
        Ea = first ? ea : Ea + ea;
        Eb = first ? eb : Eb + eb;
        n_used++;
    }

    if (count && tid == 0) count[win_id] = n_used;
    if (n_used == 0) {                  // flat in every pair
        write_flat(win_id, nS2, outside, vectors, flags, planes);
        return;
    }
    __syncthreads();                    // the last pair's sums into slice 0, for every thread
    const double inv = 1.0 / sqrt((double)Ea * (double)Eb);
    auto plane_at = [&](int sy, int sx) { return sp[sy * nSxp + sx]; };
    peak_tail(plane_at, plane_at, nS, R, ox, oy, inv, outside, win_id, vectors, flags, planes, red, redi);
}

template <int WIN>
int launch(const float *im1, const float *im2, long long pair_stride, int n_pairs, int W, int H, int step, int R, int n_rows, int n_cols,
           const int *offset, float *vectors, int *flags, int *count, float *planes, hipStream_t stream) {
    int lds_limit = 0;
    PH_TRY(piv_grid::lds_limit(&lds_limit));
    const Plan p = plan_for(WIN, R, (size_t)lds_limit);          // section 5's plan: one pair gives its bits
    if (p.K == 0) return piv_grid::lds_refused("photon_piv_correlate_ensemble", WIN, "radius", R, lds_limit);
    PH_TRY(piv_grid::raise_lds(piv_ensemble_kernel<WIN>, p.lds_bytes));
    hipLaunchKernelGGL(piv_ensemble_kernel<WIN>, dim3((unsigned)(n_rows * n_cols)), dim3(p.threads), p.lds_bytes, stream, im1, im2, pair_stride,
                       n_pairs, W, H, step, R, n_cols, offset, p.K, p.nSxp, p.nSyp, vectors, flags, count, planes);
    PH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int photon_piv_correlate_ensemble(const float *d_im1, const float *d_im2, long long pair_stride, int n_pairs, int width, int height,
                                             int win, int step, int radius, const int *d_offset, float *d_vectors, int *d_flags,
                                             int *d_count, float *d_planes, int *n_rows, int *n_cols, void *stream_p) {
    const char *bad = piv_grid::win_error(win);
    if (!bad && (radius < 1 || radius > win / 2)) bad = "radius must lie in [1, win / 2]";
    if (!bad) bad = piv_grid::grid_error(width, height, win, step);
    if (!bad && (!d_im1 || !d_im2)) bad = "null image pointer";
    if (!bad && d_vectors && !d_flags) bad = "d_vectors without d_flags";
    if (!bad && n_pairs < 1) bad = "n_pairs must be >= 1";
    if (!bad && pair_stride < (long long)width * height) bad = "pair_stride is smaller than one image";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate_ensemble: %s (win %d, step %d, radius %d, %d x %d image, %d pairs %lld apart)\n", bad, win,
                step, radius, width, height, n_pairs, pair_stride);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate_ensemble", width, height, win, step, rows, cols, n_rows, n_cols));
    if (!d_vectors) return 0;                   // the size query
    hipStream_t stream = (hipStream_t)stream_p;
    return piv_grid::dispatch_win(win, [&](auto WIN) {
        return launch<WIN()>(d_im1, d_im2, pair_stride, n_pairs, width, height, step, radius, rows, cols, d_offset, d_vectors, d_flags, d_count,
                             d_planes, stream);
    });
}
