// photon_piv_deform.hip - the three device steps of iterative image-deformation correlation (PIV / BOS) beside
// photon_piv_correlate: the cubic B-spline coefficients of an image, the warp of an image by a vector field given on the
// window grid, and the validate-and-update step between two correlations (median test, replacement, accumulation,
// predictor smoothing).  Definition: include/parallel_ray_tracing.h, section 7; host model: photon_amd/piv_deformation.py.
//
//   bspline_coefficients_kernel   one workgroup per 32 x 64 tile: the tile and a 14-pixel mirrored halo in LDS, the
//                                 29-tap FIR along the rows into a second LDS plane, then along the columns to memory
//   deform_kernel (piv_warp.hpp)  one thread per output pixel: bilinear weights of the grid from integer arithmetic, 16
//                                 coefficient taps gathered from global memory (the coefficient image of a 1024^2 frame
//                                 is 4 MB: it stays in L2), one coalesced store
//   validate_kernel               one workgroup per 16 x 16 nodes: the totals of a 22 x 22 neighbourhood in LDS, the
//                                 median test on 20 x 20, the replaced field on 18 x 18, its binomial filter on 16 x 16
//   regrid_kernel                 one thread per node of another window grid: the warp's bilinear weights at the node's
//                                 window centre (section 16: what multigrid refinement carries from level to level)
// No kernel needs device scratch, none writes what another workgroup reads, and every sum has a fixed order: two calls
// on the same inputs return the same bits.
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_grid.hpp"
#include "piv_warp.hpp"

using namespace photon;
using namespace photon::piv_warp;

namespace {

// =============================================================================================
// a. coefficients
// =============================================================================================
constexpr int kFirRadius = 14;              // |z|^15 = 2.6e-9: below f32 rounding
constexpr int kTileW = 64, kTileH = 32;
constexpr int kInW = kTileW + 2 * kFirRadius, kInH = kTileH + 2 * kFirRadius;
constexpr int kFirThreads = 256;

struct FirTaps {
    float h[kFirRadius + 1];                // h[j] = sqrt(3) z^j, z = sqrt(3) - 2, rounded from f64
};

// acc = sum over j = R .. 1 of h[j] (x[-j] + x[+j]), then + h[0] x[0]: small terms first, one order for rows and columns
__device__ __forceinline__ float fir(const FirTaps &t, const float *x, int stride) {
    float acc = 0.f;
#pragma unroll
    for (int j = kFirRadius; j >= 1; j--) acc = acc + t.h[j] * (x[-j * stride] + x[j * stride]);
    return acc + t.h[0] * x[0];
}

__global__ __launch_bounds__(kFirThreads) void bspline_coefficients_kernel(const float *__restrict__ im, int W, int H, FirTaps taps,
                                                                           float *__restrict__ coef) {
    __shared__ float s_in[kInH * kInW];     // the tile and its halo, mirrored at the image's borders
    __shared__ float s_row[kInH * kTileW];  // after the row pass: every row of s_in, the tile's columns
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, tid = threadIdx.x;
    for (int i = tid; i < kInH * kInW; i += kFirThreads) {
        const int ly = i / kInW, lx = i - ly * kInW;
        s_in[i] = im[(size_t)mirror(y0 - kFirRadius + ly, H) * W + mirror(x0 - kFirRadius + lx, W)];
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTileW; i += kFirThreads) {
        const int ly = i / kTileW, lx = i - ly * kTileW;
        s_row[i] = fir(taps, s_in + ly * kInW + lx + kFirRadius, 1);
    }
    __syncthreads();
    for (int i = tid; i < kTileH * kTileW; i += kFirThreads) {
        const int ly = i / kTileW, lx = i - ly * kTileW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < H && gx < W) coef[(size_t)gy * W + gx] = fir(taps, s_row + (ly + kFirRadius) * kTileW + lx, kTileW);
    }
}

// =============================================================================================
// b. warp
// =============================================================================================
// deform_kernel<GridField>: piv_warp.hpp, shared with the per-pixel warp of photon_optflow.hip

// =============================================================================================
// c. validate and update
// =============================================================================================
constexpr int kValTile = 16, kValThreads = 256;
constexpr int kTotW = kValTile + 6, kOutW = kValTile + 4, kFldW = kValTile + 2;

// ascending sort of 8 values (odd-even transposition; absent values are +inf and end up last)
__device__ __forceinline__ void sort8(double v[8]) {
#pragma unroll
    for (int round = 0; round < 8; round++)
#pragma unroll
        for (int i = round & 1; i + 1 < 8; i += 2) {
            const double lo = fmin(v[i], v[i + 1]), hi = fmax(v[i], v[i + 1]);
            v[i] = lo;
            v[i + 1] = hi;
        }
}

// median of the first n (1 <= n <= 8) of 8 sorted values: the middle one, or (lo + hi) / 2 of the middle two
__device__ __forceinline__ double median_sorted(const double v[8], int n) {
    const int a = (n - 1) >> 1, b = n >> 1;
    double lo = 0.0, hi = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        lo = i == a ? v[i] : lo;
        hi = i == b ? v[i] : hi;
    }
    return (lo + hi) / 2.0;
}

// The 8 neighbours of (y, x) in a plane of pitch `pitch` (2 doubles per node), component c, row-major order; `use`
// says which take part.  Returns how many do; v holds them sorted, the others +inf.
template <typename Use>
__device__ __forceinline__ int neighbours(const double *plane, int pitch, int y, int x, int c, Use use, double v[8]) {
    int n = 0, k = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if (dy == 0 && dx == 0) continue;
            const bool ok = use(dy, dx);
            v[k++] = ok ? plane[2 * ((y + dy) * pitch + (x + dx)) + c] : INFINITY;
            n += ok ? 1 : 0;
        }
    sort8(v);
    return n;
}

__global__ __launch_bounds__(kValThreads) void validate_kernel(const float *__restrict__ pred, const float *__restrict__ vectors,
                                                               const int *__restrict__ flags, int n_rows, int n_cols, double eps,
                                                               double thr2, float *__restrict__ field, float *__restrict__ smooth,
                                                               int *__restrict__ status) {
    __shared__ double s_tot[kTotW * kTotW * 2];     // totals, NaN beyond the grid: nodes tile - 3 .. tile + 18
    __shared__ unsigned char s_out[kOutW * kOutW];  // outliers: nodes tile - 2 .. tile + 17 (0 beyond the grid)
    __shared__ double s_fld[kFldW * kFldW * 2];     // the field of step 3: nodes tile - 1 .. tile + 16
    const int i0 = blockIdx.y * kValTile, j0 = blockIdx.x * kValTile, tid = threadIdx.x;
    const double qnan = __builtin_nan("");

    for (int k = tid; k < kTotW * kTotW; k += kValThreads) {
        const int i = i0 - 3 + k / kTotW, j = j0 - 3 + k % kTotW;
        double tx = qnan, ty = qnan;
        if (i >= 0 && i < n_rows && j >= 0 && j < n_cols) {
            const size_t g = (size_t)i * n_cols + j;
            if (!(flags[g] & 2)) {
                // + 0.0: a total of -0 reads as +0, so that no sign of zero depends on the order of a selection
                const double x = ((pred ? (double)pred[2 * g] : 0.0) + (double)vectors[4 * g]) + 0.0;
                const double y = ((pred ? (double)pred[2 * g + 1] : 0.0) + (double)vectors[4 * g + 1]) + 0.0;
                if (isfinite(x) && isfinite(y)) {
                    tx = x;
                    ty = y;
                }
            }
        }
        s_tot[2 * k] = tx;
        s_tot[2 * k + 1] = ty;
    }
    __syncthreads();

    for (int k = tid; k < kOutW * kOutW; k += kValThreads) {
        const int ly = k / kOutW + 1, lx = k % kOutW + 1;          // in s_tot
        const int i = i0 - 3 + ly, j = j0 - 3 + lx;
        unsigned char o = 0;
        if (i >= 0 && i < n_rows && j >= 0 && j < n_cols) {
            const double t0x = s_tot[2 * (ly * kTotW + lx)];
            if (t0x != t0x) o = 1;                                 // not finite (both components are NaN then)
            else {
                double r2 = 0.0;
                int n = 0;
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    double v[8];
                    n = neighbours(s_tot, kTotW, ly, lx, c, [&](int dy, int dx) {
                            const double t = s_tot[2 * ((ly + dy) * kTotW + (lx + dx))];
                            return t == t; }, v);
                    if (n == 0) break;
                    const double med = median_sorted(v, n);
#pragma unroll
                    for (int q = 0; q < 8; q++) v[q] = q < n ? fabs(v[q] - med) : INFINITY;
                    sort8(v);
                    const double rm = median_sorted(v, n);
                    const double r = fabs(s_tot[2 * (ly * kTotW + lx) + c] - med) / (rm + eps);
                    r2 = c == 0 ? r * r : r2 + r * r;
                }
                o = (n > 0 && r2 > thr2) ? 1 : 0;
            }
        }
        s_out[k] = o;
    }
    __syncthreads();

    for (int k = tid; k < kFldW * kFldW; k += kValThreads) {
        const int fy = k / kFldW, fx = k % kFldW;
        const int i = i0 - 1 + fy, j = j0 - 1 + fx;
        double vx = 0.0, vy = 0.0;
        if (i >= 0 && i < n_rows && j >= 0 && j < n_cols) {
            const int ly = fy + 2, lx = fx + 2, oy = fy + 1, ox = fx + 1;
            if (s_out[oy * kOutW + ox]) {
                auto use = [&](int dy, int dx) {
                    const double t = s_tot[2 * ((ly + dy) * kTotW + (lx + dx))];
                    return t == t && !s_out[(oy + dy) * kOutW + (ox + dx)];
                };
                double v[8];
                int n = neighbours(s_tot, kTotW, ly, lx, 0, use, v);
                if (n > 0) {
                    vx = median_sorted(v, n);
                    n = neighbours(s_tot, kTotW, ly, lx, 1, use, v);
                    vy = median_sorted(v, n);
                }
            } else {
                vx = s_tot[2 * (ly * kTotW + lx)];
                vy = s_tot[2 * (ly * kTotW + lx) + 1];
            }
            if (fy >= 1 && fy <= kValTile && fx >= 1 && fx <= kValTile) {
                const size_t g = (size_t)i * n_cols + j;
                field[2 * g] = (float)vx;
                field[2 * g + 1] = (float)vy;
                status[g] = flags[g] | (s_out[oy * kOutW + ox] ? 8 : 0);
            }
        }
        s_fld[2 * k] = vx;
        s_fld[2 * k + 1] = vy;
    }
    if (!smooth) return;
    __syncthreads();

    {   // [1 2 1] / 4 along the row, then along the column, edge values replicated: ((a + 2 b) + c) / 4 each time
        const int ty = tid / kValTile, tx = tid % kValTile;
        const int i = i0 + ty, j = j0 + tx;
        if (i < n_rows && j < n_cols) {
            const int ya[3] = {max(i - 1, 0) - i0 + 1, ty + 1, min(i + 1, n_rows - 1) - i0 + 1};
            const int xa[3] = {max(j - 1, 0) - j0 + 1, tx + 1, min(j + 1, n_cols - 1) - j0 + 1};
#pragma unroll
            for (int c = 0; c < 2; c++) {
                double h[3];
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    const double *row = s_fld + 2 * (ya[u] * kFldW) + c;
                    h[u] = ((row[2 * xa[0]] + 2.0 * row[2 * xa[1]]) + row[2 * xa[2]]) / 4.0;
                }
                smooth[2 * ((size_t)i * n_cols + j) + c] = (float)(((h[0] + 2.0 * h[1]) + h[2]) / 4.0);
            }
        }
    }
}

// =============================================================================================
// d. regrid (section 16)
// =============================================================================================
// one thread per node of the destination grid: GridField at the node's window centre, one 8-byte store
__global__ __launch_bounds__(kWarpX *kWarpY) void regrid_kernel(GridField D, int dst_win, int dst_step, int dst_rows, int dst_cols,
                                                                float2 *__restrict__ dst) {
    const int j = blockIdx.x * kWarpX + threadIdx.x, i = blockIdx.y * kWarpY + threadIdx.y;
    if (j >= dst_cols || i >= dst_rows) return;
    float dx, dy;
    D.at_centre(i, j, dst_win, dst_step, dx, dy);
    dst[(size_t)i * dst_cols + j] = make_float2(dx, dy);
}

}  // namespace

extern "C" int photon_piv_bspline_coefficients(const float *d_im, int width, int height, float *d_coef, void *stream_p) {
    const char *bad = nullptr;
    if (width < 1 || height < 1) bad = "width and height must be >= 1";
    else if (!d_im || !d_coef) bad = "null image pointer";
    else if (d_im == d_coef) bad = "d_coef must not be d_im";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_bspline_coefficients: %s (%d x %d image)\n", bad, width, height);
        return 1;
    }
    FirTaps taps;
    const double z = std::sqrt(3.0) - 2.0;
    double p = std::sqrt(3.0);
    for (int j = 0; j <= kFirRadius; j++, p *= z) taps.h[j] = (float)p;
    const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(bspline_coefficients_kernel, grid, dim3(kFirThreads), 0, (hipStream_t)stream_p, d_im, width, height, taps, d_coef);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_deform(const float *d_coef, int width, int height, const float *d_field, int field_stride, int n_rows,
                                 int n_cols, int win, int step, float scale, float *d_out, void *stream_p) {
    const char *bad = piv_grid::grid_error(width, height, win, step, n_rows, n_cols);
    if (!bad) {
        if (field_stride != 2 && field_stride != 4) bad = "field_stride must be 2 or 4";
        else if (width > (1 << 22) || height > (1 << 22)) bad = "the image is larger than 2^22 pixels a side";
        else if (!std::isfinite(scale)) bad = "scale must be finite";
        else if (!d_coef || !d_field || !d_out) bad = "null d_coef, d_field or d_out";
        else if (d_coef == d_out) bad = "d_out must not be d_coef";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_deform: %s (win %d, step %d, %d x %d image, %d x %d grid, stride %d, scale %g)\n", bad, win,
                step, width, height, n_rows, n_cols, field_stride, (double)scale);
        return 1;
    }
    const GridField D{d_field, field_stride, n_rows, n_cols, win, step, 1.f / (float)(2 * step)};
    hipLaunchKernelGGL(deform_kernel<GridField>, warp_grid(width, height), dim3(kWarpX, kWarpY), 0, (hipStream_t)stream_p, d_coef, width, height, D,
                       scale, d_out);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_validate(const float *d_pred, const float *d_vectors, const int *d_flags, int n_rows, int n_cols, double eps,
                                   double threshold, float *d_field, float *d_smooth, int *d_status, void *stream_p) {
    const char *bad = nullptr;
    if (n_rows < 1 || n_cols < 1) bad = "n_rows and n_cols must be >= 1";
    else if ((long long)n_rows * n_cols > INT_MAX) bad = "more than INT_MAX windows";
    else if (!(eps >= 0.0) || !std::isfinite(eps)) bad = "eps must be finite and >= 0";
    else if (!(threshold > 0.0) || !std::isfinite(threshold)) bad = "threshold must be finite and > 0";
    else if (!d_vectors || !d_flags || !d_field || !d_status) bad = "null d_vectors, d_flags, d_field or d_status";
    else if (d_pred && (d_pred == d_field || d_pred == d_smooth)) bad = "d_pred must not be an output";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_validate: %s (%d x %d grid, eps %g, threshold %g)\n", bad, n_rows, n_cols, eps, threshold);
        return 1;
    }
    const dim3 grid((unsigned)((n_cols + kValTile - 1) / kValTile), (unsigned)((n_rows + kValTile - 1) / kValTile));
    hipLaunchKernelGGL(validate_kernel, grid, dim3(kValThreads), 0, (hipStream_t)stream_p, d_pred, d_vectors, d_flags, n_rows, n_cols, eps,
                       threshold * threshold, d_field, d_smooth, d_status);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_regrid(const float *d_src, int src_stride, int src_rows, int src_cols, int src_win, int src_step, int width,
                                 int height, int dst_win, int dst_step, float *d_dst, int *dst_rows, int *dst_cols, void *stream_p) {
    const char *bad = piv_grid::grid_error(width, height, src_win, src_step, src_rows, src_cols);
    if (!bad) bad = piv_grid::grid_error(width, height, dst_win, dst_step);
    if (!bad) {
        if (src_stride != 2 && src_stride != 4) bad = "src_stride must be 2 or 4";
        else if (width > (1 << 22) || height > (1 << 22)) bad = "the image is larger than 2^22 pixels a side";
        else if ((long long)src_rows * src_cols > INT_MAX) bad = "more than INT_MAX source windows";
        else if (!d_src) bad = "null d_src";
        else if (d_dst == d_src) bad = "d_dst must not be d_src";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_regrid: %s (%d x %d image, source win %d, step %d, %d x %d grid, stride %d; destination win %d, step %d)\n",
                bad, width, height, src_win, src_step, src_rows, src_cols, src_stride, dst_win, dst_step);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_regrid", width, height, dst_win, dst_step, rows, cols, dst_rows, dst_cols));
    if (!d_dst) return 0;                       // the size query
    const GridField D{d_src, src_stride, src_rows, src_cols, src_win, src_step, 1.f / (float)(2 * src_step)};
    hipLaunchKernelGGL(regrid_kernel, warp_grid(cols, rows), dim3(kWarpX, kWarpY), 0, (hipStream_t)stream_p, D, dst_win, dst_step, rows, cols,
                       reinterpret_cast<float2 *>(d_dst));
    PH_CHECK(hipGetLastError());
    return 0;
}
