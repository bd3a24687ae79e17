// photon_piv_stereo.hip - stereo PIV beside the planar correlators: the frames of a camera resampled onto a grid on the
// light sheet's plane through the camera's polynomial, two cameras' 2-C fields on that grid combined into three
// components per node, and the disparity between the two dewarped views triangulated into points of the sheet.  Definition: include/parallel_ray_tracing.h, section 19; host models: photon_amd/piv_stereo.py.
//
//   dewarp_kernel        one thread per output pixel: where the pixel lands on the sensor (piv_camera.hpp, sensor_point: two
//                        bivariate cubics in f64, the fraction taken in f64 and rounded once), section 7b's weights and
//                        mirrors (piv_warp.hpp, BsplineTaps) computed once, then per frame 16 coefficient taps gathered
//                        from global memory and one coalesced store
//   reconstruct_kernel   one thread per node: two analytic 2 x 3 Jacobians, the 3 x 3 normal equations of four equations,
//                        Cholesky, the residual and the propagated sigmas, all in f64 in a fixed order
//   triangulate_kernel   one thread per node of a disparity field between the two cameras' dewarped frames: the two image
//                        points, then Gauss-Newton steps for the world point both saw -- per step two polynomial
//                        evaluations, the two Jacobians and the 3 x 3 Cholesky of the reconstruction -- in f64 in a fixed order
// Host rules: piv_camera.hpp.  No kernel needs device scratch or LDS, none writes what another thread reads: two calls return the same bits.
#include <cmath>

#include "photon_internal.hpp"
#include "piv_camera.hpp"
#include "piv_grid.hpp"
#include "piv_warp.hpp"

using namespace photon;
using namespace photon::piv_camera;
using namespace photon::piv_warp;

namespace {

// =============================================================================================
// a. dewarp
// =============================================================================================
struct DewarpArgs {
    const float *coef;
    long long in_stride, out_stride;
    int n_frames, W, H, OW, OH;
    double poly[2][10], grid[4];
    float *out;
    unsigned char *mask;
};

__global__ __launch_bounds__(kWarpX *kWarpY) void dewarp_kernel(const DewarpArgs a) {
    const int j = blockIdx.x * kWarpX + threadIdx.x, i = blockIdx.y * kWarpY + threadIdx.y;
    if (j >= a.OW || i >= a.OH) return;
    const size_t o = (size_t)i * a.OW + j;
    SensorPoint p;
    const bool inside = sensor_point(&a.poly[0][0], a.grid, i, j, a.W, a.H, p);
    if (a.mask) a.mask[o] = inside ? 0 : 1;
    if (!inside) {
        for (int f = 0; f < a.n_frames; f++) a.out[(size_t)f * a.out_stride + o] = 0.f;
        return;
    }
    const BsplineTaps taps(p.ix, p.iy, p.fx, p.fy, a.W, a.H);
    for (int f = 0; f < a.n_frames; f++) a.out[(size_t)f * a.out_stride + o] = taps.sample(a.coef + (size_t)f * a.in_stride);
}

// =============================================================================================
// b. reconstruction
// =============================================================================================
constexpr int kNodeThreads = 256;
constexpr double kMinPivotRatio = 1e-12;

struct StereoArgs {
    const float *field1, *field2, *sigma1, *sigma2;
    const int *flags1, *flags2;
    int stride, n_rows, n_cols, win, step;
    photon_piv_plane_t plane;
    photon_piv_camera_t cam[2];
    double *out;
    int *flags;
};

// J = d(x, y) / d(X, Y, Z) of the camera at the world point P (section 19b, step 1)
__device__ __forceinline__ void jacobian(const photon_piv_camera_t &c, const double P[3], double J[2][3]) {
    const double X = (P[0] - c.centre[0]) / c.scale[0], Y = (P[1] - c.centre[1]) / c.scale[1], Z = (P[2] - c.centre[2]) / c.scale[2];
    const double XX = X * X, YY = Y * Y, ZZ = Z * Z, X2 = 2.0 * X, Y2 = 2.0 * Y, Z2 = 2.0 * Z;
    const double D[3][19] = {{0.0, 1.0, 0.0, 0.0, X2, Y, 0.0, Z, 0.0, 0.0, 3.0 * XX, X2 * Y, YY, 0.0, X2 * Z, Y * Z, 0.0, ZZ, 0.0},
                             {0.0, 0.0, 1.0, 0.0, 0.0, X, Y2, 0.0, Z, 0.0, 0.0, XX, X2 * Y, 3.0 * YY, 0.0, X * Z, Y2 * Z, 0.0, ZZ},
                             {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, X, Y, Z2, 0.0, 0.0, 0.0, 0.0, XX, X * Y, YY, X2 * Z, Y2 * Z}};
#pragma unroll
    for (int axis = 0; axis < 3; axis++) {
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < 19; k++) {
            sx = sx + c.cx[k] * D[axis][k];
            sy = sy + c.cy[k] * D[axis][k];
        }
        J[0][axis] = sx / c.scale[axis];
        J[1][axis] = sy / c.scale[axis];
    }
}

// the node's point on the plane: the centre of window (i, j) of section 5's grid
__device__ __forceinline__ void node_point(const photon_piv_plane_t &plane, int win, int step, int i, int j, double P[3]) {
    const double half = (double)(win - 1) / 2.0;
    P[0] = plane.x0 + ((double)(j * step) + half) * plane.pitch;
    P[1] = plane.y0 + ((double)(i * step) + half) * plane.pitch;
    P[2] = plane.z;
}

struct Cholesky3 {
    double l00, l10, l20, l11, l21, l22;
    // N = L L^T.  Returns the smallest pivot over the largest; ok: that is above kMinPivotRatio and every pivot above 0 (no NaN)
    __device__ __forceinline__ double factor(const double N[3][3], bool &ok) {
        const double d0 = N[0][0];
        l00 = sqrt(d0);
        l10 = N[1][0] / l00;
        l20 = N[2][0] / l00;
        const double d1 = N[1][1] - l10 * l10;
        l11 = sqrt(d1);
        l21 = (N[2][1] - l20 * l10) / l11;
        const double d2 = (N[2][2] - l20 * l20) - l21 * l21;
        l22 = sqrt(d2);
        const double ratio = fmin(fmin(d0, d1), d2) / fmax(fmax(d0, d1), d2);
        ok = ratio > kMinPivotRatio && d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
        return ratio;
    }
    __device__ __forceinline__ void solve(const double r[3], double z[3]) const {
        const double y0 = r[0] / l00;
        const double y1 = (r[1] - l10 * y0) / l11;
        const double y2 = ((r[2] - l20 * y0) - l21 * y1) / l22;
        z[2] = y2 / l22;
        z[1] = (y1 - l21 * z[2]) / l11;
        z[0] = ((y0 - l10 * z[1]) - l20 * z[2]) / l00;
    }
};

__global__ __launch_bounds__(kNodeThreads) void reconstruct_kernel(const StereoArgs a) {
    const int k = blockIdx.x * kNodeThreads + threadIdx.x;
    if (k >= a.n_rows * a.n_cols) return;
    const int i = k / a.n_cols, j = k - i * a.n_cols;
    const double qnan = __builtin_nan(""), pitch = a.plane.pitch;
    double P[3];
    node_point(a.plane, a.win, a.step, i, j, P);
    const float *f[2] = {a.field1 + (size_t)k * a.stride, a.field2 + (size_t)k * a.stride};
    const float *sg[2] = {a.sigma1 ? a.sigma1 + 2 * (size_t)k : nullptr, a.sigma2 ? a.sigma2 + 2 * (size_t)k : nullptr};
    int flag = (a.flags1 ? a.flags1[k] : 0) | (a.flags2 ? a.flags2[k] : 0);

    double J[2][2][3], A[4][3], b[4];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        jacobian(a.cam[c], P, J[c]);
        const float dx = f[c][0], dy = f[c][1];
        finite = finite && isfinite(dx) && isfinite(dy);
        const double a0 = pitch * (double)dx, a1 = pitch * (double)dy;
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int m = 0; m < 3; m++) A[2 * c + r][m] = J[c][r][m];
            b[2 * c + r] = J[c][r][0] * a0 + J[c][r][1] * a1;
        }
    }
    double N[3][3], r[3];
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
        for (int q = 0; q < 3; q++) N[p][q] = ((A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]) + A[3][p] * A[3][q];
        r[p] = ((A[0][p] * b[0] + A[1][p] * b[1]) + A[2][p] * b[2]) + A[3][p] * b[3];
    }
    Cholesky3 L;
    bool ok;
    const double ratio = L.factor(N, ok);

    double out[8] = {qnan, qnan, qnan, qnan, qnan, qnan, qnan, qnan};
    if (!ok) flag |= 64;
    else {
        out[7] = ratio;
        if (finite) {
            double D[3];
            L.solve(r, D);
            double ss = 0.0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const double e = ((A[m][0] * D[0] + A[m][1] * D[1]) + A[m][2] * D[2]) - b[m];
                ss = ss + e * e;
            }
            out[0] = D[0];
            out[1] = D[1];
            out[2] = D[2];
            out[3] = sqrt(ss);
            if (sg[0] && sg[1]) {
                double inv[3][3];           // inv[col] = N^-1 e_col; N^-1 is symmetric up to rounding: its entry (p, col) is inv[col][p]
#pragma unroll
                for (int col = 0; col < 3; col++) {
                    const double e[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0};
                    L.solve(e, inv[col]);
                }
                double var[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const double s[2] = {pitch * (double)sg[c][0], pitch * (double)sg[c][1]};
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        double M[2];
#pragma unroll
                        for (int rr = 0; rr < 2; rr++) {
                            const double *row = A[2 * c + rr];
                            M[rr] = (inv[0][p] * row[0] + inv[1][p] * row[1]) + inv[2][p] * row[2];
                        }
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            const double g = M[0] * J[c][0][m] + M[1] * J[c][1][m];
                            var[p] = var[p] + (g * g) * (s[m] * s[m]);
                        }
                    }
                }
                out[4] = sqrt(var[0]);
                out[5] = sqrt(var[1]);
                out[6] = sqrt(var[2]);
            }
        }
    }
    if (!finite) flag |= 128;
#pragma unroll
    for (int m = 0; m < 8; m++) a.out[8 * (size_t)k + m] = out[m];
    a.flags[k] = flag;
}

// =============================================================================================
// c. triangulation of a disparity field
// =============================================================================================
constexpr int kMaxTriangulateIterations = 16;

struct TriangulateArgs {
    const float *disparity;
    const int *flags_in;
    int stride, n_rows, n_cols, win, step, iterations;
    photon_piv_plane_t plane;
    photon_piv_camera_t cam[2];
    double *out;
    int *flags;
};

// (x, y) of the camera at the world point P: the 19 terms of section 19 in their order, each coordinate summed from 0.0
__device__ __forceinline__ void image_point(const photon_piv_camera_t &c, const double P[3], double x[2]) {
    const double X = (P[0] - c.centre[0]) / c.scale[0], Y = (P[1] - c.centre[1]) / c.scale[1], Z = (P[2] - c.centre[2]) / c.scale[2];
    const double XX = X * X, XY = X * Y, YY = Y * Y, ZZ = Z * Z;
    const double T[19] = {1.0, X, Y, Z, XX, XY, YY, X * Z, Y * Z, ZZ, XX * X, XX * Y, XY * Y, YY * Y, XX * Z, XY * Z, YY * Z, X * ZZ, Y * ZZ};
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < 19; k++) {
        sx = sx + c.cx[k] * T[k];
        sy = sy + c.cy[k] * T[k];
    }
    x[0] = sx;
    x[1] = sy;
}

// the four residuals (x1 - M1(W), x2 - M2(W)) of section 19c
__device__ __forceinline__ void residuals(const TriangulateArgs &a, const double x1[2], const double x2[2], const double W[3], double r[4]) {
    double m[2];
    image_point(a.cam[0], W, m);
    r[0] = x1[0] - m[0];
    r[1] = x1[1] - m[1];
    image_point(a.cam[1], W, m);
    r[2] = x2[0] - m[0];
    r[3] = x2[1] - m[1];
}

__global__ __launch_bounds__(kNodeThreads) void triangulate_kernel(const TriangulateArgs a) {
    const int k = blockIdx.x * kNodeThreads + threadIdx.x;
    if (k >= a.n_rows * a.n_cols) return;
    const int i = k / a.n_cols, j = k - i * a.n_cols;
    const double qnan = __builtin_nan(""), pitch = a.plane.pitch;
    double P[3];
    node_point(a.plane, a.win, a.step, i, j, P);
    const float *d = a.disparity + (size_t)k * a.stride;
    const float dx = d[0], dy = d[1];
    const bool finite = isfinite(dx) && isfinite(dy);
    int flag = a.flags_in ? a.flags_in[k] : 0;

    const double hx = (pitch / 2.0) * (double)dx, hy = (pitch / 2.0) * (double)dy;
    const double P1[3] = {P[0] - hx, P[1] - hy, P[2]}, P2[3] = {P[0] + hx, P[1] + hy, P[2]};
    double x1[2], x2[2];
    image_point(a.cam[0], P1, x1);
    image_point(a.cam[1], P2, x2);

    double W[3] = {P[0], P[1], P[2]}, s[3] = {qnan, qnan, qnan}, r[4], lowest = qnan;
    bool good = true;
    for (int it = 0; it < a.iterations; it++) {
        // one camera at a time, in a loop that stays a loop (the camera is read from the kernel arguments at a uniform offset):
        // the 44 coefficients of one camera fit the scalar registers, those of two do not.  Rows 2c,
        // 2c + 1 enter N and g in the order of section 19b's sums: (row 0 + row 1), + row 2, + row 3
        double N[3][3], g[3];
#pragma unroll 1
        for (int c = 0; c < 2; c++) {
            const photon_piv_camera_t &cam = a.cam[c];
            double m[2], J[2][3];
            image_point(cam, W, m);
            const double r0 = (c == 0 ? x1[0] : x2[0]) - m[0], r1 = (c == 0 ? x1[1] : x2[1]) - m[1];
            jacobian(cam, W, J);
#pragma unroll
            for (int p = 0; p < 3; p++) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const double u = J[0][p] * J[0][q], v = J[1][p] * J[1][q];
                    N[p][q] = c == 0 ? u + v : (N[p][q] + u) + v;
                }
                const double u = J[0][p] * r0, v = J[1][p] * r1;
                g[p] = c == 0 ? u + v : (g[p] + u) + v;
            }
        }
        Cholesky3 L;
        bool ok;
        const double ratio = L.factor(N, ok);
        lowest = (ok && it > 0) ? (ratio < lowest ? ratio : lowest) : ratio;
        if (!ok) good = false;
        if (!ok || !finite) break;          // a vector that is not finite: the start point's ratio, no step
        L.solve(g, s);
        W[0] = W[0] + s[0];
        W[1] = W[1] + s[1];
        W[2] = W[2] + s[2];
    }
    double out[6] = {qnan, qnan, qnan, qnan, qnan, lowest};
    if (good && finite) {
        residuals(a, x1, x2, W, r);
        double ss = 0.0;
#pragma unroll
        for (int m = 0; m < 4; m++) ss = ss + r[m] * r[m];
        out[0] = W[0];
        out[1] = W[1];
        out[2] = W[2];
        out[3] = sqrt(ss);
        out[4] = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    }
    if (!good) flag |= 64;
    if (!finite) flag |= 128;
#pragma unroll
    for (int m = 0; m < 6; m++) a.out[6 * (size_t)k + m] = out[m];
    a.flags[k] = flag;
}

}  // namespace

extern "C" int photon_piv_dewarp(const photon_piv_dewarp_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_dewarp: null job\n");
        return 1;
    }
    const char *bad = piv_grid::side_error(job->width, job->height);
    if (!bad) bad = piv_grid::side_error(job->out_width, job->out_height);
    if (!bad) {
        if (!job->d_coef || !job->d_out) bad = "null d_coef or d_out";
        else if (job->d_coef == job->d_out) bad = "d_out must not be d_coef";
        else if (job->n_frames < 1) bad = "n_frames must be >= 1";
        else if (job->frame_stride < (long long)job->width * job->height) bad = "frame_stride is below width height";
        else if (job->out_stride < (long long)job->out_width * job->out_height) bad = "out_stride is below out_width out_height";
        else if (!all_finite(&job->poly[0][0], 20) || !all_finite(job->grid, 4)) bad = "a poly or grid value is not finite";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_dewarp: %s (%d frames %d x %d, stride %lld, to %d x %d, stride %lld)\n", bad, job->n_frames, job->width,
                job->height, job->frame_stride, job->out_width, job->out_height, job->out_stride);
        return 1;
    }
    DewarpArgs a;
    a.coef = job->d_coef;
    a.in_stride = job->frame_stride, a.out_stride = job->out_stride;
    a.n_frames = job->n_frames, a.W = job->width, a.H = job->height, a.OW = job->out_width, a.OH = job->out_height;
    for (int k = 0; k < 10; k++) a.poly[0][k] = job->poly[0][k], a.poly[1][k] = job->poly[1][k];
    for (int k = 0; k < 4; k++) a.grid[k] = job->grid[k];
    a.out = job->d_out, a.mask = job->d_mask;
    hipLaunchKernelGGL(dewarp_kernel, warp_grid(a.OW, a.OH), dim3(kWarpX, kWarpY), 0, (hipStream_t)job->stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_stereo_reconstruct(const photon_piv_stereo_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_stereo_reconstruct: null job\n");
        return 1;
    }
    const photon_piv_plane_t &pl = job->plane;
    const char *bad = piv_grid::grid_error(pl.width, pl.height, job->win, job->step);
    if (!bad && job->d_out) bad = piv_grid::grid_error(pl.width, pl.height, job->win, job->step, job->n_rows, job->n_cols);
    if (!bad && job->d_out) {
        if (!job->d_field1 || !job->d_field2 || !job->d_flags) bad = "null d_field1, d_field2 or d_flags";
        else if (job->field_stride != 2 && job->field_stride != 4) bad = "field_stride must be 2 or 4";
        else if (!job->d_sigma1 != !job->d_sigma2) bad = "d_sigma1 and d_sigma2 come together or not at all";
    }
    if (!bad) bad = plane_cameras_error(pl, job->camera1, job->camera2);
    if (bad) {
        fprintf(stderr, "photon: photon_piv_stereo_reconstruct: %s (win %d, step %d, %d x %d plane, %d x %d grid, stride %d)\n", bad, job->win,
                job->step, pl.width, pl.height, job->n_rows, job->n_cols, job->field_stride);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_stereo_reconstruct", pl.width, pl.height, job->win, job->step, rows, cols, job->rows_out, job->cols_out));
    if (!job->d_out) return 0;                  // the size query
    StereoArgs a;
    a.field1 = job->d_field1, a.field2 = job->d_field2, a.sigma1 = job->d_sigma1, a.sigma2 = job->d_sigma2;
    a.flags1 = job->d_flags1, a.flags2 = job->d_flags2;
    a.stride = job->field_stride, a.n_rows = rows, a.n_cols = cols, a.win = job->win, a.step = job->step;
    a.plane = pl, a.cam[0] = job->camera1, a.cam[1] = job->camera2;
    a.out = job->d_out, a.flags = job->d_flags;
    const unsigned blocks = (unsigned)(((long long)rows * cols + kNodeThreads - 1) / kNodeThreads);
    hipLaunchKernelGGL(reconstruct_kernel, dim3(blocks), dim3(kNodeThreads), 0, (hipStream_t)job->stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_stereo_triangulate(const photon_piv_triangulate_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_stereo_triangulate: null job\n");
        return 1;
    }
    const photon_piv_plane_t &pl = job->plane;
    const char *bad = piv_grid::grid_error(pl.width, pl.height, job->win, job->step);
    if (!bad && job->d_out) bad = piv_grid::grid_error(pl.width, pl.height, job->win, job->step, job->n_rows, job->n_cols);
    if (!bad && job->d_out) {
        if (!job->d_disparity || !job->d_flags) bad = "null d_disparity or d_flags";
        else if (job->field_stride != 2 && job->field_stride != 4) bad = "field_stride must be 2 or 4";
    }
    if (!bad && (job->iterations < 1 || job->iterations > kMaxTriangulateIterations)) bad = "iterations must be within [1, 16]";
    if (!bad) bad = plane_cameras_error(pl, job->camera1, job->camera2);
    if (bad) {
        fprintf(stderr, "photon: photon_piv_stereo_triangulate: %s (win %d, step %d, %d x %d plane, %d x %d grid, stride %d, %d iterations)\n", bad,
                job->win, job->step, pl.width, pl.height, job->n_rows, job->n_cols, job->field_stride, job->iterations);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_stereo_triangulate", pl.width, pl.height, job->win, job->step, rows, cols, job->rows_out, job->cols_out));
    if (!job->d_out) return 0;                  // the size query
    TriangulateArgs a;
    a.disparity = job->d_disparity, a.flags_in = job->d_flags_in;
    a.stride = job->field_stride, a.n_rows = rows, a.n_cols = cols, a.win = job->win, a.step = job->step, a.iterations = job->iterations;
    a.plane = pl, a.cam[0] = job->camera1, a.cam[1] = job->camera2;
    a.out = job->d_out, a.flags = job->d_flags;
    const unsigned blocks = (unsigned)(((long long)rows * cols + kNodeThreads - 1) / kNodeThreads);
    hipLaunchKernelGGL(triangulate_kernel, dim3(blocks), dim3(kNodeThreads), 0, (hipStream_t)job->stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}
