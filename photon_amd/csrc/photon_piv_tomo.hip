// photon_piv_tomo.hip - tomographic PIV beside the planar and stereo correlators: a particle volume built from the frames of
// N cameras by line of sight, and the windowed direct correlation of two volumes with three-dimensional windows and a
// three-dimensional search region.  Definition: include/parallel_ray_tracing.h, section 20; host models: photon_amd/piv_tomo.py.
//
//   los_kernel                one thread per voxel (piv_camera.hpp, VoxelGrid): per camera the dewarp of section 19a at the
//                             voxel's slice -- dewarp_kernel's own sensor_point (piv_camera.hpp) and BsplineTaps
//                             (piv_warp.hpp) --, the samples clamped at 0 and combined over the cameras in camera order
//                             (minimum or product); a camera's taps serve up to kFrameChunk frames at once
//   correlate_volume_kernel   one workgroup per window under section 5's plan (piv_direct.hpp).  A 3-D correlation at one
//                             z-shift is the ensemble correlation of the window's z-planes taken with whole-window means:
//                             per z-shift the win_z plane pairs are staged as photon_piv.hip stages a pair, correlate_tiles
//                             adds them into slice 0 as section 14 does, and the raw plane goes to d_planes, the kernel's
//                             workspace; the tail reads it back behind a barrier and normalises it in place.
// Neither kernel needs device scratch; every sum has a fixed order: two calls return the same bits.
#include <cfloat>
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_camera.hpp"
#include "piv_direct.hpp"
#include "piv_grid.hpp"
#include "piv_peak.hpp"
#include "piv_warp.hpp"

using namespace photon;

namespace {

using namespace piv_camera;
using namespace piv_direct;
using namespace piv_warp;

// =============================================================================================
// a. line-of-sight volume
// =============================================================================================
struct LosArgs {
    const float *coef[kMaxCameras];
    long long in_stride[kMaxCameras];
    int W[kMaxCameras], H[kMaxCameras];
    double grid[kMaxCameras][4];
    const double *poly;             // [n_cameras][nz][2][10]
    int n_cameras, n_frames, mode;
    VoxelGrid vox;
    long long out_stride;
    float *out;
    unsigned char *mask;
};

__global__ __launch_bounds__(kWarpX *kWarpY) void los_kernel(const LosArgs a) {
    int i, j, k;
    size_t o;
    if (!a.vox.voxel(i, j, k, o)) return;
    for (int f0 = 0; f0 < a.n_frames; f0 += kFrameChunk) {
        const int nf = min(kFrameChunk, a.n_frames - f0);
        float acc[kFrameChunk] = {0.f, 0.f, 0.f, 0.f};
        bool inside = true;
#pragma unroll 1
        for (int c = 0; c < a.n_cameras; c++) {
            const int W = a.W[c], H = a.H[c];
            SensorPoint p;
            if (!sensor_point(a.poly + ((size_t)c * a.vox.nz + k) * 20, a.grid[c], i, j, W, H, p)) {
                inside = false;
                break;
            }
            const BsplineTaps taps(p.ix, p.iy, p.fx, p.fy, W, H);
#pragma unroll
            for (int f = 0; f < kFrameChunk; f++) {
                if (f >= nf) break;
                const float s_c = taps.sample(a.coef[c] + (size_t)(f0 + f) * a.in_stride[c]);
                const float val = s_c > 0.f ? s_c : 0.f;
                acc[f] = c == 0 ? val : a.mode == 0 ? (val < acc[f] ? val : acc[f]) : acc[f] * val;
            }
        }
        if (!inside) {              // the geometry decides: found in the first chunk, for every frame
            if (a.mask) a.mask[o] = 1;
            for (int f = 0; f < a.n_frames; f++) a.out[(size_t)f * a.out_stride + o] = 0.f;
            return;
        }
        if (f0 == 0 && a.mask) a.mask[o] = 0;
#pragma unroll
        for (int f = 0; f < kFrameChunk; f++)
            if (f < nf) a.out[(size_t)(f0 + f) * a.out_stride + o] = acc[f];
    }
}

// =============================================================================================
// b. 3-D windowed direct correlation
// =============================================================================================
constexpr int kMaxWinZ = 64, kMaxRadiusZ = 16;

struct CorrelateArgs {
    const float *vol1, *vol2;
    int nx, ny, nz, step, R, win_z, step_z, Rz, n_rows, n_cols;
    const int *offset;
    int K, nSxp, nSyp;
    float *vectors;
    int *flags;
    float *planes;
};

// a flat window (block-uniform): NaN vector, NaN planes, flag 2
__device__ __forceinline__ void write_flat_volume(int win_id, int nS3, bool outside, float *vectors, int *flags, float *planes) {
    const float qnan = __builtin_nanf("");
    if (threadIdx.x == 0) {
#pragma unroll
        for (int m = 0; m < 5; m++) vectors[5 * (size_t)win_id + m] = qnan;
        flags[win_id] = 2 | (outside ? 4 : 0);
    }
    for (int i = threadIdx.x; i < nS3; i += blockDim.x) planes[(size_t)win_id * nS3 + i] = qnan;
}

// LDS layout (floats): photon_piv.hip's -- a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | K partial planes | scratch.
template <int WIN>
__global__ __launch_bounds__(kMaxThreads, 4) void correlate_volume_kernel(const CorrelateArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int R = a.R, Rz = a.Rz, K = a.K, nSxp = a.nSxp, nSyp = a.nSyp;
    const int nS = 2 * R + 1, nS2 = nS * nS, nSz = 2 * Rz + 1, nS3 = nSz * nS2;
    const int pitch = WIN + nSxp, rows = WIN + nSyp - 1, P = nSyp * nSxp;
    float *sa = lds;
    float *sb = sa + WIN * WIN;
    float *sp = sb + rows * pitch;
    float *red = sp + K * P;
    int *redi = reinterpret_cast<int *>(red + 32);

    const int W = a.nx, H = a.ny, D = a.nz, win_z = a.win_z;
    const size_t slice = (size_t)W * H;
    const int win_id = blockIdx.x, per_slab = a.n_rows * a.n_cols;
    const int in_slab = win_id % per_slab;
    const int wz0 = (win_id / per_slab) * a.step_z, wy0 = (in_slab / a.n_cols) * a.step, wx0 = (in_slab % a.n_cols) * a.step;
    const int ox = a.offset ? a.offset[3 * (size_t)win_id] : 0, oy = a.offset ? a.offset[3 * (size_t)win_id + 1] : 0;
    const int oz = a.offset && D > 1 ? a.offset[3 * (size_t)win_id + 2] : 0;         // one slice: there is no z to offset
    const int tid = threadIdx.x, B = blockDim.x, n_waves = B >> 6;
    const int span = WIN + 2 * R;
    const bool outside = wy0 + oy - R < 0 || wx0 + ox - R < 0 || wy0 + oy + WIN - 1 + R >= H || wx0 + ox + WIN - 1 + R >= W ||
                         wz0 + oz - Rz < 0 || wz0 + oz + win_z - 1 + Rz >= D;
    float *plane_out = a.planes + (size_t)win_id * nS3;

    // ---- the means over the whole window, plane after plane in photon_piv.hip's lane order, and the exact flatness counts
    const float ref_a = a.vol1[(size_t)wz0 * slice + (size_t)wy0 * W + wx0];
    const float ref_b = a.vol2[(size_t)min(max(wz0 + oz, 0), D - 1) * slice + (size_t)min(max(wy0 + oy, 0), H - 1) * W + min(max(wx0 + ox, 0), W - 1)];
    float sum_a = 0.f, sum_b = 0.f, cnt_b = 0.f, dif_a = 0.f, dif_b = 0.f;
    for (int pz = 0; pz < win_z; pz++) {
        const float *p1 = a.vol1 + (size_t)(wz0 + pz) * slice;
        const int gz = wz0 + oz + pz;
        const bool z_in = gz >= 0 && gz < D;
        const float *p2 = a.vol2 + (size_t)(z_in ? gz : 0) * slice;
        for (int i = tid; i < WIN * WIN; i += B) {
            const int y = i / WIN, x = i % WIN;
            const float v = p1[(size_t)(wy0 + y) * W + (wx0 + x)];
            sum_a += v;
            dif_a += v != ref_a ? 1.f : 0.f;
            const int gy = wy0 + oy + y, gx = wx0 + ox + x;
            if (z_in && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float u = p2[(size_t)gy * W + gx];
                sum_b += u;
                cnt_b += 1.f;
                dif_b += u != ref_b ? 1.f : 0.f;
            }
        }
    }
    float tot[5] = {sum_a, sum_b, cnt_b, dif_a, dif_b};
    block_reduce(tot, red, n_waves, Sum());         // counts up to 64 * 64^2 = 2^18 are exact in f32
    const float cnt = tot[2];
    const float mean_a = tot[0] / (float)(win_z * WIN * WIN);
    const float mean_b = cnt > 0.f ? tot[1] / cnt : 0.f;
    if (tot[3] == 0.f || tot[4] == 0.f) {           // all voxels of a equal, or all (or none) of b at zero shift: block-uniform
        write_flat_volume(win_id, nS3, outside, a.vectors, a.flags, a.planes);
        return;
    }

    // ---- per z-shift (the zero shift first: it carries the energies) the window's plane pairs, each staged and correlated
    //      as photon_piv_ensemble.hip does a pair: slice 0 takes the running total along
    float Ea = 0.f, Eb = 0.f;
    for (int it = 0; it < nSz; it++) {
        const int sz = it == 0 ? Rz : it <= Rz ? it - 1 : it;
        for (int pz = 0; pz < win_z; pz++) {
            const float *p1 = a.vol1 + (size_t)(wz0 + pz) * slice;
            const int gz = wz0 + oz + pz + sz - Rz;
            const bool z_in = gz >= 0 && gz < D;                // a plane of vol2 outside the volume: all zeros
            const float *p2 = a.vol2 + (size_t)(z_in ? gz : 0) * slice;
            float e[2] = {0.f, 0.f};
            for (int i = tid; i < WIN * WIN; i += B) {
                const int y = i / WIN, x = i % WIN;
                const float v = p1[(size_t)(wy0 + y) * W + (wx0 + x)] - mean_a;
                sa[i] = v;
                e[0] = fmaf(v, v, e[0]);
            }
            for (int i = tid; i < rows * pitch; i += B) {
                const int ry = i / pitch, rx = i % pitch;
                float v = 0.f;
                if (ry < span && rx < span) {
                    const int gy = wy0 + oy - R + ry, gx = wx0 + ox - R + rx;
                    if (z_in && gy >= 0 && gy < H && gx >= 0 && gx < W) v = p2[(size_t)gy * W + gx] - mean_b;
                    if (ry >= R && ry < R + WIN && rx >= R && rx < R + WIN) e[1] = fmaf(v, v, e[1]);
                }
                sb[i] = v;
            }
            if (it == 0) {                                      // the energies, in plane order (the barriers also publish sa and sb)
                block_reduce(e, red, n_waves, Sum());
                Ea = pz == 0 ? e[0] : Ea + e[0];
                Eb = pz == 0 ? e[1] : Eb + e[1];
            } else {
                __syncthreads();
            }
            correlate_tiles<WIN, true>(sa, sb, sp, K, P, pitch, nSxp, nSyp, pz > 0);        // total + tile, never 0 + tile
            __syncthreads();
            // slices 1 .. K-1 into slice 0, in slice order, by the thread that owns the shift below
            if (K > 1 && pz + 1 < win_z)
                for (int i = tid; i < nS2; i += B) {
                    const int j = (i / nS) * nSxp + i % nS;
                    float c = sp[j];
                    for (int k = 1; k < K; k++) c += sp[k * P + j];
                    sp[j] = c;
                }
        }
        if (it == 0 && (!(Ea > 0.f) || !(Eb > 0.f))) {          // a contrast too small for the f32 energies: block-uniform
            write_flat_volume(win_id, nS3, outside, a.vectors, a.flags, a.planes);
            return;
        }
        for (int i = tid; i < nS2; i += B) {                    // the last pair's slices, and the raw plane to the workspace
            const int j = (i / nS) * nSxp + i % nS;
            float c = sp[j];
            for (int k = 1; k < K; k++) c += sp[k * P + j];
            plane_out[sz * nS2 + i] = c;
        }
    }
    __threadfence_block();
    __syncthreads();                    // the raw planes, for every thread of the block

    // ---- the tail: argmax in (sz, sy, sx) order, the second maximum, three fits; then the planes normalised in place
    const double inv = 1.0 / sqrt((double)Ea * (double)Eb);
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < nS3; i += B) {
        const float c = plane_out[i];
        if (better(c, i, bv, bi)) {
            bv = c;
            bi = i;
        }
    }
    block_argmax(bv, bi, red, redi);
    const int pz = bi / nS2, py = (bi % nS2) / nS, px = bi % nS;
    float m2 = -INFINITY;
    for (int i = tid; i < nS3; i += B) {
        const int sz = i / nS2, sy = (i % nS2) / nS, sx = i % nS;
        if (max(abs(sz - pz), max(abs(sy - py), abs(sx - px))) >= 2) m2 = fmaxf(m2, plane_out[i]);
    }
    m2 = block_reduce(m2, red, n_waves, MaxF32());
    if (tid == 0) {
        auto at = [&](int sz, int sy, int sx) { return (double)plane_out[(sz * nS + sy) * nS + sx]; };
        int f = outside ? 4 : 0;
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if (px == 0 || px == nS - 1) f |= 1;
        else dx = subpixel(at(pz, py, px - 1), at(pz, py, px), at(pz, py, px + 1));
        if (py == 0 || py == nS - 1) f |= 1;
        else dy = subpixel(at(pz, py - 1, px), at(pz, py, px), at(pz, py + 1, px));
        if (Rz >= 1) {                                          // without a z search dz = oz and z raises no flag
            if (pz == 0 || pz == nSz - 1) f |= 1;
            else dz = subpixel(at(pz - 1, py, px), at(pz, py, px), at(pz + 1, py, px));
        }
        float *vec = a.vectors + 5 * (size_t)win_id;
        vec[0] = (float)((double)(ox + px - R) + dx);
        vec[1] = (float)((double)(oy + py - R) + dy);
        vec[2] = (float)((double)(oz + pz - Rz) + dz);
        vec[3] = (float)((double)bv * inv);
        vec[4] = m2 > 0.f ? (float)((double)bv / (double)m2) : INFINITY;
        a.flags[win_id] = f;
    }
    __syncthreads();                    // thread 0 has read its raw values
    for (int i = tid; i < nS3; i += B) plane_out[i] = (float)((double)plane_out[i] * inv);
}

template <int WIN>
int launch(const CorrelateArgs &args, long long n_windows, hipStream_t stream) {
    int lds_limit = 0;
    PH_TRY(piv_grid::lds_limit(&lds_limit));
    const Plan p = plan_for(WIN, args.R, (size_t)lds_limit);            // section 5's plan: one slice gives its bits
    if (p.K == 0) return piv_grid::lds_refused("photon_piv_correlate_volume", WIN, "radius", args.R, lds_limit);
    PH_TRY(piv_grid::raise_lds(correlate_volume_kernel<WIN>, p.lds_bytes));
    CorrelateArgs a = args;
    a.K = p.K, a.nSxp = p.nSxp, a.nSyp = p.nSyp;
    hipLaunchKernelGGL(correlate_volume_kernel<WIN>, dim3((unsigned)n_windows), dim3(p.threads), p.lds_bytes, stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int photon_piv_volume_los(const photon_piv_volume_los_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_volume_los: null job\n");
        return 1;
    }
    const photon_piv_volume_t &vol = job->volume;
    const char *bad = cameras_error(job->n_cameras);
    if (!bad && job->mode != 0 && job->mode != 1) bad = "mode must be 0 (minimum) or 1 (product)";
    if (!bad) bad = frames_error(job->n_frames);
    if (!bad && (!job->d_poly || !job->d_out)) bad = "null d_poly or d_out";
    if (!bad) bad = volume_error(vol, job->out_stride, "out_stride is below nx ny nz");
    for (int c = 0; !bad && c < job->n_cameras; c++) {
        bad = piv_grid::side_error(job->width[c], job->height[c]);
        if (bad) break;
        if (!job->d_coef[c]) bad = "a null d_coef";
        else if (job->frame_stride[c] < (long long)job->width[c] * job->height[c]) bad = "a frame_stride is below width height";
        else if (overlap(range_of(job->d_out, 4, job->out_stride, job->n_frames), range_of(job->d_coef[c], 4, job->frame_stride[c], job->n_frames)))
            bad = "d_out must not overlap a d_coef";
        else bad = grid_values_error(job->grid[c]);
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_volume_los: %s (%d cameras, %d frames, mode %d, volume %d x %d x %d, stride %lld)\n", bad, job->n_cameras,
                job->n_frames, job->mode, vol.nx, vol.ny, vol.nz, job->out_stride);
        return 1;
    }
    LosArgs a;
    for (int c = 0; c < kMaxCameras; c++) {
        const bool used = c < job->n_cameras;
        a.coef[c] = used ? job->d_coef[c] : nullptr;
        a.in_stride[c] = used ? job->frame_stride[c] : 0;
        a.W[c] = used ? job->width[c] : 0, a.H[c] = used ? job->height[c] : 0;
        for (int m = 0; m < 4; m++) a.grid[c][m] = used ? job->grid[c][m] : 0.0;
    }
    a.poly = job->d_poly;
    a.n_cameras = job->n_cameras, a.n_frames = job->n_frames, a.mode = job->mode;
    a.vox = VoxelGrid::make(vol);
    a.out_stride = job->out_stride, a.out = job->d_out, a.mask = job->d_mask;
    hipLaunchKernelGGL(los_kernel, dim3(a.vox.blocks()), dim3(kWarpX, kWarpY), 0, (hipStream_t)job->stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int photon_piv_correlate_volume(const photon_piv_correlate_volume_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_correlate_volume: null job\n");
        return 1;
    }
    const char *bad = piv_grid::win_error(job->win);
    if (!bad && (job->radius < 1 || job->radius > job->win / 2)) bad = "radius must lie in [1, win / 2]";
    if (!bad) bad = piv_grid::side_error(job->nx, job->ny);
    if (!bad) bad = piv_grid::side_error(job->nz, job->nz);
    if (!bad) bad = piv_grid::grid_error(job->nx, job->ny, job->win, job->step);
    if (!bad) {
        if (job->win_z < 1 || job->win_z > kMaxWinZ) bad = "win_z must be within [1, 64]";
        else if (job->step_z < 1) bad = "step_z must be >= 1";
        else if (job->radius_z < 0 || job->radius_z > std::min(kMaxRadiusZ, job->win_z / 2)) bad = "radius_z must lie in [0, min(16, win_z / 2)]";
        else if (job->nz < job->win_z) bad = "the volume has fewer slices than one window";
        else if ((long long)job->nx * job->ny * job->nz > INT_MAX) bad = "nx ny nz is above INT_MAX";
        else if (!job->d_vol1 || !job->d_vol2) bad = "null volume pointer";
        else if (job->d_vectors && (!job->d_flags || !job->d_planes)) bad = "d_vectors without d_flags or d_planes";
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_correlate_volume: %s (win %d, step %d, radius %d, win_z %d, step_z %d, radius_z %d, %d x %d x %d volume)\n",
                bad, job->win, job->step, job->radius, job->win_z, job->step_z, job->radius_z, job->nx, job->ny, job->nz);
        return 1;
    }
    int rows, cols;
    PH_TRY(piv_grid::grid_size("photon_piv_correlate_volume", job->nx, job->ny, job->win, job->step, rows, cols, nullptr, nullptr));
    const int slabs = (job->nz - job->win_z) / job->step_z + 1;
    const long long n_windows = (long long)slabs * rows * cols;
    if (n_windows > INT_MAX) {
        fprintf(stderr, "photon: photon_piv_correlate_volume: %d x %d x %d windows are too many for one call\n", slabs, rows, cols);
        return 1;
    }
    if (job->n_slabs) *job->n_slabs = slabs;
    if (job->n_rows) *job->n_rows = rows;
    if (job->n_cols) *job->n_cols = cols;
    if (!job->d_vectors) return 0;              // the size query
    CorrelateArgs a;
    a.vol1 = job->d_vol1, a.vol2 = job->d_vol2;
    a.nx = job->nx, a.ny = job->ny, a.nz = job->nz, a.step = job->step, a.R = job->radius;
    a.win_z = job->win_z, a.step_z = job->step_z, a.Rz = job->radius_z, a.n_rows = rows, a.n_cols = cols;
    a.offset = job->d_offset;
    a.K = a.nSxp = a.nSyp = 0;
    a.vectors = job->d_vectors, a.flags = job->d_flags, a.planes = job->d_planes;
    hipStream_t stream = (hipStream_t)job->stream;
    return piv_grid::dispatch_win(job->win, [&](auto WIN) { return launch<WIN()>(a, n_windows, stream); });
}
