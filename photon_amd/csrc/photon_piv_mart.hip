// photon_piv_mart.hip - MART particle volumes for tomographic PIV: the exact re-projection of a volume onto its cameras and
// the multiplicative, camera-sequential update that starts from a line-of-sight volume.  Definition:
// include/parallel_ray_tracing.h, section 21; host models: photon_amd/piv_mart.py.
//
//   mart_kernel<UPDATE>   one thread per voxel in los_kernel's shape (piv_camera.hpp, VoxelGrid: a 64 x 4 block over (j, i),
//                         the slice in the block index: a wave's voxels land on neighbouring pixels).  Voxels that are not
//                         above 0 leave before any coordinate is computed: the algorithm's sparsity.  UPDATE: the footprint on
//                         the update's camera, the frame and the re-projection gathered there, the ratio, its roots, the
//                         threshold, the store.  Then, for each camera of the projection list, the footprint there and four
//                         64-bit integer atomic adds of the voxel's new value: camera c's update and camera c + 1's
//                         projection are one pass, because a voxel's new value is final when the voxel scatters it.
//                         Footprints serve up to kFrameChunk frames at once.
//   image_kernel          the accumulators as f32 images (section 21a's optional output).
// The accumulators are 64-bit integers: integer addition is associative, so any arrival order of the atomics returns the same
// integers, two calls return the same bits, and the fused pass equals the two-step definition bit for bit.
// Neither entry point allocates: the accumulators are the caller's.  Footprint, voxel shape, shared rules: piv_camera.hpp.
#include <climits>
#include <cmath>

#include "photon_internal.hpp"
#include "piv_camera.hpp"
#include "piv_grid.hpp"
#include "piv_warp.hpp"

using namespace photon;

namespace {

using namespace piv_camera;
using piv_warp::kWarpX;
using piv_warp::kWarpY;

constexpr int kMaxRoots = 3;
constexpr int kScaleMin = -126, kScaleMax = 62;
#ifdef PHOTON_MART_UNFUSED
constexpr bool kFused = false;      // A/B: an update launch and a projection launch per camera step (the same bits)
#else
constexpr bool kFused = true;
#endif

struct View {
    int W, H, camera;               // the sensor; the camera's index into poly
    double grid[4];
    unsigned long long *acc;        // [n_frames] accumulators, acc_stride apart
    long long acc_stride;
};

struct MartArgs {
    float *vol;                     // [n_frames] volumes, vol_stride apart (read only without UPDATE)
    long long vol_stride;
    const unsigned char *mask;
    const double *poly;             // [n_cameras][nz][2][10]
    int n_frames;
    VoxelGrid vox;
    double scale, inv_scale;        // 2^s, 2^-s
    View upd;                       // UPDATE: the camera of the update; acc holds its re-projection
    const float *frames;            // its raw frames, frame_stride apart
    long long frame_stride;
    int roots;
    float threshold;
    int n_proj;
    View proj[kMaxCameras];         // the cameras the voxels are scattered to
};

// one contribution in fixed point: llrint(min(f64(p) 2^s, 2^31)); what is not above 0, a NaN included, is 0
__device__ __forceinline__ unsigned long long quantise(float p, double scale) {
    const double t = (double)p * scale;
    return t >= 2147483648.0 ? 2147483648ull : t > 0.0 ? (unsigned long long)llrint(t) : 0ull;
}

template <bool UPDATE>
__global__ __launch_bounds__(kWarpX *kWarpY) void mart_kernel(const MartArgs a) {
    int i, j, k;
    size_t o;
    if (!a.vox.voxel(i, j, k, o)) return;
    for (int f0 = 0; f0 < a.n_frames; f0 += kFrameChunk) {
        const int nf = min(kFrameChunk, a.n_frames - f0);
        float E[kFrameChunk] = {0.f, 0.f, 0.f, 0.f};
        bool live = false;
#pragma unroll
        for (int f = 0; f < kFrameChunk; f++)
            if (f < nf) {
                E[f] = a.vol[(size_t)(f0 + f) * a.vol_stride + o];
                live = live || E[f] > 0.f;
            }
        if (!live) continue;            // zeros, negatives and NaN: no coordinate, no store, no add
        Footprint fp;
        if (UPDATE) {
            const View &u = a.upd;
            const bool seen = !(a.mask && a.mask[o]) && footprint(a.poly + ((size_t)u.camera * a.vox.nz + k) * 20, u.grid, i, j, u.W, u.H, fp);
#pragma unroll
            for (int f = 0; f < kFrameChunk; f++) {
                if (f >= nf || !(E[f] > 0.f)) continue;
                float e = 0.f;
                if (seen) {
                    const float *img = a.frames + (size_t)(f0 + f) * a.frame_stride;
                    const long long *acc = reinterpret_cast<const long long *>(u.acc) + (size_t)(f0 + f) * u.acc_stride;
                    float I[4], P[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const size_t p = fp.pixel(t);
                        const float v = img[p];
                        I[t] = v > 0.f ? v : 0.f;
                        P[t] = (float)((double)acc[p] * a.inv_scale);
                    }
                    const float i_bar = ((fp.w[0] * I[0] + fp.w[1] * I[1]) + fp.w[2] * I[2]) + fp.w[3] * I[3];
                    const float p_bar = ((fp.w[0] * P[0] + fp.w[1] * P[1]) + fp.w[2] * P[2]) + fp.w[3] * P[3];
                    e = E[f];
                    if (p_bar > 0.f) {
                        float r = i_bar / p_bar;
                        for (int m = 0; m < a.roots; m++) r = sqrtf(r);
                        e = e * r;
                    }
                    if (e < a.threshold) e = 0.f;
                }
                E[f] = e;
                a.vol[(size_t)(f0 + f) * a.vol_stride + o] = e;
            }
        }
#pragma unroll 1
        for (int c = 0; c < a.n_proj; c++) {
            const View &v = a.proj[c];
            if (!footprint(a.poly + ((size_t)v.camera * a.vox.nz + k) * 20, v.grid, i, j, v.W, v.H, fp)) continue;
#pragma unroll
            for (int f = 0; f < kFrameChunk; f++) {
                if (f >= nf || !(E[f] > 0.f)) continue;
                unsigned long long *acc = v.acc + (size_t)(f0 + f) * v.acc_stride;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const unsigned long long q = quantise(fp.w[t] * E[f], a.scale);
                    if (q) atomicAdd(acc + fp.pixel(t), q);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void image_kernel(const long long *acc, float *image, long long stride, long long n_pixels, double inv_scale) {
    const long long *src = acc + (size_t)blockIdx.y * stride;
    float *dst = image + (size_t)blockIdx.y * stride;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (long long)gridDim.x * 256)
        dst[p] = (float)((double)src[p] * inv_scale);
}

template <bool UPDATE>
int launch(const MartArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(mart_kernel<UPDATE>, dim3(a.vox.blocks()), dim3(kWarpX, kWarpY), 0, stream, a);
    PH_CHECK(hipGetLastError());
    return 0;
}

// what sections 21a and 21b share of section 20a's rules (piv_camera.hpp): counts, scale, volume, sensors, grids, in this order
const char *common_error(int n_cameras, int n_frames, int scale_log2, const photon_piv_volume_t &vol, long long vol_stride, const int *width,
                         const int *height, const double (*grid)[4]) {
    const char *bad = cameras_error(n_cameras);
    if (!bad) bad = frames_error(n_frames);
    if (!bad && (scale_log2 < kScaleMin || scale_log2 > kScaleMax)) bad = "scale_log2 must be within [-126, 62]";
    if (!bad) bad = volume_error(vol, vol_stride, "vol_stride is below nx ny nz");
    for (int c = 0; !bad && c < n_cameras; c++) {
        bad = piv_grid::side_error(width[c], height[c]);
        if (!bad) bad = grid_values_error(grid[c]);
    }
    return bad;
}

void fill_common(MartArgs &a, const photon_piv_volume_t &vol, const float *d_vol, long long vol_stride, const double *d_poly, int n_frames, int scale_log2) {
    a.vol = const_cast<float *>(d_vol), a.vol_stride = vol_stride;
    a.mask = nullptr, a.poly = d_poly;
    a.n_frames = n_frames, a.vox = VoxelGrid::make(vol);
    a.scale = std::ldexp(1.0, scale_log2), a.inv_scale = std::ldexp(1.0, -scale_log2);
    a.upd = View{}, a.frames = nullptr, a.frame_stride = 0, a.roots = 0, a.threshold = 0.f, a.n_proj = 0;
    for (int c = 0; c < kMaxCameras; c++) a.proj[c] = View{};
}

View view_of(int c, const int *width, const int *height, const double (*grid)[4], void *acc, long long acc_stride) {
    View v;
    v.W = width[c], v.H = height[c], v.camera = c;
    for (int m = 0; m < 4; m++) v.grid[m] = grid[c][m];
    v.acc = reinterpret_cast<unsigned long long *>(acc), v.acc_stride = acc_stride;
    return v;
}

}  // namespace

extern "C" int photon_piv_volume_project(const photon_piv_volume_project_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_volume_project: null job\n");
        return 1;
    }
    const photon_piv_volume_t &vol = job->volume;
    const char *bad = nullptr;
    if (!job->d_poly || !job->d_vol) bad = "null d_poly or d_vol";
    if (!bad) bad = common_error(job->n_cameras, job->n_frames, job->scale_log2, vol, job->vol_stride, job->width, job->height, job->grid);
    Range ranges[1 + 2 * kMaxCameras];
    int n_ranges = 0;
    if (!bad) ranges[n_ranges++] = range_of(job->d_vol, 4, job->vol_stride, job->n_frames);
    for (int c = 0; !bad && c < job->n_cameras; c++) {
        if (!job->d_acc[c]) bad = "a null d_acc";
        else if (job->acc_stride[c] < (long long)job->width[c] * job->height[c]) bad = "an acc_stride is below width height";
        else {
            ranges[n_ranges++] = range_of(job->d_acc[c], 8, job->acc_stride[c], job->n_frames);
            if (job->d_image[c]) ranges[n_ranges++] = range_of(job->d_image[c], 4, job->acc_stride[c], job->n_frames);
        }
    }
    for (int p = 0; !bad && p < n_ranges; p++)
        for (int q = p + 1; q < n_ranges; q++)
            if (overlap(ranges[p], ranges[q])) bad = "the accumulators and images must not overlap each other or the volume";
    if (bad) {
        fprintf(stderr, "photon: photon_piv_volume_project: %s (%d cameras, %d frames, scale_log2 %d, volume %d x %d x %d, stride %lld)\n", bad,
                job->n_cameras, job->n_frames, job->scale_log2, vol.nx, vol.ny, vol.nz, job->vol_stride);
        return 1;
    }
    hipStream_t stream = (hipStream_t)job->stream;
    MartArgs a;
    fill_common(a, vol, job->d_vol, job->vol_stride, job->d_poly, job->n_frames, job->scale_log2);
    a.n_proj = job->n_cameras;
    for (int c = 0; c < job->n_cameras; c++) {
        a.proj[c] = view_of(c, job->width, job->height, job->grid, job->d_acc[c], job->acc_stride[c]);
        const size_t frame_bytes = 8 * (size_t)job->width[c] * job->height[c];
        if (job->acc_stride[c] == (long long)job->width[c] * job->height[c]) {
            PH_CHECK(hipMemsetAsync(job->d_acc[c], 0, frame_bytes * job->n_frames, stream));
        } else {                        // the gaps of a longer stride are not touched
            for (int f = 0; f < job->n_frames; f++) PH_CHECK(hipMemsetAsync(job->d_acc[c] + (size_t)f * job->acc_stride[c], 0, frame_bytes, stream));
        }
    }
    PH_TRY(launch<false>(a, stream));
    for (int c = 0; c < job->n_cameras; c++) {
        if (!job->d_image[c]) continue;
        const long long n_pixels = (long long)job->width[c] * job->height[c];
        const unsigned blocks = (unsigned)std::min<long long>((n_pixels + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(image_kernel, dim3(blocks, (unsigned)job->n_frames), dim3(256), 0, stream, job->d_acc[c], job->d_image[c], job->acc_stride[c],
                           n_pixels, a.inv_scale);
        PH_CHECK(hipGetLastError());
    }
    return 0;
}

extern "C" int photon_piv_volume_mart(const photon_piv_volume_mart_t *job) {
    if (!job) {
        fprintf(stderr, "photon: photon_piv_volume_mart: null job\n");
        return 1;
    }
    const photon_piv_volume_t &vol = job->volume;
    const char *bad = nullptr;
    if (!job->d_poly || !job->d_vol || !job->d_acc) bad = "null d_poly, d_vol or d_acc";
    else if (job->iterations < 1) bad = "iterations must be >= 1";
    else if (job->mu_roots < 0 || job->mu_roots > kMaxRoots) bad = "mu_roots must be within [0, 3]";
    else if (!(std::isfinite(job->threshold) && job->threshold >= 0.f)) bad = "threshold must be finite and >= 0";
    if (!bad) bad = common_error(job->n_cameras, job->n_frames, job->scale_log2, vol, job->vol_stride, job->width, job->height, job->grid);
    long long max_pixels = 0;
    for (int c = 0; !bad && c < job->n_cameras; c++) max_pixels = std::max(max_pixels, (long long)job->width[c] * job->height[c]);
    if (!bad) {
        const Range volume = range_of(job->d_vol, 4, job->vol_stride, job->n_frames), acc = range_of(job->d_acc, 8, 2 * max_pixels, job->n_frames);
        const Range mask = range_of(job->d_mask, 1, (long long)vol.nx * vol.ny * vol.nz, job->d_mask ? 1 : 0);
        if (overlap(volume, acc) || overlap(mask, acc) || overlap(mask, volume)) bad = "d_vol, d_acc and d_mask must not overlap";
        for (int c = 0; !bad && c < job->n_cameras; c++) {
            const Range frames = range_of(job->d_frame[c], 4, job->frame_stride[c], job->n_frames);
            if (!job->d_frame[c]) bad = "a null d_frame";
            else if (job->frame_stride[c] < (long long)job->width[c] * job->height[c]) bad = "a frame_stride is below width height";
            else if (overlap(frames, volume) || overlap(frames, acc)) bad = "d_vol and d_acc must not overlap a d_frame";
        }
    }
    if (bad) {
        fprintf(stderr, "photon: photon_piv_volume_mart: %s (%d cameras, %d frames, %d iterations, mu_roots %d, threshold %g, scale_log2 %d, volume %d x %d x %d, stride %lld)\n",
                bad, job->n_cameras, job->n_frames, job->iterations, job->mu_roots, (double)job->threshold, job->scale_log2, vol.nx, vol.ny, vol.nz,
                job->vol_stride);
        return 1;
    }
    hipStream_t stream = (hipStream_t)job->stream;
    MartArgs a;
    fill_common(a, vol, job->d_vol, job->vol_stride, job->d_poly, job->n_frames, job->scale_log2);
    a.mask = job->d_mask, a.roots = job->mu_roots, a.threshold = job->threshold;
    // two buffers of [n_frames][max_pixels]: a step reads the one its predecessor filled and fills the other
    const size_t half = (size_t)job->n_frames * (size_t)max_pixels, half_bytes = 8 * half;
    long long *buffer[2] = {job->d_acc, job->d_acc + half};
    const int N = job->n_cameras;
    const long long steps = (long long)job->iterations * N;
    MartArgs first = a;                 // the re-projection of the first guess on camera 0
    first.n_proj = 1, first.proj[0] = view_of(0, job->width, job->height, job->grid, buffer[0], max_pixels);
    PH_CHECK(hipMemsetAsync(buffer[0], 0, half_bytes, stream));
    PH_TRY(launch<false>(first, stream));
    for (long long t = 0; t < steps; t++) {
        const int c = (int)(t % N), next = t + 1 < steps ? (int)((t + 1) % N) : -1;
        MartArgs step = a;
        step.upd = view_of(c, job->width, job->height, job->grid, buffer[t & 1], max_pixels);
        step.frames = job->d_frame[c], step.frame_stride = job->frame_stride[c];
        if (next >= 0) PH_CHECK(hipMemsetAsync(buffer[(t + 1) & 1], 0, half_bytes, stream));
        if (kFused) {
            if (next >= 0) step.n_proj = 1, step.proj[0] = view_of(next, job->width, job->height, job->grid, buffer[(t + 1) & 1], max_pixels);
            PH_TRY(launch<true>(step, stream));
        } else {
            PH_TRY(launch<true>(step, stream));
            if (next >= 0) {
                MartArgs project = a;
                project.n_proj = 1, project.proj[0] = view_of(next, job->width, job->height, job->grid, buffer[(t + 1) & 1], max_pixels);
                PH_TRY(launch<false>(project, stream));
            }
        }
    }
    return 0;
}
