// photon_internal.hpp - what the translation units of libparallel_ray_tracing.so share on the host side: error
// handling, the handle types behind include/parallel_ray_tracing.h, and the functions one unit calls in another.
//
//   photon_pool.hip / .hpp   block cache, allocation helper, the two owners of device memory (DeviceBuffer, PoolBuffer), peer-access record
//   photon_volume.hip        NRRD parser, gradient-volume build + B-spline prefilter kernels, volume handle API, volume cache
//   photon_scene.hip         scene / source handles (their blocks are owner members: nothing is freed by hand), the workspace a scene
//                            grows on demand, on-device scene generation, the glibc rand table
//   photon_cull.hip          what a launch may leave out (dead lens samples, sources off the sensor, doomed rays), the plan of a trace
//   photon_march.hip         host side of a march launch: its plan (pieces, queue chunks, grid, kernel), the enqueue, wave-timing profile
//   photon_march_{linear,cubic,extra}.hip   the march kernels and the one plan -> kernel dispatcher (march_kernel.hpp), one unit per sampler
//   photon_sensor.hip        ray generation, sensor stage (lens / aperture / splats), finalize
//   photon_trace.hip         launch loop of a trace, photon_trace, statistics
//   photon_post.hip          sensor post-processing, the streaming-copy yardstick
//   photon_piv.hip           cross-correlation of image pairs: PIV / BOS displacement fields
//   photon_dots.hip          BOS dot tracking: per-dot shifts from an image pair
//   photon_density.hip       BOS displacement fields integrated into projected density
//   photon_tomo.hip          tomography: projector, adjoint and CG solver from several views' projected density to the 3-D field;
//                            the projector's shift derivative, its adjoint and the same solver from the views' deflections
//   photon_abi.hip           start_ray_tracing, PHOTON_DEVICES (several devices inside one call)
//   photon_sort.hip          Morton order of a range of sources
//   photon_moments.hip       per-source sensor moments: the reduction of a launch's moments block into records
//   photon_flow.hip          velocity fields on a grid, the PIV field advected through one
//   photon_piv_deform.hip    image-deformation correlation: B-spline coefficients, warp, validate-and-update
//   photon_piv_uncertainty.hip   displacement uncertainty per vector from correlation statistics
//   photon_optflow.hip       dense optical flow: per-pixel warp (piv_warp.hpp, shared with photon_piv_deform.hip), data terms, fused Jacobi sweeps
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/parallel_ray_tracing.h"
#include "device_optics.hpp"
#include "device_vec.hpp"
#include "device_volume.hpp"
#include "march_args.hpp"
#include "photon_pool.hpp"
#include "photon_sort.hpp"

// =============================================================================================
// error handling
// =============================================================================================
#define PH_CHECK(expr)                                                                          \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            fprintf(stderr, "photon: HIP error %d (%s) at %s:%d: %s\n", (int)_e,                \
                    hipGetErrorString(_e), __FILE__, __LINE__, #expr);                          \
            return (int)_e;                                                                     \
        }                                                                                       \
    } while (0)
// the same for a call of the library's own that returns 0 or a code its caller hands on (it has said why on stderr)
#define PH_TRY(expr)                                                                            \
    do {                                                                                        \
        const int _rc = (expr);                                                                 \
        if (_rc) return _rc;                                                                    \
    } while (0)

namespace photon {

inline bool verbose() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("PHOTON_VERBOSE"); v = (e && atoi(e) > 0) ? 1 : 0; }
    return v == 1;
}

// No C++ exception may cross the C boundary (a ctypes caller would be terminated): every extern "C" body that
// allocates host memory runs inside this guard.
template <typename F>
int guarded(const char *what, F &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        fprintf(stderr, "photon: %s failed: %s\n", what, e.what());
    } catch (...) {
        fprintf(stderr, "photon: %s failed: unknown exception\n", what);
    }
    return 100;
}

// a HIP event that is destroyed with its owner
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
    operator hipEvent_t() const { return e; }
};

}  // namespace photon

// =============================================================================================
// handles (opaque in the public header)
// =============================================================================================
struct photon_volume {
    float grad_max = 0.f;               // largest |grad n| of the texels (per micron)
    photon::VolumeDev dev{};
    photon_volume_info_t info{};
    photon::DeviceBuffer<photon::f4> texels, coeffs;     // dev.texels / dev.coeffs are views of them
};

struct photon_sources {                 // light-field sources generated in HBM (SoA, like lightfield_source_t)
    long long n = 0;
    photon::DeviceBuffer<float> x, y, z;
    photon::DeviceBuffer<double> radiance;
    photon::DeviceBuffer<int> diameter_index;
    // where the generator put them, when it can say (the PIV field's box): the largest distance from the z axis and the z range --
    // what the static skip of dead lens samples needs to know about sources it cannot read (photon_cull.hip, live_lens_samples)
    bool have_extent = false;
    double rmax = 0, zmin = 0, zmax = 0;
};

struct PermEntry { long long begin = -1, end = -1; photon::PoolBuffer<int> perm; unsigned long long stamp = 0; };

namespace photon {
// What the source cull of the volume-free path needs beside a source's coordinates (photon_cull.hip, source_misses_sensor)
struct LensCull {
    bool ok = false;
    bool thin = false;                  // element 't': one refraction on the element's plane (.cu:416-503); focal = its focal length
    double focal = 0;
    double za, zf, zb, z_sen, R1, R2a, n, hp, t, sag1, sag2, rp_all, half_x, half_y;
};
}  // namespace photon

// Every device block of a scene is a member that releases itself (photon_pool.hpp); the structs that kernels take (dev, ws)
// are views, filled from the owners.  The destructor only waits for the scene's work (scene_quiesce); whoever deletes a
// scene has its device current until the members are gone (photon_scene_free).
struct photon_scene {
    ~photon_scene();
    photon::SceneDev dev{};
    std::vector<photon::PoolBuffer<char>> allocs;       // what was uploaded: the block of small arrays, large arrays, the source list
    photon::RayStateDev ws{};           // march -> sensor state: views of the four blocks below, grown on demand (ensure_workspace)
    size_t ws_rays = 0;
    photon::PoolBuffer<float> ray_state, vprev;         // px .. dz; the resume state's last sampled values
    photon::PoolBuffer<double> radiance;
    photon::PoolBuffer<unsigned> resume;                // ctr | spins | seg_flag
    unsigned long long *d_counters = nullptr;   // kCounterSlots x kCounterStride statistics words; the last word of slot 0 is the march's
                                        // hand-off error count (scene_error_word), so whatever zeroes the statistics zeroes it too
    unsigned *d_queue = nullptr;        // the march's work queues: room for 64 counters a cache line apart, 8 XCDs x kSubQueues (4) in use + the
                                        // ticket of the waves that have left; zeroed at creation, re-armed by every launch's last wave
    int device = 0;                     // the device the scene was created on: every entry point that launches, allocates, frees or waits
                                        // for this scene makes it current first (DeviceScope) and hands the caller's device back
    int num_cus = 256;                  // compute units of the scene's device (size of the persistent march grid)
    unsigned march_epoch = 0;           // tag of the last segmented march launch in ws.seg_flag
    int march_segments = -1;            // photon_scene_set_march_segments: -1 the library's choice, 1 whole marches, n segments
    photon::PoolBuffer<unsigned long long> profile;     // wave-timing slots of the march launches (photon_scene_set_march_profile), or empty
    unsigned prof_next = 0;             // march launches since the slots were last zeroed
    photon::PoolBuffer<double> acc;     // f64 sensor accumulator, W*H
    bool acc_clean = false;             // the accumulator is all zeros (finalize_image_kernel leaves it so): the next trace needs no memset
    bool launched = false;              // kernels of this scene may be in flight: its blocks go back to the cache only after a device sync
    photon::Event ev[4];
    // statistics window (photon_scene_stats_begin / _end): traces inside it record their events and leave the counters
    // running instead of synchronising per call -- a timed loop then has no host sync and no D2H copy inside it
    bool win_open = false;
    std::vector<photon::Event> win_events;     // created on demand, reused by the next window
    size_t win_used = 0;
    std::vector<std::pair<size_t, size_t>> win_march, win_total;      // (begin, end) event indices
    uint64_t win_rays = 0;
    uint32_t win_traces = 0;
    bool win_have_volume = false;
    hipStream_t win_stream = nullptr;   // the stream the window was opened on: its traces must run there (the counters were zeroed there)
    int ray_order_mode = 2;             // 0 source-major, 1 lens-major, 2 auto (photon_scene_set_ray_order)
    bool skip_doomed = true;            // photon_scene_set_skip_doomed
    float lens_z = 0.f;                 // element 0's centre, for the auto rule
    const int *d_live = nullptr;        // the lens samples that can reach element 0's aperture from ANY source of this scene, ascending
    int live_count = 0;                 // (part of the upload block); == rays_per_source when none can be ruled out (or nothing is known)
    std::vector<int> live_host;         // the same list on the host (photon_scene_live_samples: tests hold the bound against exact geometry)
    const int *d_live_sources = nullptr;    // the sources whose image can fall on the sensor (photon_cull.hip, source_misses_sensor), ascending;
    std::vector<int> live_sources;      // part of the upload block, and the same list on the host; used by the volume-free path only
    bool live_sources_known = false;    // false: nothing could be ruled out (or the geometry is not covered): every source is launched
    bool live_sources_tried = false;    // the device pass has run (ensure_live_sources: with the scene's first volume-free trace)
    photon::LensCull source_cull;       // set at creation (host arithmetic only)
    photon::PoolBuffer<float> mom;      // moments block of the launches that record per-source moments (6 planes), grown on demand
    PermEntry perms[4];                 // spatial (Morton) orders of the lens-major launch ranges seen last
    unsigned long long perm_clock = 0;
    photon_sort_scratch sort_scratch;   // keys / indices / radix-sort temporaries, grown on demand (photon_sort.hip)
};

namespace photon {

// Makes `device` current for the scope and restores the caller's device afterwards (no HIP call at all when it already is).
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// rays per launch: bounded so that 32-bit ray ids suffice and the state stays a few GB
constexpr unsigned kMaxRaysPerLaunch = 1u << 26;

// March waves that gave a segment up or read a stale ray state (march_group) count themselves here: the spare word of
// statistics slot 0.  Zeroed with the statistics (photon_trace with stats, photon_scene_stats_begin) and when read.
inline unsigned *scene_error_word(const photon_scene *s) { return reinterpret_cast<unsigned *>(s->d_counters + CNT_N); }
constexpr size_t kCounterBytes = (size_t)kCounterSlots * kCounterStride * sizeof(unsigned long long);

// ---- photon_volume.hip ----
// the volume of `path` on the current device, uploaded once and kept while the file does not change (one per device)
// The NRRD of one call, parsed at most once on the host however many devices need it (PHOTON_DEVICES): the
// first device thread whose cache misses reads the file, the others build their volume from the same array.
struct SharedDensity {
    std::once_flag once;
    bool ok = false;
    std::string why;
    std::vector<float> rho;
    int dims[3] = {0, 0, 0};
    double spacing[3] = {1, 1, 1}, origin[3] = {0, 0, 0};
};
int cached_volume(const char *path, int interpolation, photon_volume **out, SharedDensity *shared = nullptr);

// ---- photon_scene.hip ----
// Wait for the device before blocks of this scene go back to the cache (its kernels may still be using them); no-op for a
// scene that never launched anything.
void scene_quiesce(photon_scene *s);
// The scene's regrow rule: a block that has to grow lets go of its old memory only after the scene's earlier launches are
// done with it.  Everything of a scene that grows on demand grows through here.
template <typename Buffer>
int scene_reserve(photon_scene *s, Buffer &b, size_t n) {
    if (b.p && b.n >= n) return 0;
    if (b.p) scene_quiesce(s);
    PH_CHECK(b.reserve(n));
    return 0;
}
// a block of `bytes` that the scene owns from here on
template <typename T>
int scene_block(photon_scene *s, size_t bytes, T **out) {
    s->allocs.emplace_back();
    PH_CHECK(s->allocs.back().alloc(bytes));
    *out = reinterpret_cast<T *>(s->allocs.back().p);
    return 0;
}
int ensure_workspace(photon_scene *s, size_t rays);
// room for what a segmented march keeps per ray between its pieces (after ensure_workspace, which drops it when it regrows)
int ensure_resume_state(photon_scene *s, bool linear);

// ---- photon_cull.hip ----
// scene creation: the lens samples that can reach the first aperture from some source; the constants of the source cull
std::vector<int> live_lens_samples(const std::vector<float> &lx, const std::vector<float> &ly, const lightfield_source_t *lsp,
                                   const photon_sources *generated, size_t n_sources, float image_distance, int num_elements,
                                   const element_data_t *edp, const double (*center)[3], const double (*plane)[4]);
LensCull lens_cull_setup(const std::vector<float> &lx, const std::vector<float> &ly, float image_distance, float beam_wavelength,
                         int num_elements, const element_data_t *edp, const double (*center)[3], const double (*plane)[4],
                         const int *sys_index, const camera_design_t *cam);
// the scene's list of sources that can reach the sensor, made on first use (a device pass on the null stream, host waits)
int ensure_live_sources(photon_scene *s);
// What the launches of one trace share.  Made per trace, never kept: the scene's setters take effect on the next trace.
struct TracePlan {
    bool live_samples_only;             // slot_rays = live_count, slot_map = d_live
    bool listed_sources;                // launches take slices of scene->live_sources
    bool lens_major;                    // lens-major order over Morton-sorted sources
    float doom_margin;                  // rays further than this outside the first aperture are not marched; 0 = off
    int slot_rays;                      // slots per source of every launch
    long long max_sources;              // (listed) sources per launch
    MarchKnobs march;                   // how the marches may be cut into pieces (march_knobs)
};
TracePlan make_trace_plan(photon_scene *s, const photon_volume *vol, int algorithm, bool dumping, bool with_moments);
// one launch of a trace: sources [begin, end) in the caller's order, of which n_sources are launched -- src_list when they are listed
struct LaunchRange { long long begin, end, n_sources; const int *src_list; };
LaunchRange next_launch(const photon_scene *s, const TracePlan &plan, long long begin, long long limit);

// ---- photon_march.hip ----
// The scene's setting (photon_scene_set_march_segments: -1 none) or else PHOTON_MARCH_SEGMENTS, and PHOTON_MARCH_SEGMENT_SHAPE.
MarchKnobs march_knobs(int scene_segments);
// What the march launch of n rays is (stage 1b): kernel, grid, queue chunks, pieces.  Pure: no HIP call, no environment, no scene.
// dumps: intermediate ray dumps are asked for; ray_order: SceneDev::ray_order of the launch; have_rays: the rays' state already
// sits in the workspace (a raygen kernel ran, or the caller put it there)
MarchPlan plan_march(unsigned n, int num_cus, const VolumeDev &vol, int algorithm, bool dumps, bool noise, int ray_order, bool have_rays,
                     const MarchKnobs &knobs);
// Enqueues the march the plan describes over the rays in the scene's workspace; decides nothing and allocates nothing (the
// caller has made room: ensure_workspace, and ensure_resume_state for a plan of several pieces).  With plan.fold the march
// generates the rays of sources [src_begin, ...) itself.  dev: the scene as this launch sees it (launch_chunk)
int launch_march(photon_scene *s, const SceneDev &dev, const photon_volume *vol, const MarchPlan &plan, unsigned long long ray_base,
                 const InterDump &idump, long long src_begin, hipStream_t stream, hipEvent_t ev_march_begin);
// Did any march wave give a segment up?  Reads (and clears) the scene's error word; the caller has synchronised.
int march_error_check(photon_scene *scene);
int profile_reset(photon_scene *s, hipStream_t stream);

// ---- the march kernels, one unit per sampler (photon_march_linear.hip / _cubic.hip / _extra.hip) ----
int march_launch_extra(int algorithm, dim3 grid, dim3 block, hipStream_t stream, const VolumeDev &vol, unsigned n_rays, const RayStateDev &st,
                       unsigned long long *counters);
// plain one-thread-per-ray grids over [n][3] position / direction arrays (photon_trace_volume_rays)
int march_rays_launch_linear(int algorithm, const VolumeDev &vol, const f4 *tex, int n, float *pos, float *dir, int *steps);
int march_rays_launch_cubic(int algorithm, const VolumeDev &vol, const f4 *tex, int n, float *pos, float *dir, int *steps);
int march_rays_launch_extra(int algorithm, const VolumeDev &vol, int n, float *pos, float *dir, int *steps);

// ---- photon_sensor.hip ----
int launch_raygen(photon_scene *s, const SceneDev &dev, long long src_begin, unsigned n, hipStream_t stream);
// the sensor stage of a launch of n rays: from the marched state (from_state) or generating its rays in place; with mom, every
// arriving ray also lands in the launch's moments block
int launch_sensor(photon_scene *s, const SceneDev &dev, bool from_state, long long src_begin, unsigned n, const DumpDev &dump,
                  hipStream_t stream, const MomentsDev *mom = nullptr);

// ---- photon_moments.hip ----
constexpr int kMomentFields = 8;        // n, sum x, y, z, sum acos dx, dy, dz, sum x^2 + y^2 (include/parallel_ray_tracing.h)
// The records of the `places` sources of a launch from its moments block: place p is source src_list[p] (src_list) or
// src_begin + p; record of source i at records + kMomentFields * i
int launch_moments(const MomentsDev &mom, unsigned places, unsigned rays_per_source, long long src_begin, const int *src_list,
                   double *records, hipStream_t stream);
// image = (float)(image + accumulator): image_array is read-modify-write (parallel_ray_tracing.cu:3309, 3675)
int launch_finalize(photon_scene *s, float *d_image, hipStream_t stream);

// ---- photon_trace.hip ----
int begin_accumulate(photon_scene *s, hipStream_t stream);
// One launch of a trace: decides nothing (plan, range: photon_cull.hip).
// d_records: also the per-source moments of the launched sources (records of the scene's source list, photon_trace_moments)
int launch_chunk(photon_scene *s, const photon_volume *vol, int algorithm, const TracePlan &plan, const LaunchRange &range, DumpDev dump,
                 hipStream_t stream, hipEvent_t ev_march_begin, hipEvent_t ev_march_end, double *d_records = nullptr);
// The launch loop for sources [src_begin, src_end) into the scene's private f64 accumulator (zeroed first); timed: 0 no
// events, 1 immediate (host waits per launch), 2 deferred (events of the open statistics window).  d_records: the records of
// [src_begin, src_end) are zeroed on the stream, then every launch writes those of the sources it traced.
int trace_accumulate(photon_scene *scene, const photon_volume *vol, int ray_tracing_algorithm, long long src_begin,
                     long long src_end, hipStream_t stream, int timed, float *march_ms_out, double *d_records = nullptr);
// zero the records of sources [src_begin, src_end) on the stream (their sources may all be culled)
int clear_records(double *d_records, long long src_begin, long long src_end, hipStream_t stream);

// photon_scene.hip: a source handle with device arrays for n sources, the caller's until it releases it; the extent of generated sources (photon_cull.hip, live_lens_samples)
int sources_alloc(long long n, std::unique_ptr<photon_sources> *out);
void sources_set_extent(photon_sources *src, double ax, double ay, double z0, double z1);

}  // namespace photon
