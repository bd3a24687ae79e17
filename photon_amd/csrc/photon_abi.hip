// photon_abi.hip - the reference's entry point: start_ray_tracing (cuda_codes/parallel_ray_tracing.cu:3078-3775) on
// host arrays, as photon's unmodified Python calls it through ctypes (perform_ray_tracing_03.py:1888-1938), and
// PHOTON_DEVICES: the sources of ONE call sharded over several devices, their accumulators summed by one kernel.
#include <chrono>
#include <cstring>
#include <fstream>
#include <map>
#include <condition_variable>
#include <thread>

#include "photon_internal.hpp"

using namespace photon;

namespace {

using Clock = std::chrono::steady_clock;
double ms(Clock::time_point from, Clock::time_point to) { return std::chrono::duration<double, std::milli>(to - from).count(); }

// The arguments of one start_ray_tracing call but the image (include/parallel_ray_tracing.h).
struct CallArgs {
    float lens_pitch, image_distance;
    scattering_data_t *sdp; char *scattering_type_str; lightfield_source_t *lsp;
    int rays_per_source; float beam_wavelength, f_number; int num_elements;
    double (*element_center)[3]; element_data_t *edp; double (*element_planes)[4]; int *sys_index;
    camera_design_t *cam; bool density; char *density_path;
    bool save_lightrays; char *pos_path, *dir_path; int num_lightrays_save; int algorithm;
    bool add_pos_noise; float pos_noise_std; bool add_ngrad_noise; float ngrad_noise_std; float ratio;
    bool save_intermediate; int num_intermediate_save;
    bool dumping() const { return save_lightrays && num_lightrays_save > 0; }
};

// The environment knobs of one call (the ABI has no room for them: include/parallel_ray_tracing.h), read once at its start.
// PHOTON_VERBOSE is the library's, not the call's (verbose()).
struct CallSettings {
    int interpolation;          // PHOTON_INTERP=cubic: 2; else 1, which the reference hard-codes (interpolation_scheme = 1, .cu:3330)
    int element_train;          // PHOTON_ELEMENT_TRAIN=sequential: the working multi-element train instead of the reference's
                                // "element 0 for every single-member group, nothing for the others" (.cu:1331-1333, 1049-1272)
    int ray_order;              // PHOTON_RAY_ORDER=source|lens|auto (photon_scene_set_ray_order)
    int skip_doomed;            // PHOTON_SKIP_DOOMED=0 marches every ray like the reference does (photon_scene_set_skip_doomed)
    int weight_bits;            // PHOTON_TEX_WEIGHTS=fixed8|exact: trilinear weights as the reference's texture unit holds them (8
                                // fractional bits: the documented arithmetic of the tex3D() the reference calls; default) or as exact f32
    uint64_t noise_seed;        // PHOTON_NOISE_SEED: the noise hooks' seed, instead of the reference's time(NULL)
    bool peer_reads;            // PHOTON_PEER_READS=0: never dereference another device's memory, always stage (for a node whose
                                // peer mappings misbehave)
    std::vector<int> devices;   // PHOTON_DEVICES (parse_devices)
};

// PHOTON_DEVICES: "all", or a comma-separated list of device ordinals (repeats allowed: "0,0" renders two
// shards side by side on device 0).  Empty = the calling thread's current device only.
std::vector<int> parse_devices(const char *e) {
    std::vector<int> out;
    if (!e || !*e) return out;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return out;
    if (strcmp(e, "all") == 0) {
        for (int d = 0; d < count; d++) out.push_back(d);
        return out;
    }
    const char *p = e;
    while (*p) {
        char *end = nullptr;
        const long d = strtol(p, &end, 10);
        if (end == p) break;
        if (d < 0 || d >= count) {
            fprintf(stderr, "photon: PHOTON_DEVICES names device %ld, %d present; using the current device\n", d, count);
            out.clear();
            return out;
        }
        out.push_back((int)d);
        p = *end == ',' ? end + 1 : end;
        if (*end && *end != ',') break;
    }
    return out;
}

CallSettings settings_from_env() {
    auto is = [](const char *e, const char *a, const char *b = nullptr) { return e && (strcmp(e, a) == 0 || (b && strcmp(e, b) == 0)); };
    CallSettings s;
    s.interpolation = is(getenv("PHOTON_INTERP"), "cubic", "2") ? 2 : 1;
    s.element_train = is(getenv("PHOTON_ELEMENT_TRAIN"), "sequential", "1") ? 1 : 0;
    const char *order = getenv("PHOTON_RAY_ORDER");
    s.ray_order = is(order, "source") ? 0 : is(order, "lens") ? 1 : 2;
    s.skip_doomed = !is(getenv("PHOTON_SKIP_DOOMED"), "0");
    s.weight_bits = is(getenv("PHOTON_TEX_WEIGHTS"), "exact", "0") ? 0 : 8;
    const char *seed = getenv("PHOTON_NOISE_SEED");
    s.noise_seed = seed ? strtoull(seed, nullptr, 0) : 0x5eedULL;
    s.peer_reads = !is(getenv("PHOTON_PEER_READS"), "0");
    s.devices = parse_devices(getenv("PHOTON_DEVICES"));
    return s;
}

// The scene of the call's sources [begin, end) on the current device, set up as the call and its settings say, and the call's
// volume (cached on the device; with `shared`, the NRRD is parsed once for all devices of the call).  Returns 2 when the scene
// upload fails (*scene stays null), else what cached_volume returns; *scene_ready is when the scene was set up.
int setup_scene(const CallArgs &a, const CallSettings &cs, long long begin, long long end, SharedDensity *shared,
                photon_scene **scene, photon_volume **vol, Clock::time_point *scene_ready = nullptr) {
    lightfield_source_t block = *a.lsp;                                 // [begin, end) of the caller's arrays
    block.x += begin; block.y += begin; block.z += begin; block.radiance += begin; block.diameter_index += begin;
    block.num_particles = (int)(end - begin);
    if (photon_scene_create(a.lens_pitch, a.image_distance, a.sdp, a.scattering_type_str, &block, a.rays_per_source,
                            a.beam_wavelength, a.f_number, a.num_elements, a.element_center, a.edp, a.element_planes,
                            a.sys_index, a.cam, a.ratio, scene)) return 2;
    photon_scene *sc = *scene;
    photon_scene_set_source_base(sc, begin);
    // the reference's noise switches; gradient noise only exists inside the volume march (Euler, .h:853-863)
    photon_scene_set_noise(sc, a.add_pos_noise, a.pos_noise_std, a.density && a.add_ngrad_noise, a.ngrad_noise_std, cs.noise_seed);
    photon_scene_set_element_train(sc, cs.element_train);
    photon_scene_set_ray_order(sc, cs.ray_order);
    photon_scene_set_skip_doomed(sc, cs.skip_doomed);
    if (scene_ready) *scene_ready = Clock::now();
    if (!a.density) return 0;
    const int rc = cached_volume(a.density_path, cs.interpolation, vol, shared);
    if (!rc) photon_volume_set_weight_bits(*vol, cs.weight_bits);
    return rc;
}

// A HIP error that ends the call: said on stderr as the call's one "image left untouched" line.
bool hip_failed(hipError_t err, int line) {
    if (err == hipSuccess) return false;
    fprintf(stderr, "photon: HIP error %d (%s) at %s:%d; image left untouched\n", (int)err, hipGetErrorString(err), __FILE__, line);
    return true;
}

bool write_dump(const char *dir, const char *prefix, int k, const std::vector<float> &v) {
    char name[64];
    snprintf(name, sizeof name, "%s%04d.bin", prefix, k);               // .cu:3574
    const std::string full = std::string(dir) + "/" + name;
    std::ofstream f(full.c_str(), std::ios::out | std::ios::binary);
    if (!f) { fprintf(stderr, "photon: cannot write %s\n", full.c_str()); return false; }
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
    f.flush();
    if (!f) { fprintf(stderr, "photon: short write to %s\n", full.c_str()); return false; }
    return true;
}


// ---------------------------------------------------------------------------------------------
// PHOTON_DEVICES: one call, several devices
// ---------------------------------------------------------------------------------------------
// The sum of the per-device f64 accumulators, on the first device, by ONE kernel: every thread reads its pixel of up to
// kGatherPeers other accumulators THROUGH THEIR PEER-MAPPED POINTERS (xGMI is point to point: the seven links of the
// first device are read concurrently, 8 MiB each for a 1024^2 sensor) and adds them in device-list order -- f64 end to
// end, one rounding per pixel, the same bits whatever the number of devices -- and, in the last launch of a call, folds
// the sum into the caller's image (image_array is read-modify-write: parallel_ray_tracing.cu:3309, 3675).  No staging
// buffer, no host synchronisation per peer.  Two pixels per thread: 16-byte loads across the links.
constexpr int kGatherPeers = 15;
struct GatherArgs { const double *peer[kGatherPeers]; int n; };
__global__ __launch_bounds__(256) void gather_sum_kernel(double *__restrict__ acc, GatherArgs g, float *__restrict__ image, size_t n) {
    const size_t i = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 1 < n) {
        double2 s = *reinterpret_cast<const double2 *>(acc + i);
#pragma unroll
        for (int k = 0; k < kGatherPeers; k++)
            if (k < g.n) { const double2 p = *reinterpret_cast<const double2 *>(g.peer[k] + i); s.x += p.x; s.y += p.y; }
        if (image) { image[i] = (float)((double)image[i] + s.x); image[i + 1] = (float)((double)image[i + 1] + s.y); }
        else *reinterpret_cast<double2 *>(acc + i) = s;
    } else if (i < n) {                                                 // odd pixel count: the last one alone
        double s = acc[i];
#pragma unroll
        for (int k = 0; k < kGatherPeers; k++) if (k < g.n) s += g.peer[k][i];
        if (image) image[i] = (float)((double)image[i] + s); else acc[i] = s;
    }
}

// A non-blocking stream per (device, worker slot), created once per process: workers that share a device (PHOTON_DEVICES
// with repeats: tests, rehearsals) then run side by side instead of queueing on the null stream.
hipStream_t worker_stream(int device, int slot) {
    static std::mutex lock;
    static std::map<std::pair<int, int>, hipStream_t> *streams = new std::map<std::pair<int, int>, hipStream_t>;
    std::lock_guard<std::mutex> g(lock);
    auto it = streams->find({device, slot});
    if (it != streams->end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s = nullptr; }     // the null stream still works
    (*streams)[{device, slot}] = s;
    return s;
}

// PHOTON_DEVICES (SURVEY 8e inside ONE call, for photon's single Python process).  What is distributed is the reference's
// chunk loop over light-field sources (parallel_ray_tracing.cu:3505-3558): the sources are cut into contiguous,
// count-balanced blocks, one per listed device; each device's host thread uploads ONLY its block (plus the replicated
// tables, optics and volume -- the NRRD is parsed once, SharedDensity); when every thread has done so (a rendezvous) each
// renders into its scene's private f64 accumulator on a stream of its own, while the calling thread uploads the caller's image to the first device (peer access
// from the first device to the others has been settled before: once per pair and process).  When the workers are done ONE kernel on the first device sums the
// accumulators through their peer-mapped pointers and folds the sum into the image (gather_sum_kernel).  A device the
// first one cannot map (no xGMI / PCIe peer path) has its accumulator copied into a block of the cache first
// (hipMemcpyPeerAsync, all such copies in flight together) -- said on stderr when the pair is first seen, and per call
// under PHOTON_VERBOSE.
// moments (photon_start_ray_tracing_moments): each worker also reduces its shard's per-source moments on its device and copies
// them into its own slice of the caller's f64[num_particles][8].
int render_on_devices(const CallArgs &a, const CallSettings &cs, float *image_array, double *moments) {
    const std::vector<int> &devices = cs.devices;
    const long long n_src = a.lsp->num_particles;
    const size_t npix = (size_t)a.cam->x_pixel_number * a.cam->y_pixel_number;
    const size_t K = devices.size();
    std::vector<photon_scene *> scenes(K, nullptr);
    std::vector<int> rcs(K, 0), slot(K, 0);
    for (size_t k = 0; k < K; k++)                                      // k-th worker of its device
        for (size_t j = 0; j < k; j++) slot[k] += devices[j] == devices[k];
    SharedDensity shared;
    std::vector<std::thread> workers;
    const auto t_start = Clock::now();
    // peer access from the first device to the others, BEFORE any worker allocates its accumulator: what the sum's kernel
    // dereferences must have been allocated under the mapping (photon_pool.hpp); once per pair and process, then a table look-up
    std::vector<char> direct(K, 1);
    for (size_t k = 1; k < K; k++) direct[k] = devices[k] == devices[0] || (cs.peer_reads && peer_access(devices[0], devices[k])) ? 1 : 0;
    // Two phases with a rendezvous between them: every worker first builds its scene (uploads) and gets its volume, THEN all
    // start tracing.  With distinct devices the rendezvous costs the spread of eight equal uploads; with a device listed more
    // than once (rehearsals, tests: all eight on one) it keeps one shard's uploads -- blit kernels -- from queueing behind
    // another shard's march, whose persistent waves hold every wave slot of the device until they are done.
    struct Rendezvous {
        std::mutex m; std::condition_variable cv; size_t waiting = 0, total;
        explicit Rendezvous(size_t n) : total(n) {}
        void arrive_and_wait() {
            std::unique_lock<std::mutex> g(m);
            if (++waiting >= total) cv.notify_all();
            else cv.wait(g, [&] { return waiting >= total; });
        }
        void expect(size_t n) {                                         // fewer parties after all (a thread could not be started)
            std::lock_guard<std::mutex> g(m);
            total = n;
            if (waiting >= total) cv.notify_all();
        }
    } rendezvous(K);
    std::vector<photon_volume *> volumes(K, nullptr);
    bool all_started = true;
    for (size_t k = 0; k < K && all_started; k++) {
        try {
        workers.emplace_back([&, k]() {
            const long long b = n_src * (long long)k / (long long)K, e2 = n_src * (long long)(k + 1) / (long long)K;
            hipStream_t stream = nullptr;
            const int rc_setup = guarded("start_ray_tracing (device worker, setup)", [&]() -> int {
                if (hipSetDevice(devices[k]) != hipSuccess) return 1;
                stream = worker_stream(devices[k], slot[k]);
                return setup_scene(a, cs, b, e2, &shared, &scenes[k], &volumes[k]);
            });
            rendezvous.arrive_and_wait();                               // on every path: a worker that failed still arrives
            if (rc_setup) { rcs[k] = rc_setup; return; }
            rcs[k] = guarded("start_ray_tracing (device worker)", [&]() -> int {
                const auto tw = Clock::now();
                PoolBuffer<double> d_records;                           // this shard's records (moments only)
                if (moments && d_records.alloc((size_t)(e2 - b) * kMomentFields) != hipSuccess) return 2;
                int rc = trace_accumulate(scenes[k], volumes[k], a.algorithm, 0, e2 - b, stream, 0, nullptr, d_records.p);
                if (rc) (void)hipStreamSynchronize(stream);             // launches may be in flight: d_records goes back to the cache
                if (!rc && hipStreamSynchronize(stream) != hipSuccess) rc = 4;
                if (!rc) rc = march_error_check(scenes[k]);
                if (!rc && moments && hipMemcpy(moments + (size_t)b * kMomentFields, d_records.p, (size_t)(e2 - b) * kMomentFields * sizeof(double),
                                                hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
                if (!rc && verbose())
                    fprintf(stderr, "photon: device %d: sources [%lld, %lld) traced in %.3f ms\n", devices[k], b, e2,
                            ms(tw, Clock::now()));
                return rc;
            });
        });
        } catch (const std::exception &ex) {                            // no thread: the ones already running must not wait for it
            fprintf(stderr, "photon: cannot start the worker thread of device %d (%s); image left untouched\n", devices[k], ex.what());
            rendezvous.expect(workers.size());
            all_started = false;
        }
    }
    // meanwhile, on the calling thread: the caller's image onto the first device
    int rc = all_started ? 0 : 1;
    auto check = [&](hipError_t err, int line) {
        if (!rc && hip_failed(err, line)) rc = (int)err;
        return rc == 0;
    };
    PoolBuffer<float> d_img;
    if (check(hipSetDevice(devices[0]), __LINE__) && check(d_img.alloc(npix), __LINE__))
        check(hipMemcpy(d_img.p, image_array, npix * sizeof(float), hipMemcpyHostToDevice), __LINE__);      // .cu:3309
    for (auto &w : workers) w.join();
    const auto t_traced = Clock::now();
    for (size_t k = 0; k < K && !rc; k++)
        if (rcs[k]) { fprintf(stderr, "photon: device %d failed (%d); image left untouched\n", devices[k], rcs[k]); rc = rcs[k]; }
    // ---- the sum, on the first device ----
    std::vector<PoolBuffer<double>> staged(K);
    size_t n_staged = 0;
    if (!rc && check(hipSetDevice(devices[0]), __LINE__)) {
        std::vector<const double *> peers;
        for (size_t k = 1; k < K && !rc; k++) {
            const double *other = scenes[k]->acc.p;
            if (!direct[k]) {                                           // no peer mapping: the runtime stages the copy through the host
                if (!check(staged[k].alloc(npix), __LINE__)) break;
                if (!check(hipMemcpyPeerAsync(staged[k].p, devices[0], other, devices[k], npix * sizeof(double), nullptr), __LINE__)) break;
                other = staged[k].p;
                n_staged++;
            }
            peers.push_back(other);
        }
        const dim3 grid((unsigned)((npix / 2 + 1 + 255) / 256)), block(256);
        for (size_t at = 0; !rc; at += kGatherPeers) {
            GatherArgs g{};
            g.n = (int)std::min<size_t>(kGatherPeers, peers.size() - at);
            for (int j = 0; j < g.n; j++) g.peer[j] = peers[at + j];
            const bool last = at + g.n >= peers.size();
            hipLaunchKernelGGL(gather_sum_kernel, grid, block, 0, nullptr, scenes[0]->acc.p, g, last ? d_img.p : nullptr, npix);
            if (!check(hipGetLastError(), __LINE__) || last) break;
        }
        if (!rc) check(hipMemcpy(image_array, d_img.p, npix * sizeof(float), hipMemcpyDeviceToHost), __LINE__);      // .cu:3675 (waits for the kernel)
    }
    if (verbose()) {
        const auto t_end = Clock::now();
        fprintf(stderr, "photon: %zu devices: shards traced in %.3f ms (uploads included); sum of %zu accumulators on device %d (%zu by direct peer reads, "
                        "%zu staged) + fold + image out: %.3f ms\n", K, ms(t_start, t_traced), K, devices[0],
                K - 1 - n_staged, n_staged, ms(t_traced, t_end));
    }
    for (size_t k = 0; k < K; k++)
        if (scenes[k]) { (void)hipSetDevice(devices[k]); photon_scene_free(scenes[k]); }       // waits for the device first
    (void)hipSetDevice(devices[0]);
    if (rc) (void)hipDeviceSynchronize();                               // a failed call may have left copies or the sum in flight: the
                                                                        // staged blocks and the image block go back to the cache on return
    return rc;
}

// Device blocks of the ray dumps (save_lightrays, save_intermediate_ray_data).
struct DumpBuffers { PoolBuffer<float> pos, dir, inter_pos, inter_dir; };

// The trace of a call that dumps its rays, folded into d_image.  The reference's chunking decides which rays land in which
// pos_/dir_ file (.cu:3366-3372, 3515-3611): chunks of source_point_number sources, one file pair per chunk; intermediate
// dumps ride on the same chunking (.cu:3484-3492, 3535-3546, 3613-3670).
// d_records: also the per-source moments of every chunk (photon_start_ray_tracing_moments).
int trace_with_dumps(const CallArgs &a, photon_scene *scene, const photon_volume *vol, float *d_image, DumpBuffers &d, double *d_records) {
    const long long num_particles = a.lsp->num_particles;
    long long chunk = a.lsp->source_point_number;
    if (num_particles < chunk) chunk = num_particles;
    if (chunk < 1) chunk = 1;
    if ((unsigned long long)(chunk * a.rays_per_source) > kMaxRaysPerLaunch) {
        fprintf(stderr, "photon: source_point_number*rays exceeds %u rays per launch\n", kMaxRaysPerLaunch);
        return 1;
    }
    const size_t nsave = (size_t)a.num_lightrays_save * 3;
    const bool inter = a.density && a.save_intermediate && a.num_intermediate_save > 0;
    const size_t ninter = inter ? nsave * (size_t)a.num_intermediate_save : 0;
    PH_CHECK(d.pos.alloc(nsave));
    PH_CHECK(d.dir.alloc(nsave));
    if (inter) {
        PH_CHECK(d.inter_pos.alloc(ninter));
        PH_CHECK(d.inter_dir.alloc(ninter));
    }
    std::vector<float> host(nsave), host_inter(ninter);
    const DumpDev dump{d.pos.p, d.dir.p, a.num_lightrays_save, d.inter_pos.p, d.inter_dir.p, inter ? a.num_intermediate_save : 0};
    const long long kmax = (num_particles + chunk - 1) / chunk;
    const TracePlan plan = make_trace_plan(scene, vol, a.algorithm, dump.final_pos || dump.inter_pos, d_records != nullptr);
    PH_TRY(begin_accumulate(scene, nullptr));
    if (d_records) PH_TRY(clear_records(d_records, 0, num_particles, nullptr));
    for (long long k = 0; k < kmax; k++) {
        PH_CHECK(hipMemsetAsync(d.pos.p, 0xFF, nsave * sizeof(float), nullptr));     // all-ones = NaN (.cu:3527-3533); the null stream, like the chunk's launches
        PH_CHECK(hipMemsetAsync(d.dir.p, 0xFF, nsave * sizeof(float), nullptr));
        if (inter) {
            PH_CHECK(hipMemsetAsync(d.inter_pos.p, 0xFF, ninter * sizeof(float), nullptr));
            PH_CHECK(hipMemsetAsync(d.inter_dir.p, 0xFF, ninter * sizeof(float), nullptr));
        }
        const LaunchRange range = next_launch(scene, plan, k * chunk, std::min(num_particles, (k + 1) * chunk));     // the whole chunk
        PH_TRY(launch_chunk(scene, vol, a.algorithm, plan, range, dump, nullptr, nullptr, nullptr, d_records));
        bool wrote = true;                                              // a dump that cannot be written fails the call
        PH_CHECK(hipMemcpy(host.data(), d.pos.p, nsave * sizeof(float), hipMemcpyDeviceToHost));
        wrote = write_dump(a.pos_path, "pos_", (int)k, host) && wrote;
        PH_CHECK(hipMemcpy(host.data(), d.dir.p, nsave * sizeof(float), hipMemcpyDeviceToHost));
        wrote = write_dump(a.dir_path, "dir_", (int)k, host) && wrote;
        if (inter) {
            PH_CHECK(hipMemcpy(host_inter.data(), d.inter_pos.p, ninter * sizeof(float), hipMemcpyDeviceToHost));
            wrote = write_dump(a.pos_path, "intermediate_pos_", (int)k, host_inter) && wrote;
            PH_CHECK(hipMemcpy(host_inter.data(), d.inter_dir.p, ninter * sizeof(float), hipMemcpyDeviceToHost));
            wrote = write_dump(a.dir_path, "intermediate_dir_", (int)k, host_inter) && wrote;
        }
        if (!wrote) return 5;
    }
    return launch_finalize(scene, d_image, nullptr);
}

// When the phases of a one-device call ended (PHOTON_VERBOSE: where a call's time goes beside the trace itself).
struct Phases { Clock::time_point start, scene, volume, image_in, trace, image_out; };

// The call on the current device: 0, or non-zero once stderr has said why.  The device blocks are declared before the
// scene, so the scene is freed first: photon_scene_free waits for the device, and no block may go back to the cache while
// a kernel of the call can still use it.
// moments: also the per-source moments, into the caller's f64[num_particles][8] (photon_start_ray_tracing_moments).
int render_on_one_device(const CallArgs &a, const CallSettings &cs, float *image_array, Phases &t, double *moments) {
    PoolBuffer<float> d_image;
    PoolBuffer<double> d_records;
    DumpBuffers dumps;
    struct SceneOwner { photon_scene *p = nullptr; ~SceneOwner() { photon_scene_free(p); } } scene;
    photon_volume *vol = nullptr;                                       // the device's cached volume: not the call's to free
    const long long num_particles = a.lsp->num_particles;
    if (const int rc = setup_scene(a, cs, 0, num_particles, nullptr, &scene.p, &vol, &t.scene)) {
        // (a volume says why itself, but not what becomes of the image)
        fprintf(stderr, "photon: %s failed; image left untouched\n", scene.p ? "the density volume" : "scene upload");
        return rc;
    }
    t.volume = Clock::now();
    const size_t npix = (size_t)a.cam->x_pixel_number * a.cam->y_pixel_number;
    if (hip_failed(d_image.alloc(npix), __LINE__) ||
        hip_failed(hipMemcpy(d_image.p, image_array, npix * sizeof(float), hipMemcpyHostToDevice), __LINE__)) return 1;  // .cu:3309
    if (moments && hip_failed(d_records.alloc((size_t)num_particles * kMomentFields), __LINE__)) return 1;
    t.image_in = Clock::now();
    int rc;
    if (a.dumping()) {
        rc = trace_with_dumps(a, scene.p, vol, d_image.p, dumps, d_records.p);
    } else {
        if (a.density && a.save_intermediate)
            fprintf(stderr, "photon: warning: save_intermediate_ray_data needs save_lightrays with num_lightrays_save > 0 "
                            "(the reference sizes the intermediate buffers by it, .cu:3488); nothing recorded\n");
        rc = moments ? photon_trace_moments(scene.p, vol, a.algorithm, 0, num_particles, d_image.p, d_records.p, nullptr)
                     : photon_trace(scene.p, vol, a.algorithm, 0, num_particles, d_image.p, nullptr, nullptr);
    }
    if (rc) {
        fprintf(stderr, "photon: trace failed (%d); image left untouched\n", rc);
        return rc;
    }
    if (hip_failed(hipDeviceSynchronize(), __LINE__)) return 1;
    t.trace = Clock::now();
    if (march_error_check(scene.p)) {
        fprintf(stderr, "photon: trace failed; image left untouched\n");
        return 1;
    }
    if (hip_failed(hipMemcpy(image_array, d_image.p, npix * sizeof(float), hipMemcpyDeviceToHost), __LINE__)) return 1;  // .cu:3675
    if (moments && hip_failed(hipMemcpy(moments, d_records.p, (size_t)num_particles * kMomentFields * sizeof(double), hipMemcpyDeviceToHost),
                              __LINE__)) return 1;
    t.image_out = Clock::now();
    return 0;
}

// 0, or non-zero once stderr has said why.  moments: also the per-source moments (photon_start_ray_tracing_moments).
int start_ray_tracing_impl(const CallArgs &a, float *image_array, double *moments = nullptr) {
    const auto t0 = Clock::now();
    if (!image_array || !a.cam || !a.lsp) {
        fprintf(stderr, "photon: start_ray_tracing: null argument; image left untouched\n");
        return 1;
    }
    const CallSettings cs = settings_from_env();
    int caller_device = 0;                                              // the caller's current device is restored on every path
    const bool have_caller_device = hipGetDevice(&caller_device) == hipSuccess;
    struct RestoreDevice { bool on; int dev; ~RestoreDevice() { if (on) (void)hipSetDevice(dev); } } restore{have_caller_device, caller_device};
    const long long n_src = a.lsp->num_particles, rps = a.rays_per_source;
    // PHOTON_DEVICES: shard the sources of one call over several GPUs.  Ray dumps keep the
    // reference's chunk -> file mapping and stay on one device.
    if (cs.devices.size() > 1 && !a.dumping()) {
        const int rc = render_on_devices(a, cs, image_array, moments);
        if (!rc && verbose()) {
            const double sec = ms(t0, Clock::now()) * 1e-3;
            printf("photon: %lld sources x %d rays on %zu devices in %.3f s (%.2f Mrays/s incl. transfers)\n", n_src,
                   a.rays_per_source, cs.devices.size(), sec, n_src * (double)rps / sec * 1e-6);
        }
        return rc;
    }
    if (!cs.devices.empty() && hipSetDevice(cs.devices[0]) != hipSuccess) {
        fprintf(stderr, "photon: cannot select device %d; image left untouched\n", cs.devices[0]);
        return 1;
    }
    Phases t{t0};
    PH_TRY(render_on_one_device(a, cs, image_array, t, moments));
    if (!verbose()) return 0;
    const auto t_end = Clock::now();                                    // the call's blocks and scene are freed
    const double s = ms(t0, t_end) * 1e-3;
    printf("photon: %lld sources x %lld rays in %.3f s (%.2f Mrays/s incl. transfers)\n", n_src, rps, s, n_src * rps / s * 1e-6);
    printf("photon:   scene upload %.2f ms, volume %.2f, image in %.2f, trace (launches + wait) %.2f, image out %.2f, frees %.2f\n",
           ms(t.start, t.scene), ms(t.scene, t.volume), ms(t.volume, t.image_in), ms(t.image_in, t.trace), ms(t.trace, t.image_out),
           ms(t.image_out, t_end));
    return 0;
}

}  // namespace

// The exported symbol: no C++ exception crosses the C boundary.
extern "C" void start_ray_tracing(float lens_pitch, float image_distance, scattering_data_t *scattering_data_p,
                                  char *scattering_type_str, lightfield_source_t *lightfield_source_p,
                                  int lightray_number_per_particle, float beam_wavelength, float aperture_f_number,
                                  int num_elements, double (*element_center)[3], element_data_t *element_data_p,
                                  double (*element_plane_parameters)[4], int *element_system_index,
                                  camera_design_t *camera_design_p, float *image_array,
                                  bool simulate_density_gradients, char *density_grad_filename, bool save_lightrays,
                                  char *lightray_position_save_path, char *lightray_direction_save_path,
                                  int num_lightrays_save, int ray_tracing_algorithm, bool add_pos_noise,
                                  float pos_noise_std, bool add_ngrad_noise, float ngrad_noise_std,
                                  float ray_cone_pitch_ratio, bool save_intermediate_ray_data,
                                  int num_intermediate_positions_save) {
    (void)guarded("start_ray_tracing", [&]() -> int {
        const CallArgs a{lens_pitch, image_distance, scattering_data_p, scattering_type_str, lightfield_source_p,
                         lightray_number_per_particle, beam_wavelength, aperture_f_number, num_elements, element_center,
                         element_data_p, element_plane_parameters, element_system_index, camera_design_p,
                         simulate_density_gradients, density_grad_filename, save_lightrays, lightray_position_save_path,
                         lightray_direction_save_path, num_lightrays_save, ray_tracing_algorithm, add_pos_noise, pos_noise_std,
                         add_ngrad_noise, ngrad_noise_std, ray_cone_pitch_ratio, save_intermediate_ray_data,
                         num_intermediate_positions_save};
        start_ray_tracing_impl(a, image_array);
        return 0;
    });
}

// start_ray_tracing plus the per-source sensor moments (include/parallel_ray_tracing.h): the same call setup, settings and
// launch plans, and source_moments = host f64[num_particles][8].
extern "C" int photon_start_ray_tracing_moments(float lens_pitch, float image_distance, scattering_data_t *scattering_data_p,
                                                char *scattering_type_str, lightfield_source_t *lightfield_source_p,
                                                int lightray_number_per_particle, float beam_wavelength, float aperture_f_number,
                                                int num_elements, double (*element_center)[3], element_data_t *element_data_p,
                                                double (*element_plane_parameters)[4], int *element_system_index,
                                                camera_design_t *camera_design_p, float *image_array,
                                                bool simulate_density_gradients, char *density_grad_filename, bool save_lightrays,
                                                char *lightray_position_save_path, char *lightray_direction_save_path,
                                                int num_lightrays_save, int ray_tracing_algorithm, bool add_pos_noise,
                                                float pos_noise_std, bool add_ngrad_noise, float ngrad_noise_std,
                                                float ray_cone_pitch_ratio, bool save_intermediate_ray_data,
                                                int num_intermediate_positions_save, double *source_moments) {
    if (!source_moments) {
        fprintf(stderr, "photon: photon_start_ray_tracing_moments: null source_moments; image left untouched\n");
        return 1;
    }
    return guarded("photon_start_ray_tracing_moments", [&]() -> int {
        const CallArgs a{lens_pitch, image_distance, scattering_data_p, scattering_type_str, lightfield_source_p,
                         lightray_number_per_particle, beam_wavelength, aperture_f_number, num_elements, element_center,
                         element_data_p, element_plane_parameters, element_system_index, camera_design_p,
                         simulate_density_gradients, density_grad_filename, save_lightrays, lightray_position_save_path,
                         lightray_direction_save_path, num_lightrays_save, ray_tracing_algorithm, add_pos_noise, pos_noise_std,
                         add_ngrad_noise, ngrad_noise_std, ray_cone_pitch_ratio, save_intermediate_ray_data,
                         num_intermediate_positions_save};
        return start_ray_tracing_impl(a, image_array, source_moments);
    });
}
