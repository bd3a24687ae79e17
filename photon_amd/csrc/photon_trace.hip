// photon_trace.hip - the launch loop of a trace (the reference's chunk loop, parallel_ray_tracing.cu:3505-3558, on
// inputs resident in HBM): one launch as its plan says (photon_cull.hip), raygen -> march -> sensor stage, photon_trace and
// the statistics window.  Host code only: every kernel is launched through the unit that defines it.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "photon_internal.hpp"

using namespace photon;

// Spatial order of the sources for lens-major launches: Morton code of (x, y) on a 2^16 grid over the bounding
// box of the LAUNCHED range [src_begin, src_end), sorted on the device (photon_sort.hip) -- start_ray_tracing
// builds a new scene per call, so this sits on the per-image path of every PIV-through-volume frame (1e6 sources:
// a host sort cost a D2H of the coordinates, ~0.1 s of std::stable_sort and an H2D per call).  The permutation
// covers exactly the launched range, so [src_begin, src_end) always counts sources in the CALLER's order,
// whatever order the lanes then use; it is kept for the next launch of the same range.

// The permutation of a launched range is kept (a few ranges: a job's chunks, a caller alternating shards), and the sort's
// scratch lives in the scene: a lens-major launch of a range seen before costs nothing, a new range costs the sort's
// kernels on the stream -- no allocation, no host wait, so photon_trace without stats stays asynchronous.
// The slot of the range, with room for it: its own when the range was seen before, else the least recently used one, marked
// empty (begin < 0) until sort_sources has filled it.
static int source_order_slot(photon_scene *s, long long src_begin, long long src_end, PermEntry **out) {
    const size_t n = (size_t)(src_end - src_begin);
    s->perm_clock++;
    PermEntry *slot = nullptr;
    for (auto &p : s->perms)
        if (p.perm.p && p.begin == src_begin && p.end == src_end) { p.stamp = s->perm_clock; *out = &p; return 0; }
    for (auto &p : s->perms)                                            // least recently used (an empty one first)
        if (!slot || (!p.perm.p && slot->perm.p) || (!!p.perm.p == !!slot->perm.p && p.stamp < slot->stamp)) slot = &p;
    slot->begin = slot->end = -1;
    PH_TRY(scene_reserve(s, slot->perm, n));                            // an earlier launch may still read the old one
    *out = slot;
    return 0;
}
static int sort_sources(photon_scene *s, PermEntry *slot, long long src_begin, long long src_end, hipStream_t stream) {
    PH_TRY(photon_morton_order(s->dev.sx, s->dev.sy, (int)src_begin, src_end - src_begin, slot->perm.p, stream, &s->sort_scratch));
    slot->begin = src_begin; slot->end = src_end; slot->stamp = s->perm_clock;
    return 0;
}

// Room for the moments block of a launch of `places` sources: six planes of places x rays_per_source floats (grown on demand).
// places x rays_per_source <= kMaxRaysPerLaunch (make_trace_plan caps the sources of a launch by it), so the block stays below
// 24 B x kMaxRaysPerLaunch = 1.5 GiB.
static int moments_block(photon_scene *s, size_t rays, MomentsDev *out) {
    if (rays > kMaxRaysPerLaunch) {
        fprintf(stderr, "photon: a moments block of %zu rays exceeds the %u-ray limit per launch\n", rays, kMaxRaysPerLaunch);
        return 1;
    }
    PH_TRY(scene_reserve(s, s->mom, rays * 6));                         // an earlier launch may still use the old one
    float *f = s->mom.p;
    const size_t stride = s->mom.n / 6;
    *out = MomentsDev{f, f + stride, f + 2 * stride, f + 3 * stride, f + 4 * stride, f + 5 * stride};
    return 0;
}

namespace photon {

int begin_accumulate(photon_scene *s, hipStream_t stream) {
    const size_t npix = (size_t)s->dev.cam.x_pixel_number * s->dev.cam.y_pixel_number;
    s->launched = true;                                     // the fill and, later, the finalize kernel use d_acc even when no source is traced
    if (!s->acc_clean) PH_CHECK(hipMemsetAsync(s->acc.p, 0, npix * sizeof(double), stream));      // else: left zeroed by the last finalize
    s->acc_clean = false;
    return 0;
}

int launch_chunk(photon_scene *s, const photon_volume *vol, int algorithm, const TracePlan &plan, const LaunchRange &range, DumpDev dump,
                 hipStream_t stream, hipEvent_t ev_march_begin, hipEvent_t ev_march_end, double *d_records) {
    const long long src_begin = range.begin, src_end = range.end;
    const unsigned long long n64 = (unsigned long long)range.n_sources * (unsigned)plan.slot_rays;
    if (n64 == 0) return 0;
    if (n64 > kMaxRaysPerLaunch) {
        fprintf(stderr, "photon: a launch of %llu rays (sources [%lld, %lld) x %d) exceeds the %u-ray limit per launch\n", n64,
                src_begin, src_end, s->dev.rays_per_source, kMaxRaysPerLaunch);
        return 1;
    }
    const unsigned n = (unsigned)n64, places = (unsigned)range.n_sources;
    // Room first: whatever has to grow waits for the scene's earlier launches (scene_quiesce, which clears `launched`) ...
    const size_t mom_rays = (size_t)places * (unsigned)s->dev.rays_per_source;
    MomentsDev mom{};
    PermEntry *order = nullptr;
    if (d_records) PH_TRY(moments_block(s, mom_rays, &mom));
    if (plan.lens_major) PH_TRY(source_order_slot(s, src_begin, src_end, &order));
    MarchPlan march{};
    if (vol) {
        march = plan_march(n, s->num_cus, vol->dev, algorithm, dump.inter_pos != nullptr, s->dev.noise.add_ngrad != 0, order ? 1 : 0, false, plan.march);
        PH_TRY(ensure_workspace(s, n));
        if (march.segmented) PH_TRY(ensure_resume_state(s, march.interp == 1));
    }
    // ... then the launch: from here on kernels of this scene may be in flight
    s->launched = true;
    if (d_records) PH_CHECK(hipMemsetAsync(mom.x, 0xFF, mom_rays * sizeof(float), stream));       // all-ones = NaN: "did not arrive"
    if (order && order->begin < 0) PH_TRY(sort_sources(s, order, src_begin, src_end, stream));
    SceneDev dev = s->dev;                                      // the scene as this launch sees it
    dev.slot_rays = plan.slot_rays;
    dev.slot_map = plan.live_samples_only ? s->d_live : nullptr;
    dev.src_list = range.src_list;
    dev.doom_margin = plan.doom_margin;
    dev.ray_order = order ? 1 : 0;
    dev.src_perm = order ? order->perm.p : nullptr;
    const MomentsDev *mom_p = d_records ? &mom : nullptr;
    if (vol) {
        // ray generation: the prologue of the march's first piece for Euler and RK4, a kernel of its own for the others
        if (!march.fold) PH_TRY(launch_raygen(s, dev, src_begin, n, stream));
        const unsigned long long ray_base = (unsigned long long)(dev.source_base + src_begin) * (unsigned)dev.rays_per_source;
        const InterDump idump{dump.inter_pos, dump.inter_dir, dump.inter_slots, dump.num_save, 0u};
        PH_TRY(launch_march(s, dev, vol, march, ray_base, idump, src_begin, stream, ev_march_begin));
        if (ev_march_end) PH_CHECK(hipEventRecord(ev_march_end, stream));
    }
    PH_TRY(launch_sensor(s, dev, vol != nullptr, src_begin, n, dump, stream, mom_p));
    if (!d_records) return 0;
    return launch_moments(mom, places, (unsigned)dev.rays_per_source, src_begin, dev.src_list, d_records, stream);
}

}  // namespace photon

constexpr unsigned kWindowMaxTraces = 1u << 16;        // traces per statistics window (each keeps a few HIP events alive)

// An event of the open statistics window (created on first use, kept for the next window).
static int window_event(photon_scene *s, size_t *index_out) {
    if (s->win_used == s->win_events.size()) {
        Event e;
        PH_CHECK(e.create());
        s->win_events.push_back(std::move(e));
    }
    *index_out = s->win_used++;
    return 0;
}

namespace photon {

// The launch loop for sources [src_begin, src_end) into the scene's private f64 accumulator (zeroed first); the
// caller folds the accumulator into an image (end_accumulate) -- or, when several devices share one call, sums the
// accumulators first.  timed: 0 no events; 1 immediate (the march of every launch is timed with ev[1], ev[2] and the host
// waits for it: photon_trace with a stats pointer); 2 deferred (events of the open statistics window, no host wait).
int trace_accumulate(photon_scene *scene, const photon_volume *vol, int ray_tracing_algorithm, long long src_begin,
                            long long src_end, hipStream_t stream, int timed, float *march_ms_out, double *d_records) {
    const unsigned rps = (unsigned)scene->dev.rays_per_source;
    if (rps > kMaxRaysPerLaunch) { fprintf(stderr, "photon: too many rays per source\n"); return 1; }
    float march_ms = 0.f;
    const DumpDev no_dump{nullptr, nullptr, 0, nullptr, nullptr, 0};
    const TracePlan plan = make_trace_plan(scene, vol, ray_tracing_algorithm, false, d_records != nullptr);
    PH_TRY(begin_accumulate(scene, stream));
    if (d_records) PH_TRY(clear_records(d_records, src_begin, src_end, stream));
    for (long long b = src_begin; b < src_end;) {
        const LaunchRange r = next_launch(scene, plan, b, src_end);
        b = r.end;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed == 1 && vol) { e0 = scene->ev[1]; e1 = scene->ev[2]; }
        size_t i0 = 0, i1 = 0;
        if (timed == 2 && vol) {
            PH_TRY(window_event(scene, &i0));
            PH_TRY(window_event(scene, &i1));
            e0 = scene->win_events[i0]; e1 = scene->win_events[i1];
        }
        PH_TRY(launch_chunk(scene, vol, ray_tracing_algorithm, plan, r, no_dump, stream, e0, e1, d_records));
        if (timed == 2 && vol) scene->win_march.emplace_back(i0, i1);      // only pairs whose events were recorded
        if (timed == 1 && vol) {
            PH_CHECK(hipEventSynchronize(scene->ev[2]));
            float ms = 0.f;
            PH_CHECK(hipEventElapsedTime(&ms, scene->ev[1], scene->ev[2]));
            march_ms += ms;
        }
    }
    if (march_ms_out) *march_ms_out = march_ms;
    return 0;
}

}  // namespace photon

// Sum the counter slots into stats (the caller has made sure the device is done with them).
static int read_counters(photon_scene *scene, bool have_volume, photon_trace_stats_t *stats) {
    std::vector<unsigned long long> slots((size_t)kCounterSlots * kCounterStride);
    PH_CHECK(hipMemcpy(slots.data(), scene->d_counters, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long c[CNT_N] = {};
    for (int k = 0; k < kCounterSlots; k++)
        for (int j = 0; j < CNT_N; j++) c[j] += slots[(size_t)k * kCounterStride + j];
    PH_TRY(march_error_check(scene));
    stats->rays_on_sensor = c[CNT_ON_SENSOR];
    stats->rk_iterations = c[CNT_ITER];
    stats->volume_samples = c[CNT_SAMPLES];
    stats->sensor_taps = c[CNT_TAPS];
    stats->rays_marched = have_volume ? c[CNT_MARCHED] : 0;
    // s_memtime ticks per s_memrealtime tick (100 MHz), over all waves of the march: the clock the kernel ran at
    stats->shader_clock_mhz = c[CNT_REAL] ? (float)((double)c[CNT_CLK] / (double)c[CNT_REAL] * 100.0) : 0.f;
    // mean time a wave spends on one 64-ray group: with 5 waves per SIMD a launch lasts about (groups / 5120) of these
    stats->march_wave_ms = c[CNT_MARCHED] ? (float)((double)c[CNT_REAL] * 1e-5 / ((double)(c[CNT_MARCHED] + 63) / 64.0)) : 0.f;
    return 0;
}

// photon_trace and photon_trace_moments (d_records != nullptr)
static int trace_call(photon_scene_t *scene, const photon_volume_t *vol, int ray_tracing_algorithm, int64_t src_begin, int64_t src_end,
                      float *d_image, void *stream_p, photon_trace_stats_t *stats, double *d_records) {
    if (stats && scene->win_open) {
        fprintf(stderr, "photon: photon_trace: per-call stats inside an open statistics window (photon_scene_stats_begin); "
                        "pass stats = NULL and read them with photon_scene_stats_end\n");
        return 1;
    }
    if (scene->win_open && (hipStream_t)stream_p != scene->win_stream) {
        fprintf(stderr, "photon: photon_trace: a statistics window is open on another stream (its counters were zeroed there)\n");
        return 1;
    }
    if (scene->win_open && scene->win_traces >= kWindowMaxTraces) {
        fprintf(stderr, "photon: photon_trace: more than %u traces in one statistics window; close it with photon_scene_stats_end\n", kWindowMaxTraces);
        return 1;
    }
    return guarded(d_records ? "photon_trace_moments" : "photon_trace", [&]() -> int {
        photon::DeviceScope on_scene_device(scene->device);
        hipStream_t stream = (hipStream_t)stream_p;
        const unsigned rps = (unsigned)scene->dev.rays_per_source;
        size_t w0 = 0, w1 = 0;
        if (stats) {
            PH_CHECK(hipMemsetAsync(scene->d_counters, 0, kCounterBytes, stream));
            PH_TRY(profile_reset(scene, stream));
            PH_CHECK(hipEventRecord(scene->ev[0], stream));
        } else if (scene->win_open) {
            PH_TRY(window_event(scene, &w0));
            PH_TRY(window_event(scene, &w1));
            PH_CHECK(hipEventRecord(scene->win_events[w0], stream));
        }
        float march_ms = 0.f;
        const int timed = stats ? 1 : (scene->win_open ? 2 : 0);
        PH_TRY(trace_accumulate(scene, vol, ray_tracing_algorithm, src_begin, src_end, stream, timed, &march_ms, d_records));
        PH_TRY(launch_finalize(scene, d_image, stream));
        if (stats) {
            PH_CHECK(hipEventRecord(scene->ev[3], stream));
            PH_CHECK(hipEventSynchronize(scene->ev[3]));
            memset(stats, 0, sizeof *stats);
            PH_TRY(read_counters(scene, vol != nullptr, stats));
            stats->rays_launched = (uint64_t)(src_end - src_begin) * rps;
            stats->march_ms = march_ms;
            stats->traces = 1;
            PH_CHECK(hipEventElapsedTime(&stats->total_ms, scene->ev[0], scene->ev[3]));
        } else if (scene->win_open) {
            PH_CHECK(hipEventRecord(scene->win_events[w1], stream));
            scene->win_total.emplace_back(w0, w1);
            scene->win_rays += (uint64_t)(src_end - src_begin) * rps;
            scene->win_traces += 1;
            scene->win_have_volume = scene->win_have_volume || vol != nullptr;
        }
        return 0;
    });
}

extern "C" int photon_trace(photon_scene_t *scene, const photon_volume_t *vol, int ray_tracing_algorithm,
                            int64_t src_begin, int64_t src_end, float *d_image, void *stream_p,
                            photon_trace_stats_t *stats) {
    if (!scene || !d_image || src_begin < 0 || src_end < src_begin || src_end > scene->dev.num_sources) {
        fprintf(stderr, "photon: photon_trace: bad arguments (sources [%lld,%lld) of %d)\n", (long long)src_begin,
                (long long)src_end, scene ? scene->dev.num_sources : -1);
        return 1;
    }
    return trace_call(scene, vol, ray_tracing_algorithm, src_begin, src_end, d_image, stream_p, stats, nullptr);
}

extern "C" int photon_trace_moments(photon_scene_t *scene, const photon_volume_t *vol, int ray_tracing_algorithm, int64_t src_begin,
                                    int64_t src_end, float *d_image, double *d_records, void *stream_p) {
    if (!scene || !d_image || !d_records || src_begin < 0 || src_end < src_begin || src_end > scene->dev.num_sources) {
        fprintf(stderr, "photon: photon_trace_moments: bad arguments (sources [%lld,%lld) of %d, records %p)\n", (long long)src_begin,
                (long long)src_end, scene ? scene->dev.num_sources : -1, (void *)d_records);
        return 1;
    }
    return trace_call(scene, vol, ray_tracing_algorithm, src_begin, src_end, d_image, stream_p, nullptr, d_records);
}

// Statistics over a WINDOW of photon_trace calls without a host synchronisation inside it: _begin zeroes the counters (on
// the stream), every photon_trace(stats = NULL) of this scene up to _end records its events on its stream and lets the
// counters run; _end waits for the stream and returns the sums (march_ms, total_ms: summed over the traces; counters:
// summed over the traces; shader_clock_mhz: over all march waves of the window).
extern "C" int photon_scene_stats_begin(photon_scene_t *scene, void *stream_p) {
    if (!scene) return 1;
    return guarded("photon_scene_stats_begin", [&]() -> int {
        photon::DeviceScope on_scene_device(scene->device);
        hipStream_t stream = (hipStream_t)stream_p;
        PH_CHECK(hipMemsetAsync(scene->d_counters, 0, kCounterBytes, stream));
        PH_TRY(profile_reset(scene, stream));
        scene->win_used = 0;
        scene->win_march.clear();
        scene->win_total.clear();
        scene->win_rays = 0;
        scene->win_traces = 0;
        scene->win_have_volume = false;
        scene->win_stream = stream;
        scene->win_open = true;
        return 0;
    });
}

extern "C" int photon_scene_check(photon_scene_t *scene, void *stream_p) {
    if (!scene) return 1;
    PH_CHECK(hipStreamSynchronize((hipStream_t)stream_p));
    return march_error_check(scene);
}

extern "C" int photon_scene_stats_end(photon_scene_t *scene, void *stream_p, photon_trace_stats_t *stats) {
    if (!scene || !stats || !scene->win_open) {
        fprintf(stderr, "photon: photon_scene_stats_end: no open statistics window\n");
        return 1;
    }
    return guarded("photon_scene_stats_end", [&]() -> int {
        photon::DeviceScope on_scene_device(scene->device);
        scene->win_open = false;
        PH_CHECK(hipStreamSynchronize((hipStream_t)stream_p));
        memset(stats, 0, sizeof *stats);
        PH_TRY(read_counters(scene, scene->win_have_volume, stats));
        double march = 0.0, total = 0.0;
        for (const auto &pr : scene->win_march) {
            float ms = 0.f;
            PH_CHECK(hipEventElapsedTime(&ms, scene->win_events[pr.first], scene->win_events[pr.second]));
            march += ms;
        }
        for (const auto &pr : scene->win_total) {
            float ms = 0.f;
            PH_CHECK(hipEventElapsedTime(&ms, scene->win_events[pr.first], scene->win_events[pr.second]));
            total += ms;
        }
        stats->march_ms = (float)march;
        stats->total_ms = (float)total;
        stats->rays_launched = scene->win_rays;
        stats->traces = scene->win_traces;
        return 0;
    });
}
