// photon_pool.hip - device memory of the library (photon_pool.hpp): a cache of freed device blocks, the allocation
// helper of every other hipMalloc site, the process-wide peer-access record.  Host code only.
//
// photon's unchanged Python builds everything anew for every start_ray_tracing call: per call ~25 hipMalloc / hipFree
// pairs, among them the ray-state workspace (320 MB for the 1e7-ray job) -- measured, the frees alone take 0.8-1.3 ms of a
// call (PHOTON_VERBOSE), 10 % of one GPU's eighth of the headline job, most of a small PIV frame.  Scene-lifetime blocks are
// therefore handed back to this cache instead of the runtime and the next call of the same shape takes them from it
// (exact size match, per device); the cache holds at most PHOTON_POOL_MAX_MB (default 4096; 0 = off), evicting its largest
// blocks first; photon_trim_caches() empties it, and so does any allocation of this library that finds the device out of
// memory (device_malloc).  Recycled memory is not zeroed -- neither is hipMalloc'd memory: every buffer that needs a
// defined start is cleared where it is allocated or used.  Held by tests/test_dirty_memory_gpu.py (solvers on recycled blocks).
#include "photon_pool.hpp"

#include "../../include/parallel_ray_tracing.h"

#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace photon {
namespace {

struct PoolKey {
    int device; size_t bytes;
    bool operator<(const PoolKey &o) const { return device != o.device ? device < o.device : bytes < o.bytes; }
};
struct DevicePool {
    std::mutex lock;
    std::multimap<PoolKey, void *> idle;        // ordered by (device, size): a device's largest block is the last of its run
    std::map<void *, PoolKey> live;
    std::map<void *, size_t> direct;            // blocks of device_malloc that are not the cache's, until device_free
    size_t idle_bytes = 0, live_bytes = 0, direct_bytes = 0;
};
DevicePool &device_pool() { static DevicePool *p = new DevicePool; return *p; }      // never destroyed: the runtime may be gone by then
size_t pool_cap_bytes() {
    static const size_t cap = [] { const char *e = getenv("PHOTON_POOL_MAX_MB"); return (size_t)(e ? strtoull(e, nullptr, 10) : 4096ull) << 20; }();
    return cap;
}

// the largest idle block of any device (caller holds the lock): the last entry of each device's run
std::multimap<PoolKey, void *>::iterator largest_idle(DevicePool &p) {
    auto best = p.idle.end();
    for (auto it = p.idle.begin(); it != p.idle.end();) {
        auto next = p.idle.upper_bound(PoolKey{it->first.device, (size_t)-1});      // first entry of the next device
        auto last = std::prev(next);
        if (best == p.idle.end() || last->first.bytes > best->first.bytes) best = last;
        it = next;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------
// failure injection (photon_selftest_fail_alloc): a REQUEST is one pool_malloc, or one device_malloc that does not come from
// pool_malloc.  Requests are numbered per process; those whose number lies in [fail_first, fail_last] fail.  Disarmed
// (fail_first = 0) a request pays the increment and one relaxed load.  All of it is atomics: it may be armed while the
// worker threads of a PHOTON_DEVICES call allocate.
// ---------------------------------------------------------------------------------------------
std::atomic<long long> g_requests{0}, g_injected{0}, g_retries{0}, g_retry_blocks{0};
std::atomic<long long> g_fail_first{0}, g_fail_last{0};
std::atomic<int> g_fail_first_attempt_only{0};

enum class Inject { none, whole_request, first_attempt };
Inject next_request() {
    const long long n = g_requests.fetch_add(1, std::memory_order_relaxed) + 1;
    const long long first = g_fail_first.load(std::memory_order_relaxed);
    if (first == 0 || n < first || n > g_fail_last.load(std::memory_order_relaxed)) return Inject::none;
    g_injected.fetch_add(1, std::memory_order_relaxed);
    return g_fail_first_attempt_only.load(std::memory_order_relaxed) ? Inject::first_attempt : Inject::whole_request;
}

size_t trim(size_t keep_bytes);

// hipMalloc, and once more after the cache has been emptied when the device is out of memory
hipError_t malloc_with_retry(void **out, size_t bytes, bool fail_first_attempt) {
    hipError_t e = fail_first_attempt ? hipErrorOutOfMemory : hipMalloc(out, bytes ? bytes : 1);
    if (e == hipErrorOutOfMemory) {
        if (!fail_first_attempt) (void)hipGetLastError();
        g_retries.fetch_add(1, std::memory_order_relaxed);
        g_retry_blocks.fetch_add((long long)trim(0), std::memory_order_relaxed);
        e = hipMalloc(out, bytes ? bytes : 1);
    }
    return e;
}

size_t trim(size_t keep_bytes) {                                 // caller holds no lock; returns the blocks handed back
    DevicePool &p = device_pool();
    std::vector<void *> victims;
    {
        std::lock_guard<std::mutex> g(p.lock);
        while (p.idle_bytes > keep_bytes && !p.idle.empty()) {
            auto big = largest_idle(p);
            p.idle_bytes -= big->first.bytes;
            victims.push_back(big->second);
            p.idle.erase(big);
        }
    }
    for (void *v : victims) (void)hipFree(v);                   // outside the lock: hipFree synchronises the device
    return victims.size();
}

}  // namespace

void pool_trim(size_t keep_bytes) { (void)trim(keep_bytes); }

hipError_t device_malloc(void **out, size_t bytes) {
    const Inject inject = next_request();
    if (inject == Inject::whole_request) { *out = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = malloc_with_retry(out, bytes, inject == Inject::first_attempt);
    if (e == hipSuccess) {
        DevicePool &p = device_pool();
        std::lock_guard<std::mutex> g(p.lock);
        p.direct[*out] = bytes ? bytes : 1;
        p.direct_bytes += bytes ? bytes : 1;
    }
    return e;
}

void device_free(void *ptr) {
    if (!ptr) return;
    {
        DevicePool &p = device_pool();
        std::lock_guard<std::mutex> g(p.lock);
        auto it = p.direct.find(ptr);
        if (it != p.direct.end()) { p.direct_bytes -= it->second; p.direct.erase(it); }
    }
    (void)hipFree(ptr);                                         // waits for the device by itself
}

hipError_t device_zero(void *p, size_t bytes) {
    if (!bytes) return hipSuccess;
    const hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

hipError_t pool_malloc(void **out, size_t bytes) {
    if (bytes == 0) bytes = 1;
    int device = 0;
    (void)hipGetDevice(&device);
    DevicePool &p = device_pool();
    const Inject inject = next_request();
    if (inject == Inject::whole_request) { *out = nullptr; return hipErrorOutOfMemory; }
    if (inject == Inject::none) {                               // first_attempt: past the cache, to the allocation that "fails"
        std::lock_guard<std::mutex> g(p.lock);
        auto it = p.idle.find(PoolKey{device, bytes});
        if (it != p.idle.end()) {
            *out = it->second;
            p.idle.erase(it);
            p.idle_bytes -= bytes;
            p.live[*out] = PoolKey{device, bytes};
            p.live_bytes += bytes;
            return hipSuccess;
        }
    }
    const hipError_t e = malloc_with_retry(out, bytes, inject == Inject::first_attempt);
    if (e == hipSuccess) { std::lock_guard<std::mutex> g(p.lock); p.live[*out] = PoolKey{device, bytes}; p.live_bytes += bytes; }
    return e;
}

void pool_free(void *ptr) {
    if (!ptr) return;
    DevicePool &p = device_pool();
    bool keep = false, over = false;
    {
        std::lock_guard<std::mutex> g(p.lock);
        auto it = p.live.find(ptr);
        if (it != p.live.end()) {
            const PoolKey k = it->second;
            p.live.erase(it);
            p.live_bytes -= k.bytes;
            if (k.bytes <= pool_cap_bytes()) { p.idle.emplace(k, ptr); p.idle_bytes += k.bytes; keep = true; }
        }
        over = p.idle_bytes > pool_cap_bytes();                 // decided under the lock
    }
    if (!keep) { (void)hipFree(ptr); return; }
    if (over) pool_trim(pool_cap_bytes());
}

// ---------------------------------------------------------------------------------------------
// peer access, once per ordered pair of devices and process
// ---------------------------------------------------------------------------------------------
bool peer_access(int dev, int peer) {
    static std::mutex lock;
    static std::map<std::pair<int, int>, bool> *known = new std::map<std::pair<int, int>, bool>;
    (void)hipSetDevice(dev);
    if (dev == peer) return true;
    std::lock_guard<std::mutex> g(lock);
    auto it = known->find({dev, peer});
    if (it != known->end()) return it->second;
    int can = 0;
    bool direct = false;
    const hipError_t ce = hipDeviceCanAccessPeer(&can, dev, peer);
    if (ce == hipSuccess && can) {
        const hipError_t pe = hipDeviceEnablePeerAccess(peer, 0);
        direct = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
        if (pe != hipSuccess) (void)hipGetLastError();
        // Kernels on `dev` will dereference pointers into `peer`'s memory.  The runtime maps what is allocated from now on;
        // blocks idling in the cache were allocated before.  Hand them back so that whatever a scene gets from here on is a
        // fresh allocation (once per pair and process).
        if (direct) pool_trim(0);
        if (!direct)
            fprintf(stderr, "photon: hipDeviceEnablePeerAccess(device %d from device %d) failed: %s; its accumulators are copied through host staging\n",
                    peer, dev, hipGetErrorString(pe));
    } else {
        if (ce != hipSuccess) (void)hipGetLastError();
        fprintf(stderr, "photon: device %d cannot access device %d as a peer (%s); its accumulators are copied through host staging\n", dev, peer,
                ce == hipSuccess ? "hipDeviceCanAccessPeer: no" : hipGetErrorString(ce));
    }
    (*known)[{dev, peer}] = direct;
    return direct;
}

}  // namespace photon

extern "C" void photon_trim_caches(void) { photon::pool_trim(0); }

extern "C" int photon_selftest_fail_alloc(long long first, long long count, int first_attempt_only) {
    using namespace photon;
    if (first < 0 || (first > 0 && count < 1)) {
        fprintf(stderr, "photon: photon_selftest_fail_alloc: bad arguments\n");
        return 1;
    }
    g_fail_first.store(0, std::memory_order_relaxed);           // disarmed while the range changes
    if (first == 0) return 0;
    const long long from = g_requests.load(std::memory_order_relaxed) + first;
    g_fail_last.store(count - 1 > LLONG_MAX - from ? LLONG_MAX : from + count - 1, std::memory_order_relaxed);
    g_fail_first_attempt_only.store(first_attempt_only != 0, std::memory_order_relaxed);
    g_fail_first.store(from, std::memory_order_relaxed);
    return 0;
}

extern "C" int photon_selftest_alloc_stats(photon_alloc_stats_t *out) {
    using namespace photon;
    if (!out) return 1;
    out->requests = g_requests.load(std::memory_order_relaxed);
    out->injected_failures = g_injected.load(std::memory_order_relaxed);
    out->oom_retries = g_retries.load(std::memory_order_relaxed);
    out->retry_blocks_returned = g_retry_blocks.load(std::memory_order_relaxed);
    DevicePool &p = device_pool();
    std::lock_guard<std::mutex> g(p.lock);
    out->idle_blocks = (long long)p.idle.size();
    out->idle_bytes = (long long)p.idle_bytes;
    out->outstanding_blocks = (long long)(p.live.size() + p.direct.size());
    out->outstanding_bytes = (long long)(p.live_bytes + p.direct_bytes);
    return 0;
}
