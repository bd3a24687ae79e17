// photon_march_cubic.hip - the march kernels of the TRICUBIC B-spline sampler (the headline's): Euler and RK4, whole
// and segmented marches.  One translation unit per sampler: a kernel edit recompiles one unit.
#include "march_kernel.hpp"
#include "photon_internal.hpp"

namespace photon {

template int march_launch<2>(const MarchPlan &, hipStream_t, const MarchArgs &);     // and with it the tricubic march kernels

int march_rays_launch_cubic(int algorithm, const VolumeDev &vol, const f4 *tex, int n, float *pos, float *dir, int *steps) {
    const dim3 grid((n + 255) / 256), block(256);
    if (algorithm == 1) hipLaunchKernelGGL((march_rays_kernel<1, 2>), grid, block, 0, 0, vol, tex, n, pos, dir, steps);
    else hipLaunchKernelGGL((march_rays_kernel<2, 2>), grid, block, 0, 0, vol, tex, n, pos, dir, steps);
    PH_CHECK(hipGetLastError());
    return 0;
}

#if PHOTON_PATH_STATS
int march_path_slots() { return kPathSlots; }
int march_path_stats_cubic(unsigned long long *out) {    // debug builds only: read (and clear) this unit's sampler-path counters
    PH_CHECK(hipDeviceSynchronize());
    PH_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(photon::g_path_stats), kPathSlots * sizeof(unsigned long long)));
    unsigned long long zero[kPathSlots] = {};
    PH_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(photon::g_path_stats), zero, sizeof zero));
    return 0;
}
#endif

}  // namespace photon
