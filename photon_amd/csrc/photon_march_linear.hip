// photon_march_linear.hip - the march kernels of the TRILINEAR sampler (the one the reference executes,
// parallel_ray_tracing.cu:3330): Euler and RK4, with and without intermediate dumps, gradient noise, segments.
// One translation unit per sampler: a kernel edit recompiles one unit.
#include "march_kernel.hpp"
#include "photon_internal.hpp"

namespace photon {

template int march_launch<1>(const MarchPlan &, hipStream_t, const MarchArgs &);     // and with it the trilinear march kernels

int march_rays_launch_linear(int algorithm, const VolumeDev &vol, const f4 *tex, int n, float *pos, float *dir, int *steps) {
    const dim3 grid((n + 255) / 256), block(256);
    if (algorithm == 1) hipLaunchKernelGGL((march_rays_kernel<1, 1>), grid, block, 0, 0, vol, tex, n, pos, dir, steps);
    else hipLaunchKernelGGL((march_rays_kernel<2, 1>), grid, block, 0, 0, vol, tex, n, pos, dir, steps);
    PH_CHECK(hipGetLastError());
    return 0;
}

#if PHOTON_PATH_STATS
int march_path_stats_linear(unsigned long long *out) {    // debug builds only: read (and clear) this unit's sampler-path counters
    PH_CHECK(hipDeviceSynchronize());
    PH_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(photon::g_path_stats), kPathSlots * sizeof(unsigned long long)));
    unsigned long long zero[kPathSlots] = {};
    PH_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(photon::g_path_stats), zero, sizeof zero));
    return 0;
}
#endif

}  // namespace photon
