// photon_moments.hip - per-source sensor moments (photon_trace_moments, photon_start_ray_tracing_moments): the reduction of a
// launch's moments block (written by sensor_kernel<..., MOM = true>, photon_sensor.hip) into one record of kMomentFields doubles per source.
//
// The summation order is part of the contract (include/parallel_ray_tracing.h): lane l of 64 adds, in increasing j, the values
// of the source's rays j = l (mod 64) that arrived, starting from +0.0; the 64 partials are then folded by halves
// (p[l] += p[l + off] for off = 32, 16, ..., 1) and p[0] is the record.  Every value is an f32 widened to f64 (exact), and
// x*x + y*y of two widened f32 rounds once whatever the compiler contracts, so a record has the same bits whatever the ray
// order, culls, segments or launch boundaries of the trace -- and photon_amd/deflections.py reproduces it on the host.
//
// A source of at most 32 rays is reduced by a group of G = its ray count rounded up to a power of two lanes (64 / G sources
// per wave): the missing lanes' partials would be +0.0, and a partial that starts at +0.0 is never -0.0, so adding them
// changes no bit.
#include "photon_internal.hpp"

using namespace photon;

// One group of G lanes per place of the launch; the block is [place][rps], so the lanes of a group read consecutive floats.
template <int G>
__global__ __launch_bounds__(256) void moments_kernel(MomentsDev m, unsigned places, unsigned rps, long long src_begin,
                                                      const int *__restrict__ src_list, double *__restrict__ records) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned lane = (unsigned)(t % G);
    const size_t place = t / G;
    if (place >= places) return;                                        // whole groups only: G divides the block size
    double p[kMomentFields];
#pragma unroll
    for (int f = 0; f < kMomentFields; f++) p[f] = 0.0;
    const size_t base = place * rps;
    for (unsigned j = lane; j < rps; j += G) {
        const float x = m.x[base + j];
        if (isnan(x)) continue;                                         // did not reach the sensor: adds nothing
        const double X = x, Y = m.y[base + j], Z = m.z[base + j];
        const double r2 = X * X + Y * Y;                                // both squares exact in f64: one rounding
        p[0] += 1.0;
        p[1] += X; p[2] += Y; p[3] += Z;
        p[4] += acos((double)m.dx[base + j]);
        p[5] += acos((double)m.dy[base + j]);
        p[6] += acos((double)m.dz[base + j]);
        p[7] += r2;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int f = 0; f < kMomentFields; f++) p[f] += __shfl_down(p[f], off, G);
    }
    if (lane == 0) {
        const long long src = src_list ? (long long)src_list[place] : src_begin + (long long)place;
        double *out = records + (size_t)src * kMomentFields;
#pragma unroll
        for (int f = 0; f < kMomentFields; f++) out[f] = p[f];
    }
}

namespace photon {

int launch_moments(const MomentsDev &mom, unsigned places, unsigned rps, long long src_begin, const int *src_list,
                   double *records, hipStream_t stream) {
    if (places == 0) return 0;
    const dim3 block(256);
    auto grid = [&](int g) { return dim3((unsigned)(((size_t)places * g + 255) / 256)); };
#define PH_MOMENTS(G) hipLaunchKernelGGL(moments_kernel<G>, grid(G), block, 0, stream, mom, places, rps, src_begin, src_list, records)
    if (rps > 32) PH_MOMENTS(64);
    else if (rps > 16) PH_MOMENTS(32);
    else if (rps > 8) PH_MOMENTS(16);
    else if (rps > 4) PH_MOMENTS(8);
    else if (rps > 2) PH_MOMENTS(4);
    else if (rps > 1) PH_MOMENTS(2);
    else PH_MOMENTS(1);
#undef PH_MOMENTS
    PH_CHECK(hipGetLastError());
    return 0;
}

int clear_records(double *d_records, long long src_begin, long long src_end, hipStream_t stream) {
    if (src_end > src_begin)
        PH_CHECK(hipMemsetAsync(d_records + (size_t)src_begin * kMomentFields, 0,
                                (size_t)(src_end - src_begin) * kMomentFields * sizeof(double), stream));
    return 0;
}

}  // namespace photon
