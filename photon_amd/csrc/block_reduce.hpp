// block_reduce.hpp - the fixed-order block reduction of the two window correlators (photon_piv.hip, photon_piv_phase.hip,
// the peak tail of piv_peak.hpp): the order contract below is stated once.  The uncertainty
// kernel and the solvers' fixed_sum.hpp keep reductions of their own with the same contract: through this one they
// measured outside the run-to-run spread of their timings.
#pragma once
#include <hip/hip_runtime.h>

namespace photon {

// the operators, by the exact functions the kernels' host models mirror
struct Sum {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct MaxF32 {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// Fixed-order reduction of N values per thread over the block: a butterfly inside each wave (partners 32, 16 .. 1; op is
// commutative, so every lane ends with the same bits), then the wave totals in wave order, starting from wave 0's total.
// Every thread returns with the block's values; each value's order is its own, so reducing values together or in
// separate calls gives the same bits.  Two barriers, whatever N.  blockDim.x == 64 n_waves; red holds N * n_waves values
// and may alias anything that is dead between the call's first barrier and the caller's next.
// n_waves is what the caller knows: with a constant the combine loop has a constant trip count after inlining.
// The scratch is value-major (value n's wave totals at red[n n_waves ..]) and the combine loop runs over the waves with
// the values inside, as the direct correlator's own reductions did: with a wave's values kept together that kernel's
// correlation loop is scheduled differently, and with a loop per value a block waits for N times as many LDS round trips,
// which showed at win 64 / R 32, where a CU holds one block.
// Starting from wave 0's total and not from zero matters for one input only: a total of -0 stays -0 (0 + -0 is +0).  The
// direct correlator once started its sums from 0.f; none of them can tell: its energies and counts are >= +0, and a pixel
// sum of -0 needs every pixel -0, a window the exact flatness test sends to the NaN path before the sum is used (and every
// thread's partial there starts from +0.f, so under round-to-nearest no wave total is -0 in the first place).
template <int N, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (&v)[N], T *red, int n_waves, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int n = 0; n < N; n++) v[n] = op(v[n], __shfl_xor(v[n], o, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int n = 0; n < N; n++) red[n * n_waves + w] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) v[n] = red[n * n_waves];
    for (int i = 1; i < n_waves; i++)           // the waves outside: one trip's N reads are in flight together
#pragma unroll
        for (int n = 0; n < N; n++) v[n] = op(v[n], red[n * n_waves + i]);
}

// one value
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *red, int n_waves, Op op) {
    T one[1] = {v};
    block_reduce(one, red, n_waves, op);
    return one[0];
}

}  // namespace photon
