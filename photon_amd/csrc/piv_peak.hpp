// piv_peak.hpp - what the window correlators (photon_piv.hip, photon_piv_phase.hip) share after the plane is in LDS: the
// block-wide maximum and argmax in a fixed order, and the three-point subpixel fit of section 5.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace photon {

// Fixed-order block reductions: a butterfly inside each wave (every lane ends with the same bits), then the wave totals in
// wave order.  blockDim.x is a multiple of 64; red / redi hold 16 words each.
__device__ __forceinline__ float block_max(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < nw; i++) v = fmaxf(v, red[i]);
    return v;
}

// argmax with the tie rule: the larger value, then the smaller index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ void block_argmax(float &bv, int &bi, float *red, int *redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = bv;
        redi[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    bv = red[0];
    bi = redi[0];
    for (int i = 1; i < nw; i++)
        if (better(red[i], redi[i], bv, bi)) {
            bv = red[i];
            bi = redi[i];
        }
}

// 3-point fit through (cm, c0, cp) in f64: Gaussian when all three are positive, parabolic otherwise; 0 for a flat triple
__device__ __forceinline__ double subpixel(double cm, double c0, double cp) {
    if (cm > 0.0 && c0 > 0.0 && cp > 0.0) {
        const double lm = log(cm), l0 = log(c0), lp = log(cp);
        const double den = 2.0 * (lm - 2.0 * l0 + lp);
        return den != 0.0 ? (lm - lp) / den : 0.0;
    }
    const double den = 2.0 * (cm - 2.0 * c0 + cp);
    return den != 0.0 ? (cm - cp) / den : 0.0;
}

}  // namespace photon
