// piv_peak.hpp - what the window correlators (photon_piv.hip, photon_piv_phase.hip) share once the plane is in LDS: the
// flat-window write-out and the peak tail (argmax, second peak, edge flags, the three-point subpixel fit of section 5, the
// stores), the device form of piv_correlation.peak_outputs.  photon_dots.hip takes the fit alone.  DESIGN.md section 4.3k.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "block_reduce.hpp"

namespace photon {

// argmax with the tie rule: the larger value, then the smaller index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// block_reduce's order for a (value, index) pair.  blockDim.x is a multiple of 64; red / redi hold one word per wave.
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

// a flat window (block-uniform): NaN vector, NaN plane, flag 2
__device__ __forceinline__ void write_flat(int win_id, int nS2, bool outside, float *vectors, int *flags, float *planes) {
    const float qnan = __builtin_nanf("");
    if (threadIdx.x == 0) {
        vectors[4 * (size_t)win_id + 0] = qnan;
        vectors[4 * (size_t)win_id + 1] = qnan;
        vectors[4 * (size_t)win_id + 2] = qnan;
        vectors[4 * (size_t)win_id + 3] = qnan;
        flags[win_id] = 2 | (outside ? 4 : 0);
    }
    if (planes)
        for (int i = threadIdx.x; i < nS2; i += blockDim.x) planes[(size_t)win_id * nS2 + i] = qnan;
}

// From the unnormalised plane of nS x nS shifts to the window's outputs.  Two callables fetch a plane value: the first pass
// calls first(sy, sx) once per shift, from the thread that owns it, and first may compute and store (the direct correlator
// sums its partial planes there); every later read is at(sy, sx), from any thread, and only reads.  red and redi hold one
// word per wave.
template <typename First, typename At>
__device__ __forceinline__ void peak_tail(First first, At at, int nS, int R, int ox, int oy, double inv, bool outside, int win_id,
                                          float *vectors, int *flags, float *planes, float *red, int *redi) {
    const int tid = threadIdx.x, B = blockDim.x, nS2 = nS * nS;
    // ---- the plane's normalised copy, and the argmax
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < nS2; i += B) {
        const float c = first(i / nS, i % nS);
        if (planes) planes[(size_t)win_id * nS2 + i] = (float)((double)c * inv);
        if (better(c, i, bv, bi)) {
            bv = c;
            bi = i;
        }
    }
    block_argmax(bv, bi, red, redi);            // its barriers also publish what first() stored: at() below reads other threads' shifts
    const int py = bi / nS, px = bi % nS;

    // ---- the largest value at least 2 shifts away from the peak (Chebyshev distance)
    float m2 = -INFINITY;
    for (int i = tid; i < nS2; i += B) {
        const int sy = i / nS, sx = i % nS;
        if (max(abs(sy - py), abs(sx - px)) >= 2) m2 = fmaxf(m2, at(sy, sx));
    }
    m2 = block_reduce(m2, red, B >> 6, MaxF32());

    if (tid == 0) {
        int f = outside ? 4 : 0;
        double dx = 0.0, dy = 0.0;
        if (px == 0 || px == nS - 1) f |= 1;
        else dx = subpixel(at(py, px - 1), at(py, px), at(py, px + 1));
        if (py == 0 || py == nS - 1) f |= 1;
        else dy = subpixel(at(py - 1, px), at(py, px), at(py + 1, px));
        vectors[4 * (size_t)win_id + 0] = (float)((double)(ox + px - R) + dx);
        vectors[4 * (size_t)win_id + 1] = (float)((double)(oy + py - R) + dy);
        vectors[4 * (size_t)win_id + 2] = (float)((double)bv * inv);
        vectors[4 * (size_t)win_id + 3] = m2 > 0.f ? (float)((double)bv / (double)m2) : INFINITY;
        flags[win_id] = f;
    }
}

}  // namespace photon
