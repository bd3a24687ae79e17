// piv_direct.hpp - what the direct correlators share: photon_piv.hip (section 5, one image pair) and
// photon_piv_ensemble.hip (section 14, the sum over many pairs).  The plan (K row slices, threads, padded plane) and the
// tile loop that fills the partial planes in LDS.  Section 14 with one pair has to return section 5's bits, so both take
// the plan and every FMA of the correlation from here.  DESIGN.md sections 4.3b and 4.3m.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "block_reduce.hpp"

namespace photon {
namespace piv_direct {

constexpr int kTileX = 4;           // shifts per lane along x (one float4 of im2 per step)
constexpr int kTileY = 4;           // shifts per lane along y
constexpr int kMaxThreads = 512;
constexpr int kRedWords = 64;       // block-reduction scratch, 8 waves at most: 5 floats a wave, or a float a wave and (from word 32) an int a wave

static_assert(5 * (kMaxThreads / 64) <= kRedWords && 32 + kMaxThreads / 64 <= kRedWords, "the reduction scratch holds kRedWords words");

typedef float v4f __attribute__((ext_vector_type(4)));

// LDS layout (floats): a [WIN][WIN] | b [WIN + nSyp - 1][WIN + nSxp] | K partial planes [nSyp][nSxp] | reduction scratch.
// nSxp, nSyp: 2R + 1 rounded up to the tile; the shifts past 2R read zero padding and are dropped.

// How the shift tiles of one window are spread over a workgroup: K row slices and B threads (a multiple of 64), chosen
// to waste the fewest lane-rows (the lanes past the last item of a round idle) within the LDS the device allows.
struct Plan {
    int K, threads, nSxp, nSyp;
    size_t lds_bytes;
};

inline Plan plan_for(int win, int R, size_t lds_limit) {
    Plan best{0, 0, 0, 0, 0};
    const int nS = 2 * R + 1;
    const int nSxp = (nS + kTileX - 1) / kTileX * kTileX, nSyp = (nS + kTileY - 1) / kTileY * kTileY;
    const int units = (nSxp / kTileX) * (nSyp / kTileY);
    const size_t fixed = (size_t)win * win + (size_t)(win + nSyp - 1) * (win + nSxp) + kRedWords;
    long long best_cost = LLONG_MAX;
    for (int K = 1; K <= 8 && K <= win / 4; K++) {
        const size_t bytes = 4 * (fixed + (size_t)K * nSxp * nSyp);
        if (bytes > lds_limit) break;
        const int items = units * K;
        const int threads = std::min(kMaxThreads, (items + 63) / 64 * 64);
        const long long rounds = (items + threads - 1) / threads;
        const long long cost = rounds * threads * ((win + K - 1) / K);
        if (cost < best_cost) {
            best_cost = cost;
            best = Plan{K, threads, nSxp, nSyp, bytes};
        }
    }
    return best;
}

// The correlation of the staged window: item = (row slice k, shift tile ty, shift tile tx).  A lane sums its tile over its
// slice's rows from zero and stores it into partial plane k of sp (P floats apart).  ADD (section 14): where add_total is
// set, the lanes of slice 0 store what slice 0 holds + tile instead, in that order.
template <int WIN, bool ADD = false>
__device__ __forceinline__ void correlate_tiles(const float *sa, const float *sb, float *sp, int K, int P, int pitch, int nSxp, int nSyp,
                                                bool add_total = false) {
    const int tid = threadIdx.x, B = blockDim.x;
    const int ntx = nSxp / kTileX, nty = nSyp / kTileY, units = ntx * nty;
    for (int item = tid; item < units * K; item += B) {
        const int k = item / units, unit = item % units;
        const int sy0 = (unit / ntx) * kTileY, sx0 = (unit % ntx) * kTileX;
        const int y0 = (k * WIN) / K, y1 = ((k + 1) * WIN) / K;
        float acc[kTileY][kTileX];
#pragma unroll
        for (int u = 0; u < kTileY; u++)
#pragma unroll
            for (int t = 0; t < kTileX; t++) acc[u][t] = 0.f;
        for (int y = y0; y < y1; y++) {
            const float *arow = sa + y * WIN;
            const float *brow = sb + (y + sy0) * pitch + sx0;
            v4f prev[kTileY];
#pragma unroll
            for (int u = 0; u < kTileY; u++) prev[u] = *reinterpret_cast<const v4f *>(brow + u * pitch);
#pragma unroll
            for (int x = 0; x < WIN; x += 4) {
                const v4f av = *reinterpret_cast<const v4f *>(arow + x);
#pragma unroll
                for (int u = 0; u < kTileY; u++) {
                    const v4f nxt = *reinterpret_cast<const v4f *>(brow + u * pitch + x + 4);
                    const float s[8] = {prev[u].x, prev[u].y, prev[u].z, prev[u].w, nxt.x, nxt.y, nxt.z, nxt.w};
#pragma unroll
                    for (int t = 0; t < kTileX; t++) {
                        float c = acc[u][t];
                        c = fmaf(av.x, s[t + 0], c);
                        c = fmaf(av.y, s[t + 1], c);
                        c = fmaf(av.z, s[t + 2], c);
                        c = fmaf(av.w, s[t + 3], c);
                        acc[u][t] = c;
                    }
                    prev[u] = nxt;
                }
            }
        }
        float *out = sp + k * P + sy0 * nSxp + sx0;
#pragma unroll
        for (int u = 0; u < kTileY; u++) {
            v4f t = v4f{acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
            if (ADD && add_total && k == 0) t = *reinterpret_cast<const v4f *>(out + u * nSxp) + t;
            *reinterpret_cast<v4f *>(out + u * nSxp) = t;
        }
    }
}

}  // namespace piv_direct
}  // namespace photon
