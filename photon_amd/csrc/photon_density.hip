// photon_density.hip - weighted least-squares integration of a gradient field on the device (BOS: the measured
// displacements -> projected density).  Definition: include/parallel_ray_tracing.h, section 6; host model:
// photon_amd/bos_density.py (integrate_model, the same iteration in numpy).
//
// One assembly kernel writes the edge weights, the diagonal, the right-hand side and a byte per node (live-edge and fixed
// bits).  The host copies the bytes down, runs a BFS from the fixed nodes (O(N), no device loop of unbounded length) and
// uploads them again with the solve bit set.  Jacobi-preconditioned CG then runs two plain stream launches per iteration:
//   pcg_direction: p = z + beta p_old (neighbours' p formed from z and p_old the same way), q = A p, partials of p.q
//   pcg_update:    x += alpha p, r -= alpha q, z = r / diag, partials of r.z and r.r
// alpha and beta never leave the device: every block sums the same partial arrays in the same order (a fixed grid of at
// most kMaxBlocks blocks, grid-stride over the nodes), so every block holds the same bits and no further launch is
// needed.  The host reads one f64 (||r||^2, summed by a one-block kernel) every PHOTON_INTEGRATE_CHECK_EVERY iterations.
// Every sum has a fixed order that depends on the grid size alone: two calls on the same inputs return the same bits.
// Bytes per node and iteration: pcg_direction reads z, p_old, diag, wh, wv (+ the byte) and writes p, q; pcg_update reads
// x, p, r, q, diag and writes x, r, z: 15 f64 -- 120 MB per iteration at 1024^2.
#include <climits>
#include <cmath>
#include <vector>

#include "fixed_sum.hpp"
#include "photon_internal.hpp"

using namespace photon;

namespace {

constexpr unsigned char kEdgeE = 1;          // live edge (i,j)->(i,j+1)
constexpr unsigned char kEdgeS = 2;          // live edge (i,j)->(i+1,j)
constexpr unsigned char kEdgeW = 4;          // live edge (i,j-1)->(i,j)
constexpr unsigned char kEdgeN = 8;          // live edge (i-1,j)->(i,j)
constexpr unsigned char kFixed = 16;
constexpr unsigned char kSolve = 32;         // set by the host: a reachable unknown node

struct Inputs {
    const double *gx, *gy, *w;
    const unsigned char *fixed;
    const double *value;
    int nx, ny;
};

__device__ __forceinline__ bool node_valid(const Inputs &in, unsigned k) {
    const double a = in.gx[k], b = in.gy[k], c = in.w ? in.w[k] : 1.0;
    return isfinite(a) && isfinite(b) && isfinite(c) && c > 0.0;
}
__device__ __forceinline__ bool node_fixed(const Inputs &in, unsigned k, int i, int j) {
    return in.fixed ? in.fixed[k] != 0 : (i == 0 || j == 0 || i == in.ny - 1 || j == in.nx - 1);
}
__device__ __forceinline__ double node_value(const Inputs &in, unsigned k) { return in.value ? in.value[k] : 0.0; }

// weight of the edge between nodes a and b (both in the grid)
__device__ __forceinline__ double edge_weight(const Inputs &in, unsigned a, int ia, int ja, unsigned b, int ib, int jb) {
    if (!node_valid(in, a) || !node_valid(in, b)) return 0.0;
    if (node_fixed(in, a, ia, ja) && !isfinite(node_value(in, a))) return 0.0;
    if (node_fixed(in, b, ib, jb) && !isfinite(node_value(in, b))) return 0.0;
    return in.w ? fmin(in.w[a], in.w[b]) : 1.0;
}

// Per node: the east and south edge weights, the diagonal and the right-hand side (the 4 incident edges in the order
// W, E, N, S; a fixed neighbour adds w * value), and the byte of live-edge and fixed bits.
__global__ __launch_bounds__(kThreads) void assemble_kernel(Inputs in, double hx, double hy, double *__restrict__ wh,
                                                            double *__restrict__ wv, double *__restrict__ diag,
                                                            double *__restrict__ rhs, unsigned char *__restrict__ mask) {
    const unsigned N = (unsigned)in.nx * (unsigned)in.ny, nx = (unsigned)in.nx;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        const int i = (int)(k / nx), j = (int)(k - (unsigned)i * nx);
        const bool fixed = node_fixed(in, k, i, j);
        double d = 0.0, b = 0.0, e = 0.0, s = 0.0;
        unsigned char m = fixed ? kFixed : 0;
        if (j > 0) {                                            // W: (i,j-1)->(i,j), this node is the b end
            const double we = edge_weight(in, k - 1, i, j - 1, k, i, j);
            if (we > 0.0) {
                const double t = hx * ((in.gx[k - 1] + in.gx[k]) * 0.5);
                d += we;
                b += we * t;
                if (node_fixed(in, k - 1, i, j - 1)) b += we * node_value(in, k - 1);
                m |= kEdgeW;
            }
        }
        if (j < in.nx - 1) {                                    // E: (i,j)->(i,j+1), this node is the a end
            e = edge_weight(in, k, i, j, k + 1, i, j + 1);
            if (e > 0.0) {
                const double t = hx * ((in.gx[k] + in.gx[k + 1]) * 0.5);
                d += e;
                b -= e * t;
                if (node_fixed(in, k + 1, i, j + 1)) b += e * node_value(in, k + 1);
                m |= kEdgeE;
            }
        }
        if (i > 0) {                                            // N: (i-1,j)->(i,j)
            const double we = edge_weight(in, k - nx, i - 1, j, k, i, j);
            if (we > 0.0) {
                const double t = hy * ((in.gy[k - nx] + in.gy[k]) * 0.5);
                d += we;
                b += we * t;
                if (node_fixed(in, k - nx, i - 1, j)) b += we * node_value(in, k - nx);
                m |= kEdgeN;
            }
        }
        if (i < in.ny - 1) {                                    // S: (i,j)->(i+1,j)
            s = edge_weight(in, k, i, j, k + nx, i + 1, j);
            if (s > 0.0) {
                const double t = hy * ((in.gy[k] + in.gy[k + nx]) * 0.5);
                d += s;
                b -= s * t;
                if (node_fixed(in, k + nx, i + 1, j)) b += s * node_value(in, k + nx);
                m |= kEdgeS;
            }
        }
        wh[k] = e;
        wv[k] = s;
        diag[k] = d;
        rhs[k] = b;
        mask[k] = m;
    }
}

// x = 0, r = b on the solved nodes (0 elsewhere), z = r / diag, p (both buffers) = q = 0; partials of r.z and r.r
__global__ __launch_bounds__(kThreads) void pcg_init_kernel(unsigned N, const unsigned char *__restrict__ mask,
                                                            const double *__restrict__ diag, double *__restrict__ x,
                                                            double *__restrict__ r, double *__restrict__ z,
                                                            double *__restrict__ p0, double *__restrict__ p1, double *__restrict__ q,
                                                            double *__restrict__ rz_part, double *__restrict__ rr_part) {
    __shared__ double red[kThreads / 64];
    double rz = 0.0, rr = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        double rk = 0.0, zk = 0.0;
        if (mask[k] & kSolve) {
            rk = r[k];
            zk = rk / diag[k];
            rz += rk * zk;
            rr += rk * rk;
        }
        x[k] = 0.0;
        r[k] = rk;
        z[k] = zk;
        p0[k] = 0.0;
        p1[k] = 0.0;
        q[k] = 0.0;
    }
    rz = block_sum(rz, red);
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) {
        rz_part[blockIdx.x] = rz;
        rr_part[blockIdx.x] = rr;
    }
}

// Launch 1 of an iteration: beta = (r.z) / (r.z)_old (0 on the first iteration, or when the old value is 0), p = z + beta
// p_old, q = A p.  p is 0 off the solved nodes (z and p_old are), so a fixed neighbour adds nothing to q.
__global__ __launch_bounds__(kThreads) void pcg_direction_kernel(unsigned N, int nx, const unsigned char *__restrict__ mask,
                                                                 const double *__restrict__ z, const double *__restrict__ p_old,
                                                                 double *__restrict__ p, double *__restrict__ q,
                                                                 const double *__restrict__ diag, const double *__restrict__ wh,
                                                                 const double *__restrict__ wv, const double *__restrict__ rz_cur,
                                                                 const double *__restrict__ rz_old, int n_parts, int first,
                                                                 double *__restrict__ pq_part) {
    __shared__ double red[kThreads / 64];
    double beta = 0.0;
    if (!first) {
        const double a = sum_parts(rz_cur, n_parts, red), b = sum_parts(rz_old, n_parts, red);
        beta = b != 0.0 ? a / b : 0.0;
    }
    const unsigned unx = (unsigned)nx;
    double pq = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        const unsigned char m = mask[k];
        if (!(m & kSolve)) continue;
        const double pk = z[k] + beta * p_old[k];
        double qk = diag[k] * pk;
        if (m & kEdgeW) qk -= wh[k - 1] * (z[k - 1] + beta * p_old[k - 1]);
        if (m & kEdgeE) qk -= wh[k] * (z[k + 1] + beta * p_old[k + 1]);
        if (m & kEdgeN) qk -= wv[k - unx] * (z[k - unx] + beta * p_old[k - unx]);
        if (m & kEdgeS) qk -= wv[k] * (z[k + unx] + beta * p_old[k + unx]);
        p[k] = pk;
        q[k] = qk;
        pq += pk * qk;
    }
    pq = block_sum(pq, red);
    if (threadIdx.x == 0) pq_part[blockIdx.x] = pq;
}

// Launch 2: alpha = (r.z) / (p.q) (0 when p.q is 0), x += alpha p, r -= alpha q, z = r / diag; partials of r.z and r.r
__global__ __launch_bounds__(kThreads) void pcg_update_kernel(unsigned N, const unsigned char *__restrict__ mask,
                                                              double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                              const double *__restrict__ p, const double *__restrict__ q,
                                                              const double *__restrict__ diag, const double *__restrict__ rz_cur,
                                                              const double *__restrict__ pq_part, int n_parts,
                                                              double *__restrict__ rz_next, double *__restrict__ rr_part) {
    __shared__ double red[kThreads / 64];
    const double rz_c = sum_parts(rz_cur, n_parts, red), pq = sum_parts(pq_part, n_parts, red);
    const double alpha = pq != 0.0 ? rz_c / pq : 0.0;
    double rz = 0.0, rr = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        if (!(mask[k] & kSolve)) continue;
        x[k] = x[k] + alpha * p[k];
        const double rk = r[k] - alpha * q[k];
        const double zk = rk / diag[k];
        r[k] = rk;
        z[k] = zk;
        rz += rk * zk;
        rr += rk * rk;
    }
    rz = block_sum(rz, red);
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) {
        rz_next[blockIdx.x] = rz;
        rr_part[blockIdx.x] = rr;
    }
}

// phi: fixed nodes their value, solved nodes x (already in place), every other node NaN
__global__ __launch_bounds__(kThreads) void finalize_kernel(unsigned N, const unsigned char *__restrict__ mask,
                                                            const double *__restrict__ value, double *__restrict__ phi) {
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        const unsigned char m = mask[k];
        if (m & kFixed) phi[k] = value ? value[k] : 0.0;
        else if (!(m & kSolve)) phi[k] = __builtin_nan("");
    }
}

// The solve bits: a BFS from every fixed node along live edges into the unknown nodes.  Returns (unknowns, unreachable).
std::pair<long long, long long> reachability(std::vector<unsigned char> &mask, int nx) {
    const long long N = (long long)mask.size();
    std::vector<int> queue;
    queue.reserve((size_t)N);
    for (long long k = 0; k < N; k++)
        if (mask[k] & kFixed) queue.push_back((int)k);
    for (size_t h = 0; h < queue.size(); h++) {
        const int k = queue[h];
        const unsigned char m = mask[k];
        const int nb[4] = {k + 1, k + nx, k - 1, k - nx};
        const unsigned char bit[4] = {kEdgeE, kEdgeS, kEdgeW, kEdgeN};
        for (int e = 0; e < 4; e++) {
            if (!(m & bit[e])) continue;
            unsigned char &mn = mask[nb[e]];
            if (mn & (kFixed | kSolve)) continue;
            mn |= kSolve;
            queue.push_back(nb[e]);
        }
    }
    long long unknowns = 0, unreachable = 0;
    for (long long k = 0; k < N; k++) {
        if (mask[k] & kFixed) continue;
        if (mask[k] & kSolve) unknowns++;
        else unreachable++;
    }
    return {unknowns, unreachable};
}

// the device work vectors of one call (N values each; parts: 4 kMaxBlocks + 1)
struct Work {
    double *wh, *wv, *diag, *r, *z, *p0, *p1, *q, *parts;
    unsigned char *mask;
};

int solve(hipStream_t stream, unsigned N, int blocks, int nx, int ny, double hx, double hy, double tol, int max_iter, const Inputs &in,
          double *d_phi, const Work &w, photon_integrate_stats_t *stats) {
    (void)ny;
    double *rz_part[2] = {w.parts, w.parts + kMaxBlocks};
    double *pq_part = w.parts + 2 * kMaxBlocks, *rr_part = w.parts + 3 * kMaxBlocks, *d_scalar = w.parts + 4 * kMaxBlocks;
    double *x = d_phi;                                          // the iterate lives in the output

    hipLaunchKernelGGL(assemble_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, hx, hy, w.wh, w.wv, w.diag, w.r, w.mask);
    PH_CHECK(hipGetLastError());
    std::vector<unsigned char> mask(N);
    PH_CHECK(hipMemcpyAsync(mask.data(), w.mask, N, hipMemcpyDeviceToHost, stream));
    PH_CHECK(hipStreamSynchronize(stream));
    const auto counts = reachability(mask, nx);
    PH_CHECK(hipMemcpyAsync(w.mask, mask.data(), N, hipMemcpyHostToDevice, stream));

    hipLaunchKernelGGL(pcg_init_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, w.mask, w.diag, x, w.r, w.z, w.p0, w.p1, w.q,
                       rz_part[0], rr_part);
    PH_CHECK(hipGetLastError());
    auto residual_sq = [&](double *out) -> int {
        PH_CHECK(read_sum(rr_part, blocks, d_scalar, out, stream));
        return 0;
    };
    double rr = 0.0;
    if (int e = residual_sq(&rr)) return e;
    const double bnorm = std::sqrt(rr);

    double *pbuf[2] = {w.p0, w.p1};
    int it = 0;
    if (bnorm > 0.0) {
        for (;;) {
            if (it % PHOTON_INTEGRATE_CHECK_EVERY == 0) {
                if (it > 0)
                    if (int e = residual_sq(&rr)) return e;
                if (tol > 0.0 && std::sqrt(rr) <= tol * bnorm) break;
            }
            if (it == max_iter) {
                if (it % PHOTON_INTEGRATE_CHECK_EVERY != 0)     // the final residual of a run that stops between checks
                    if (int e = residual_sq(&rr)) return e;
                break;
            }
            const int cur = it & 1, old = cur ^ 1;
            hipLaunchKernelGGL(pcg_direction_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, nx, w.mask, w.z, pbuf[old], pbuf[cur],
                               w.q, w.diag, w.wh, w.wv, rz_part[cur], rz_part[old], blocks, it == 0 ? 1 : 0, pq_part);
            PH_CHECK(hipGetLastError());
            hipLaunchKernelGGL(pcg_update_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, w.mask, x, w.r, w.z, pbuf[cur], w.q,
                               w.diag, rz_part[cur], pq_part, blocks, rz_part[old], rr_part);
            PH_CHECK(hipGetLastError());
            it++;
        }
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, w.mask, in.value, d_phi);
    PH_CHECK(hipGetLastError());
    PH_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        stats->iterations = it;
        stats->converged = bnorm > 0.0 ? (std::sqrt(rr) <= tol * bnorm ? 1 : 0) : 1;
        stats->residual = bnorm > 0.0 ? std::sqrt(rr) / bnorm : 0.0;
        stats->unknowns = (int)counts.first;
        stats->unreachable = (int)counts.second;
    }
    return 0;
}

}  // namespace

extern "C" int photon_integrate_gradient(const double *d_gx, const double *d_gy, const double *d_w, const unsigned char *d_fixed,
                                         const double *d_value, int nx, int ny, double hx, double hy, double tol, int max_iter,
                                         double *d_phi, photon_integrate_stats_t *stats, void *stream_p) {
    const char *bad = nullptr;
    if (nx < 2 || ny < 2) bad = "nx and ny must be >= 2";
    else if ((long long)nx * ny > INT_MAX) bad = "more than INT_MAX nodes";
    else if (!std::isfinite(hx) || !(hx > 0.0) || !std::isfinite(hy) || !(hy > 0.0)) bad = "hx and hy must be finite and > 0";
    else if (!(tol >= 0.0)) bad = "tol must be >= 0";
    else if (max_iter < 0) bad = "max_iter must be >= 0";
    else if (!d_gx || !d_gy || !d_phi) bad = "null d_gx, d_gy or d_phi";
    if (bad) {
        fprintf(stderr, "photon: photon_integrate_gradient: %s (%d x %d nodes, hx %g, hy %g, tol %g, max_iter %d)\n", bad, ny, nx,
                hx, hy, tol, max_iter);
        return 1;
    }
    return guarded("photon_integrate_gradient", [&]() -> int {
        hipStream_t stream = (hipStream_t)stream_p;
        const unsigned N = (unsigned)nx * (unsigned)ny;
        const int blocks = (int)std::min<unsigned>(kMaxBlocks, (N + kThreads - 1) / kThreads);
        PoolBuffer<double> wh, wv, diag, r, z, p0, p1, q, parts;
        PoolBuffer<unsigned char> d_mask;
        PH_CHECK(wh.alloc(N));
        PH_CHECK(wv.alloc(N));
        PH_CHECK(diag.alloc(N));
        PH_CHECK(r.alloc(N));
        PH_CHECK(z.alloc(N));
        PH_CHECK(p0.alloc(N));
        PH_CHECK(p1.alloc(N));
        PH_CHECK(q.alloc(N));
        PH_CHECK(parts.alloc(4 * kMaxBlocks + 1));
        PH_CHECK(d_mask.alloc(N));
        const int rc = solve(stream, N, blocks, nx, ny, hx, hy, tol, max_iter, Inputs{d_gx, d_gy, d_w, d_fixed, d_value, nx, ny}, d_phi,
                             Work{wh.p, wv.p, diag.p, r.p, z.p, p0.p, p1.p, q.p, parts.p, d_mask.p}, stats);
        if (rc) (void)hipStreamSynchronize(stream);          // the blocks go back to the cache: nothing may still use them
        return rc;
    });
}
