// photon_tomo.hip - tomography: the 3-D field from several views' projected density (section 9) or from their deflections
// (section 10).  Definition: include/parallel_ray_tracing.h; host model: photon_amd/tomography.py (the same operations in
// numpy).
//
// One walk (RayWalk) yields the taps of a ray -- Joseph's method: the grid planes along the ray's dominant axis, a bilinear
// footprint of four voxels in each (RayWalk::cell: does the plane count, and where in its cell does the ray cross it).  An
// operator is that walk with K weights per tap, and a policy says which:
//   Projection (K = 1): the bilinear weights times the path length per plane -- A f of section 9;
//   Deflection (K = 2): per transverse vector tau the derivative of those weights under a parallel shift of the ray along
//                       tau (ShiftRates) -- D_t1 f and D_t2 f of section 10.
// A policy has K, init(rw, rays, ray) (false: the ray is a miss) and weights(fb, fc, w[K][4]), and three kernels are
// templated on it: forward_kernel sums w[k][j] * f[voxel j] per component in registers, adjoint_kernel adds one value per
// tap (the sum over k of w[k][j] * y[k]) into the voxel with a f64 atomic, rays_kernel (the solver's set-up) only asks
// whether a plane counts: the three cannot disagree about a tap.  One ray per lane: the rays of a view are stored row by
// row, so the 64 rays of a wave cross a slice at neighbouring voxels -- the forward gathers and the adjoint's atomics of
// one wave-instruction fall into a few rows of one slice (contiguous when the in-slice axis the lanes run along is x), and
// the adjoint sums lanes that meet in a voxel before it adds (wave_add).
//
// The solver is CG on the normal equations with alpha and beta kept on the device (fixed_sum.hpp, as photon_density.hip
// does): per iteration forward, zero, adjoint and three element-wise launches over the voxels
//   apply:     s = m (s + reg G^T G q), partials of q.s
//   update:    alpha = rho / q.s, x += alpha q, r -= alpha s, partials of r.r
//   direction: beta = rho' / rho, q = r + beta q
// with reg = lambda h^2 in section 9 and lambda in section 10.  The host reads one f64 (|r|^2) every
// PHOTON_TOMO_CHECK_EVERY iterations.
#include <climits>
#include <cmath>

#include "fixed_sum.hpp"
#include "photon_internal.hpp"

using namespace photon;

namespace {

struct Grid {
    int nx, ny, nz;
    double hx, hy, hz, gx, gy, gz;              // spacing, origin
};

// the rays of a call: origins and dirs [n, 3]; tau: section 10's transverse vectors [n, 3] (section 9: unused)
struct Rays {
    const double *origins, *dirs, *tau[2];
    long long n;
};

// K values per ray, one array per component
template <int K>
struct PerRay {
    const double *p[K];
};
template <int K>
struct PerRayOut {
    double *p[K];
};

// One ray's walk through the grid (the definition's steps 1 to 3): init, then cell(kappa) for kappa = 0 .. na - 1.
struct RayWalk {
    // axis a, then the other two in axis order (b, c): extent, voxel stride, ray origin, unit direction, grid origin, spacing
    int axis, na, nb, nc, sa, sb, sc;
    double oa, ob, oc, ea, eb, ec, ga, gb, gc, ha, hb, hc, scale;

    // false: the ray is a miss
    __device__ __forceinline__ bool init(const Grid &g, const double *__restrict__ origins, const double *__restrict__ dirs, long long ray) {
        const double ox = origins[3 * ray], oy = origins[3 * ray + 1], oz = origins[3 * ray + 2];
        const double dx = dirs[3 * ray], dy = dirs[3 * ray + 1], dz = dirs[3 * ray + 2];
        if (!(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz))) return false;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        if (!(isfinite(len) && len > 0.0)) return false;
        const double ex = dx / len, ey = dy / len, ez = dz / len;
        int a = 0;
        double ma = fabs(ex);
        if (fabs(ey) > ma) { a = 1; ma = fabs(ey); }
        if (fabs(ez) > ma) { a = 2; ma = fabs(ez); }
        const int sy = g.nx, sz = g.nx * g.ny;
        if (a == 0) {
            na = g.nx; nb = g.ny; nc = g.nz; sa = 1; sb = sy; sc = sz;
            oa = ox; ob = oy; oc = oz; ea = ex; eb = ey; ec = ez; ga = g.gx; gb = g.gy; gc = g.gz; ha = g.hx; hb = g.hy; hc = g.hz;
        } else if (a == 1) {
            na = g.ny; nb = g.nx; nc = g.nz; sa = sy; sb = 1; sc = sz;
            oa = oy; ob = ox; oc = oz; ea = ey; eb = ex; ec = ez; ga = g.gy; gb = g.gx; gc = g.gz; ha = g.hy; hb = g.hx; hc = g.hz;
        } else {
            na = g.nz; nb = g.nx; nc = g.ny; sa = sz; sb = 1; sc = sy;
            oa = oz; ob = ox; oc = oy; ea = ez; eb = ex; ec = ey; ga = g.gz; gb = g.gx; gc = g.gy; ha = g.hz; hb = g.hx; hc = g.hy;
        }
        axis = a;
        scale = ha / ma;
        return true;
    }

    // Does plane kappa count?  Then its taps are the voxels c, c + sb, c + sc, c + sb + sc, and (fb, fc) is where the ray
    // crosses the plane inside that cell (step 3 of the definition).
    __device__ __forceinline__ bool cell(int kappa, int &c, double &fb, double &fc) const {
        const double at = ga + (double)kappa * ha;
        const double t = (at - oa) / ea;
        const double u = ((ob + t * eb) - gb) / hb, v = ((oc + t * ec) - gc) / hc;
        if (!(u >= 0.0 && u <= (double)(nb - 1) && v >= 0.0 && v <= (double)(nc - 1))) return false;
        const int ib = min((int)floor(u), nb - 2), ic = min((int)floor(v), nc - 2);     // 0 <= ib <= nb - 2: every tap is a voxel
        fb = u - (double)ib;
        fc = v - (double)ic;
        c = kappa * sa + ib * sb + ic * sc;
        return true;
    }
};

// Section 9's projector: the weights of a counted plane's four taps (step 4 of the definition).
struct Projection {
    static constexpr int K = 1;
    double scale;

    __device__ __forceinline__ bool init(const RayWalk &rw, const Rays &, long long) {
        scale = rw.scale;
        return true;
    }

    __device__ __forceinline__ void weights(double fb, double fc, double (&w)[K][4]) const {
        const double hb1 = 1.0 - fb, hc1 = 1.0 - fc;
        w[0][0] = (hb1 * hc1) * scale;
        w[0][1] = (fb * hc1) * scale;
        w[0][2] = (hb1 * fc) * scale;
        w[0][3] = (fb * fc) * scale;
    }
};

// Per ray and vector tau: how fast the crossing point (u, v) of every plane moves under a parallel shift of the ray along
// tau, times scale.
struct ShiftRates {
    double pu, pv;

    // false: an entry of tau is not finite (the ray is a miss)
    __device__ __forceinline__ bool init(const RayWalk &rw, const double *__restrict__ tau, long long ray) {
        const double tx = tau[3 * ray], ty = tau[3 * ray + 1], tz = tau[3 * ray + 2];
        if (!(isfinite(tx) && isfinite(ty) && isfinite(tz))) return false;
        const double ta = rw.axis == 0 ? tx : (rw.axis == 1 ? ty : tz);
        const double tb = rw.axis == 0 ? ty : tx;
        const double tc = rw.axis == 2 ? ty : tz;
        const double r = ta / rw.ea;
        pu = ((tb - r * rw.eb) / rw.hb) * rw.scale;
        pv = ((tc - r * rw.ec) / rw.hc) * rw.scale;
        return true;
    }

    // the weights of a counted plane's four taps, in the projector's tap order
    __device__ __forceinline__ void weights(double fb, double fc, double (&w)[4]) const {
        const double gb = 1.0 - fb, gc = 1.0 - fc;
        const double gcu = gc * pu, gbv = gb * pv, fcu = fc * pu, fbv = fb * pv;
        w[0] = -gcu - gbv;
        w[1] = gcu - fbv;
        w[2] = gbv - fcu;
        w[3] = fcu + fbv;
    }
};

// Section 10's operator pair: the derivative of the projector under a parallel shift of the ray along rays.tau[0], tau[1].
struct Deflection {
    static constexpr int K = 2;
    ShiftRates s[K];

    __device__ __forceinline__ bool init(const RayWalk &rw, const Rays &rays, long long ray) {
        return s[0].init(rw, rays.tau[0], ray) && s[1].init(rw, rays.tau[1], ray);
    }

    __device__ __forceinline__ void weights(double fb, double fc, double (&w)[K][4]) const {
        s[0].weights(fb, fc, w[0]);
        s[1].weights(fb, fc, w[1]);
    }
};

// out[k] = (Op f)[k]; with `weight` (the solver): weight (Op f), 0 where the weight is 0
template <typename Op>
__global__ __launch_bounds__(kThreads) void forward_kernel(Grid g, const double *__restrict__ f, Rays rays,
                                                           const double *__restrict__ weight, PerRayOut<Op::K> out) {
    constexpr int K = Op::K;
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < rays.n; ray += (long long)gridDim.x * kThreads) {
        const double w = weight ? weight[ray] : 1.0;
        double acc[K] = {};
        RayWalk rw;
        Op op;
        if (w > 0.0 && rw.init(g, rays.origins, rays.dirs, ray) && op.init(rw, rays, ray)) {
            for (int kappa = 0; kappa < rw.na; kappa++) {
                int c;
                double fb, fc, wt[K][4];
                if (!rw.cell(kappa, c, fb, fc)) continue;
                op.weights(fb, fc, wt);
                const double fv[4] = {f[c], f[c + rw.sb], f[c + rw.sc], f[c + rw.sb + rw.sc]};
#pragma unroll
                for (int k = 0; k < K; k++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[k] += wt[k][j] * fv[j];
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) out.p[k][ray] = weight ? (w > 0.0 ? w * acc[k] : 0.0) : acc[k];
    }
}

// One tap of every lane of the wave: v[voxel] += value, voxel < 0 = nothing to add.  Neighbouring rays cross a slice at
// neighbouring voxels, several to a voxel where the rays are denser than the grid, and adds of one wave-instruction to one
// address are served one after the other.  So every run of adjacent lanes with one voxel is summed first (a segmented
// shift-and-add: after the step of distance d a lane holds the sum of its run's lanes [l, l + 2d)), and only the first lane
// of the run adds.  Lanes with the same voxel that are not adjacent stay separate adds.  Every lane of the wave calls this
// together.  -DPHOTON_TOMO_MERGE_LANES=0 builds the form it is measured against: one atomic per tap (tools/build_variant.py,
// tools/bos_tomography.py --compare-library).
#ifndef PHOTON_TOMO_MERGE_LANES
#define PHOTON_TOMO_MERGE_LANES 1
#endif
__device__ __forceinline__ void wave_add(double *__restrict__ v, int voxel, double value) {
    if (!PHOTON_TOMO_MERGE_LANES) {
        if (voxel >= 0) atomicAdd(v + voxel, value);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(voxel, 1, 64);
    const bool head = lane == 0 || before != voxel;
    const unsigned long long heads = __ballot(head);
    const unsigned long long later_heads = lane < 63 ? heads >> (lane + 1) : 0ull;
    const int rest = voxel < 0 ? 0 : (later_heads ? __ffsll(later_heads) - 1 : 63 - lane);      // lanes of the run after this one
    for (int d = 1; d < 64; d <<= 1) {
        const double more = __shfl_down(value, d, 64);
        if (__ballot(d <= rest) == 0) break;                    // no run reaches beyond d lanes
        if (d <= rest) value += more;
    }
    if (head && voxel >= 0) atomicAdd(v + voxel, value);
}

// v += Op^T y, one add per tap: w[0][j] y[0] (+ w[1][j] y[1]).  Every lane of a wave walks the same number of planes (the
// longest axis any of its rays walks), so that the lanes can sum what goes to one voxel (wave_add); a lane whose plane does
// not count offers voxel -1.
template <typename Op>
__global__ __launch_bounds__(kThreads) void adjoint_kernel(Grid g, PerRay<Op::K> y, Rays rays, double *__restrict__ v) {
    constexpr int K = Op::K;
    for (long long base = (long long)blockIdx.x * kThreads; base < rays.n; base += (long long)gridDim.x * kThreads) {
        const long long ray = base + threadIdx.x;
        double yi[K];
        bool live = false;                                      // a ray whose y are all 0 adds nothing
#pragma unroll
        for (int k = 0; k < K; k++) {
            yi[k] = ray < rays.n ? y.p[k][ray] : 0.0;
            live = live || yi[k] != 0.0;
        }
        RayWalk rw;
        Op op;
        live = live && rw.init(g, rays.origins, rays.dirs, ray) && op.init(rw, rays, ray);
        const int mine = live ? rw.na : 0;
        int planes = 0;                                         // the wave's maximum of `mine`: one of the three extents
        if (__ballot(mine == g.nx)) planes = g.nx;
        if (__ballot(mine == g.ny)) planes = max(planes, g.ny);
        if (__ballot(mine == g.nz)) planes = max(planes, g.nz);
        for (int kappa = 0; kappa < planes; kappa++) {
            int c = 0;
            double fb = 0.0, fc = 0.0, wt[K][4] = {};
            const bool counts = kappa < mine && rw.cell(kappa, c, fb, fc);
            if (counts) op.weights(fb, fc, wt);
            double tap[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                tap[j] = wt[0][j] * yi[0];
#pragma unroll
                for (int k = 1; k < K; k++) tap[j] += wt[k][j] * yi[k];
            }
            wave_add(v, counts ? c : -1, tap[0]);
            wave_add(v, counts ? c + rw.sb : -1, tap[1]);
            wave_add(v, counts ? c + rw.sc : -1, tap[2]);
            wave_add(v, counts ? c + rw.sb + rw.sc : -1, tap[3]);
        }
    }
}

// the solver's rays: weight = w where all K data values and w are finite and w > 0, else 0; wdata = weight data (0 at
// weight 0); counts the rays of positive weight that are no miss (section 10: their vectors included) and cross the grid
template <typename Op>
__global__ __launch_bounds__(kThreads) void rays_kernel(Grid g, PerRay<Op::K> data, const double *__restrict__ w, Rays rays,
                                                        double *__restrict__ weight, PerRayOut<Op::K> wdata,
                                                        unsigned long long *__restrict__ rays_used) {
    constexpr int K = Op::K;
    __shared__ double red[kThreads / 64];
    double count = 0.0;
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < rays.n; ray += (long long)gridDim.x * kThreads) {
        const double wi = w ? w[ray] : 1.0;
        double di[K];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < K; k++) {
            di[k] = data.p[k][ray];
            ok = ok && isfinite(di[k]);
        }
        ok = ok && isfinite(wi) && wi > 0.0;
        weight[ray] = ok ? wi : 0.0;
#pragma unroll
        for (int k = 0; k < K; k++) wdata.p[k][ray] = ok ? wi * di[k] : 0.0;
        RayWalk rw;
        Op op;
        bool used = false;
        if (ok && rw.init(g, rays.origins, rays.dirs, ray) && op.init(rw, rays, ray)) {
            int c;
            double fb, fc;
            for (int kappa = 0; kappa < rw.na && !used; kappa++) used = rw.cell(kappa, c, fb, fc);
        }
        count += used ? 1.0 : 0.0;
    }
    count = block_sum(count, red);                              // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0 && count > 0.0) atomicAdd(rays_used, (unsigned long long)count);
}

__device__ __forceinline__ bool in_support(const unsigned char *__restrict__ support, unsigned k) { return support ? support[k] != 0 : true; }

// r holds A^T (W p): r = b = m r, q = r, x = 0; partials of r.r; the number of support voxels
__global__ __launch_bounds__(kThreads) void cg_init_kernel(unsigned N, const unsigned char *__restrict__ support, double *__restrict__ x,
                                                           double *__restrict__ r, double *__restrict__ q, double *__restrict__ rho_part,
                                                           unsigned long long *__restrict__ unknowns) {
    __shared__ double red[kThreads / 64];
    double rr = 0.0, count = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        const bool m = in_support(support, k);
        const double rk = m ? r[k] : 0.0;
        x[k] = 0.0;
        r[k] = rk;
        q[k] = rk;
        rr += rk * rk;
        count += m ? 1.0 : 0.0;
    }
    rr = block_sum(rr, red);
    count = block_sum(count, red);                              // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0) {
        rho_part[blockIdx.x] = rr;
        atomicAdd(unknowns, (unsigned long long)count);
    }
}

// s holds A^T (W (A q)): s = m (s + lam_h2 G^T G q), the neighbours in the order -x, +x, -y, +y, -z, +z; partials of q.s
__global__ __launch_bounds__(kThreads) void cg_apply_kernel(unsigned N, int nx, int ny, int nz, const unsigned char *__restrict__ support,
                                                            double lam_h2, const double *__restrict__ q, double *__restrict__ s,
                                                            double *__restrict__ qs_part) {
    __shared__ double red[kThreads / 64];
    const unsigned unx = (unsigned)nx, uny = (unsigned)ny, slab = unx * uny;
    double qs = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        double sk = 0.0;
        if (in_support(support, k)) {
            const unsigned kk = k / slab, rem = k - kk * slab, j = rem / unx, i = rem - j * unx;
            const double qc = q[k];
            double lap = 0.0;
            if (i > 0) lap += qc - q[k - 1];
            if (i < unx - 1) lap += qc - q[k + 1];
            if (j > 0) lap += qc - q[k - unx];
            if (j < uny - 1) lap += qc - q[k + unx];
            if (kk > 0) lap += qc - q[k - slab];
            if (kk < (unsigned)nz - 1) lap += qc - q[k + slab];
            sk = s[k] + lam_h2 * lap;
            qs += qc * sk;
        }
        s[k] = sk;
    }
    qs = block_sum(qs, red);
    if (threadIdx.x == 0) qs_part[blockIdx.x] = qs;
}

// alpha = rho / q.s (0 when q.s is 0), x += alpha q, r -= alpha s; partials of the new r.r
__global__ __launch_bounds__(kThreads) void cg_update_kernel(unsigned N, double *__restrict__ x, double *__restrict__ r,
                                                             const double *__restrict__ q, const double *__restrict__ s,
                                                             const double *__restrict__ rho_cur, const double *__restrict__ qs_part,
                                                             int n_parts, double *__restrict__ rho_next) {
    __shared__ double red[kThreads / 64];
    const double rho = sum_parts(rho_cur, n_parts, red), qs = sum_parts(qs_part, n_parts, red);
    const double alpha = qs != 0.0 ? rho / qs : 0.0;
    double rr = 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) {
        x[k] = x[k] + alpha * q[k];
        const double rk = r[k] - alpha * s[k];
        r[k] = rk;
        rr += rk * rk;
    }
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) rho_next[blockIdx.x] = rr;
}

// beta = rho' / rho (0 when rho is 0), q = r + beta q
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(unsigned N, const double *__restrict__ r, double *__restrict__ q,
                                                                const double *__restrict__ rho_new, const double *__restrict__ rho_old,
                                                                int n_parts) {
    __shared__ double red[kThreads / 64];
    const double a = sum_parts(rho_new, n_parts, red), b = sum_parts(rho_old, n_parts, red);
    const double beta = b != 0.0 ? a / b : 0.0;
    for (unsigned k = blockIdx.x * kThreads + threadIdx.x; k < N; k += gridDim.x * kThreads) q[k] = r[k] + beta * q[k];
}

// what every entry point refuses about the grid and the rays
const char *grid_refusal(int nx, int ny, int nz, const double *spacing, const double *origin, long long n_rays) {
    if (nx < 2 || ny < 2 || nz < 2) return "nx, ny and nz must be >= 2";
    if ((long long)nx * ny * nz > INT_MAX) return "more than INT_MAX voxels";
    if (n_rays < 1) return "n_rays must be >= 1";
    if (!spacing || !origin) return "null spacing or origin";
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0)) return "every spacing must be finite and > 0";
        if (!std::isfinite(origin[a])) return "every origin must be finite";
    }
    return nullptr;
}

Grid make_grid(int nx, int ny, int nz, const double *spacing, const double *origin) {
    return Grid{nx, ny, nz, spacing[0], spacing[1], spacing[2], origin[0], origin[1], origin[2]};
}

int ray_blocks(long long n_rays) { return (int)std::min<long long>((n_rays + kThreads - 1) / kThreads, INT_MAX); }

// the device work vectors of one solve: r, q, s over the voxels; weight and t[k], k < K, over the rays; parts: 3 kMaxBlocks
// + 1; 2 counters
struct Work {
    double *r, *q, *s, *weight, *t[2], *parts;
    unsigned long long *counters;
};

// The operator of policy Op on a grid and its rays: the launches of the three kernels.
template <typename Op>
struct Operator {
    static constexpr int K = Op::K;
    Grid g;
    Rays rays;

    // out = Op f, or weight (Op f) with `weight`
    int forward(const double *f, const double *weight, const PerRayOut<K> &out, hipStream_t stream) const {
        hipLaunchKernelGGL(forward_kernel<Op>, dim3(ray_blocks(rays.n)), dim3(kThreads), 0, stream, g, f, rays, weight, out);
        PH_CHECK(hipGetLastError());
        return 0;
    }
    // v += Op^T y
    int adjoint(const PerRay<K> &y, double *v, hipStream_t stream) const {
        hipLaunchKernelGGL(adjoint_kernel<Op>, dim3(ray_blocks(rays.n)), dim3(kThreads), 0, stream, g, y, rays, v);
        PH_CHECK(hipGetLastError());
        return 0;
    }
    // a solve's weight and weighted data over the rays (w.weight, w.t), the used rays in w.counters[0]
    int prepare(const PerRay<K> &data, const double *d_w, const Work &w, hipStream_t stream) const {
        PerRayOut<K> wdata;
        for (int k = 0; k < K; k++) wdata.p[k] = w.t[k];
        hipLaunchKernelGGL(rays_kernel<Op>, dim3(ray_blocks(rays.n)), dim3(kThreads), 0, stream, g, data, d_w, rays, w.weight, wdata,
                           w.counters);
        PH_CHECK(hipGetLastError());
        return 0;
    }
};

// CG on  m (Op^T W Op + reg G^T G) m x = m Op^T W data  from x = 0 (the iteration of section 9)
template <typename Op>
int solve(hipStream_t stream, const Operator<Op> &op, const PerRay<Op::K> &data, const double *d_w, const unsigned char *d_support,
          double reg, double tol, int max_iter, double *x, const Work &w, photon_tomo_stats_t *stats) {
    const Grid &g = op.g;
    const unsigned N = (unsigned)g.nx * (unsigned)g.ny * (unsigned)g.nz;
    const int blocks = (int)std::min<unsigned>(kMaxBlocks, (N + kThreads - 1) / kThreads);
    double *rho_part[2] = {w.parts, w.parts + kMaxBlocks};
    double *qs_part = w.parts + 2 * kMaxBlocks, *d_scalar = w.parts + 3 * kMaxBlocks;
    PerRayOut<Op::K> t_out;                                     // w.t as the forward's output and the adjoint's input
    PerRay<Op::K> t_in;
    for (int k = 0; k < Op::K; k++) t_in.p[k] = t_out.p[k] = w.t[k];

    PH_CHECK(hipMemsetAsync(w.counters, 0, 2 * sizeof(unsigned long long), stream));
    PH_CHECK(hipMemsetAsync(w.r, 0, (size_t)N * sizeof(double), stream));
    PH_TRY(op.prepare(data, d_w, w, stream));
    PH_TRY(op.adjoint(t_in, w.r, stream));
    hipLaunchKernelGGL(cg_init_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, d_support, x, w.r, w.q, rho_part[0], w.counters + 1);
    PH_CHECK(hipGetLastError());

    double rr = 0.0;
    PH_CHECK(read_sum(rho_part[0], blocks, d_scalar, &rr, stream));
    const double bnorm = std::sqrt(rr);

    int it = 0;
    if (bnorm > 0.0) {
        for (;;) {
            const int cur = it & 1, old = cur ^ 1;               // rho_part[cur] holds r.r after `it` iterations
            if (it % PHOTON_TOMO_CHECK_EVERY == 0) {
                if (it > 0) PH_CHECK(read_sum(rho_part[cur], blocks, d_scalar, &rr, stream));
                if (tol > 0.0 && std::sqrt(rr) <= tol * bnorm) break;
            }
            if (it == max_iter) {
                if (it % PHOTON_TOMO_CHECK_EVERY != 0) PH_CHECK(read_sum(rho_part[cur], blocks, d_scalar, &rr, stream));    // a run that stops between checks
                break;
            }
            PH_TRY(op.forward(w.q, w.weight, t_out, stream));
            PH_CHECK(hipMemsetAsync(w.s, 0, (size_t)N * sizeof(double), stream));
            PH_TRY(op.adjoint(t_in, w.s, stream));
            hipLaunchKernelGGL(cg_apply_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, g.nx, g.ny, g.nz, d_support, reg, w.q, w.s,
                               qs_part);
            PH_CHECK(hipGetLastError());
            hipLaunchKernelGGL(cg_update_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, x, w.r, w.q, w.s, rho_part[cur], qs_part, blocks,
                               rho_part[old]);
            PH_CHECK(hipGetLastError());
            hipLaunchKernelGGL(cg_direction_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, w.r, w.q, rho_part[old], rho_part[cur], blocks);
            PH_CHECK(hipGetLastError());
            it++;
        }
    }
    unsigned long long counters[2] = {0, 0};
    PH_CHECK(hipMemcpyAsync(counters, w.counters, sizeof counters, hipMemcpyDeviceToHost, stream));
    PH_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        stats->iterations = it;
        stats->converged = bnorm > 0.0 ? (std::sqrt(rr) <= tol * bnorm ? 1 : 0) : 1;
        stats->residual = bnorm > 0.0 ? std::sqrt(rr) / bnorm : 0.0;
        stats->rays_used = (long long)counters[0];
        stats->unknowns = (long long)counters[1];
    }
    return 0;
}

// a solve with its work vectors from the pool (t[1] only when there is a second component)
template <typename Op>
int pooled_solve(const char *what, hipStream_t stream, const Operator<Op> &op, const PerRay<Op::K> &data, const double *d_w,
                 const unsigned char *d_support, double reg, double tol, int max_iter, double *d_f, photon_tomo_stats_t *stats) {
    return guarded(what, [&]() -> int {
        const size_t N = (size_t)op.g.nx * op.g.ny * op.g.nz, n_rays = (size_t)op.rays.n;
        PoolBuffer<double> r, q, s, weight, t[2], parts;
        PoolBuffer<unsigned long long> counters;
        PH_CHECK(r.alloc(N));
        PH_CHECK(q.alloc(N));
        PH_CHECK(s.alloc(N));
        PH_CHECK(weight.alloc(n_rays));
        for (int k = 0; k < Op::K; k++) PH_CHECK(t[k].alloc(n_rays));
        PH_CHECK(parts.alloc(3 * kMaxBlocks + 1));
        PH_CHECK(counters.alloc(2));
        const int rc = solve(stream, op, data, d_w, d_support, reg, tol, max_iter, d_f,
                             Work{r.p, q.p, s.p, weight.p, {t[0].p, t[1].p}, parts.p, counters.p}, stats);
        if (rc) (void)hipStreamSynchronize(stream);          // the blocks go back to the cache: nothing may still use them
        return rc;
    });
}

// what both solvers refuse about lambda, tol and max_iter
const char *solver_refusal(double lambda, double tol, int max_iter) {
    if (!(lambda >= 0.0)) return "lambda must be >= 0";
    if (!(tol >= 0.0)) return "tol must be >= 0";
    if (max_iter < 0) return "max_iter must be >= 0";
    return nullptr;
}

// Every entry point's first step -- true: the call is refused, with the reason on stderr.  What is wrong with the grid
// comes first, then `solver_bad` (solver_refusal; nullptr for the operators), then `nulls` when `has_null`.
bool refused(const char *what, int nx, int ny, int nz, const double *spacing, const double *origin, long long n_rays,
             const char *solver_bad, bool has_null, const char *nulls) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad) bad = solver_bad;
    if (!bad && has_null) bad = nulls;
    if (bad) fprintf(stderr, "photon: %s: %s (%d x %d x %d voxels, %lld rays)\n", what, bad, nx, ny, nz, n_rays);
    return bad != nullptr;
}

}  // namespace

extern "C" int photon_tomo_project(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                   const double *d_origins, const double *d_dirs, long long n_rays, double *d_p, void *stream) {
    if (refused("photon_tomo_project", nx, ny, nz, spacing, origin, n_rays, nullptr, !d_f || !d_origins || !d_dirs || !d_p,
                "null d_f, d_origins, d_dirs or d_p"))
        return 1;
    const Operator<Projection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {nullptr, nullptr}, n_rays}};
    return op.forward(d_f, nullptr, {{d_p}}, (hipStream_t)stream);
}

extern "C" int photon_tomo_backproject(const double *d_y, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                       const double *d_origins, const double *d_dirs, long long n_rays, double *d_v, void *stream) {
    if (refused("photon_tomo_backproject", nx, ny, nz, spacing, origin, n_rays, nullptr, !d_y || !d_origins || !d_dirs || !d_v,
                "null d_y, d_origins, d_dirs or d_v"))
        return 1;
    const Operator<Projection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {nullptr, nullptr}, n_rays}};
    return op.adjoint({{d_y}}, d_v, (hipStream_t)stream);
}

extern "C" int photon_tomo_reconstruct(const double *d_p, const double *d_w, const unsigned char *d_support, int nx, int ny, int nz,
                                       const double spacing[3], const double origin[3], const double *d_origins, const double *d_dirs,
                                       long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                                       photon_tomo_stats_t *stats, void *stream) {
    if (refused("photon_tomo_reconstruct", nx, ny, nz, spacing, origin, n_rays, solver_refusal(lambda, tol, max_iter),
                !d_p || !d_origins || !d_dirs || !d_f, "null d_p, d_origins, d_dirs or d_f"))
        return 1;
    const Operator<Projection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {nullptr, nullptr}, n_rays}};
    const double h = std::min(spacing[0], std::min(spacing[1], spacing[2]));
    return pooled_solve("photon_tomo_reconstruct", (hipStream_t)stream, op, {{d_p}}, d_w, d_support, lambda * (h * h), tol, max_iter, d_f,
                        stats);
}

// ---- section 10 --------------------------------------------------------------------------------------------------------------
extern "C" int photon_tomo_deflect(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                   const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2, long long n_rays,
                                   double *d_g1, double *d_g2, void *stream) {
    if (refused("photon_tomo_deflect", nx, ny, nz, spacing, origin, n_rays, nullptr,
                !d_f || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_g1 || !d_g2, "null d_f, d_origins, d_dirs, d_t1, d_t2, d_g1 or d_g2"))
        return 1;
    const Operator<Deflection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {d_t1, d_t2}, n_rays}};
    return op.forward(d_f, nullptr, {{d_g1, d_g2}}, (hipStream_t)stream);
}

extern "C" int photon_tomo_deflect_adjoint(const double *d_y1, const double *d_y2, int nx, int ny, int nz, const double spacing[3],
                                           const double origin[3], const double *d_origins, const double *d_dirs, const double *d_t1,
                                           const double *d_t2, long long n_rays, double *d_v, void *stream) {
    if (refused("photon_tomo_deflect_adjoint", nx, ny, nz, spacing, origin, n_rays, nullptr,
                !d_y1 || !d_y2 || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_v, "null d_y1, d_y2, d_origins, d_dirs, d_t1, d_t2 or d_v"))
        return 1;
    const Operator<Deflection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {d_t1, d_t2}, n_rays}};
    return op.adjoint({{d_y1, d_y2}}, d_v, (hipStream_t)stream);
}

extern "C" int photon_tomo_reconstruct_deflections(const double *d_g1, const double *d_g2, const double *d_w, const unsigned char *d_support,
                                                   int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                                   const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2,
                                                   long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                                                   photon_tomo_stats_t *stats, void *stream) {
    if (refused("photon_tomo_reconstruct_deflections", nx, ny, nz, spacing, origin, n_rays, solver_refusal(lambda, tol, max_iter),
                !d_g1 || !d_g2 || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_f, "null d_g1, d_g2, d_origins, d_dirs, d_t1, d_t2 or d_f"))
        return 1;
    const Operator<Deflection> op{make_grid(nx, ny, nz, spacing, origin), Rays{d_origins, d_dirs, {d_t1, d_t2}, n_rays}};
    // no h^2: D carries 1 / length against A, so lambda weighs G^T G as it does in section 9
    return pooled_solve("photon_tomo_reconstruct_deflections", (hipStream_t)stream, op, {{d_g1, d_g2}}, d_w, d_support, lambda, tol,
                        max_iter, d_f, stats);
}
