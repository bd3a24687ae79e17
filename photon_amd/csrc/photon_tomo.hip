// photon_tomo.hip - tomography: the 3-D field from several views' projected density.  Definition:
// include/parallel_ray_tracing.h, section 9; host model: photon_amd/tomography.py (the same operations in numpy).
//
// One walk (RayWalk) yields the taps of a ray -- Joseph's method: the grid planes along the ray's dominant axis, a bilinear
// footprint of four voxels in each.  The projector sums weight * f[voxel] in a register, the adjoint adds weight * y into
// the voxel with a f64 atomic, the solver's set-up only asks whether a plane counts: the three cannot disagree about a tap.
// One ray per lane: the rays of a view are stored row by row, so the 64 rays of a wave cross a slice at neighbouring voxels
// -- the projector's gathers and the adjoint's atomics of one wave-instruction fall into a few rows of one slice
// (contiguous when the in-slice axis the lanes run along is x), and the adjoint sums lanes that meet in a voxel before it
// adds (wave_add).
//
// The solver is CG on the normal equations with alpha and beta kept on the device (fixed_sum.hpp, as photon_density.hip
// does): per iteration project, zero, backproject and three element-wise launches over the voxels
//   apply:     s = m (s + lambda h^2 G^T G q), partials of q.s
//   update:    alpha = rho / q.s, x += alpha q, r -= alpha s, partials of r.r
//   direction: beta = rho' / rho, q = r + beta q
// The host reads one f64 (|r|^2) every PHOTON_TOMO_CHECK_EVERY iterations.
//
// Section 10 (tomography from deflections) is the same walk with differentiated weights: D_tau f is the derivative of A f
// under a parallel shift of the ray along tau, so a counted plane has the same four taps and, per vector tau, the weights
// of ShiftRates::weights.  tomo_deflect_kernel sums both components in one walk, tomo_deflect_adjoint_kernel adds one
// value per tap (w1 y1 + w2 y2: the atomics of tomo_backproject_kernel, not twice them), and the solver is the one above
// (solve<Op>) with the operator pair of DeflectionOp and no h^2 on the regulariser.
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

// One ray's walk through the grid (the definition's steps 1 to 4): init, then plane(kappa) for kappa = 0 .. na - 1.
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

    // a counted plane's taps with the projector's weights w[0 .. 3] (step 4)
    __device__ __forceinline__ bool plane(int kappa, int &c, double (&w)[4]) const {
        double fb, fc;
        if (!cell(kappa, c, fb, fc)) return false;
        const double hb1 = 1.0 - fb, hc1 = 1.0 - fc;
        w[0] = (hb1 * hc1) * scale;
        w[1] = (fb * hc1) * scale;
        w[2] = (hb1 * fc) * scale;
        w[3] = (fb * fc) * scale;
        return true;
    }
};

// p = A f; with `weight` (the solver): p = weight (A f), 0 where the weight is 0
__global__ __launch_bounds__(kThreads) void tomo_project_kernel(Grid g, const double *__restrict__ f, const double *__restrict__ origins,
                                                                const double *__restrict__ dirs, long long n_rays,
                                                                const double *__restrict__ weight, double *__restrict__ p) {
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < n_rays; ray += (long long)gridDim.x * kThreads) {
        const double w = weight ? weight[ray] : 1.0;
        double acc = 0.0;
        RayWalk rw;
        if (w > 0.0 && rw.init(g, origins, dirs, ray)) {
            for (int kappa = 0; kappa < rw.na; kappa++) {
                int c;
                double wt[4];
                if (!rw.plane(kappa, c, wt)) continue;
                acc += wt[0] * f[c];
                acc += wt[1] * f[c + rw.sb];
                acc += wt[2] * f[c + rw.sc];
                acc += wt[3] * f[c + rw.sb + rw.sc];
            }
        }
        p[ray] = weight ? (w > 0.0 ? w * acc : 0.0) : acc;
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

// v += A^T y.  Every lane of a wave walks the same number of planes (the longest axis any of its rays walks), so that the
// lanes can sum what goes to one voxel (wave_add); a lane whose plane does not count offers voxel -1.
__global__ __launch_bounds__(kThreads) void tomo_backproject_kernel(Grid g, const double *__restrict__ y, const double *__restrict__ origins,
                                                                    const double *__restrict__ dirs, long long n_rays,
                                                                    double *__restrict__ v) {
    for (long long base = (long long)blockIdx.x * kThreads; base < n_rays; base += (long long)gridDim.x * kThreads) {
        const long long ray = base + threadIdx.x;
        const double yi = ray < n_rays ? y[ray] : 0.0;
        RayWalk rw;
        const bool live = yi != 0.0 && rw.init(g, origins, dirs, ray);     // a ray whose y is 0 adds nothing
        const int mine = live ? rw.na : 0;
        int planes = 0;                                         // the wave's maximum of `mine`: one of the three extents
        if (__ballot(mine == g.nx)) planes = g.nx;
        if (__ballot(mine == g.ny)) planes = max(planes, g.ny);
        if (__ballot(mine == g.nz)) planes = max(planes, g.nz);
        for (int kappa = 0; kappa < planes; kappa++) {
            int c = 0;
            double wt[4] = {0.0, 0.0, 0.0, 0.0};
            const bool counts = kappa < mine && rw.plane(kappa, c, wt);
            wave_add(v, counts ? c : -1, wt[0] * yi);
            wave_add(v, counts ? c + rw.sb : -1, wt[1] * yi);
            wave_add(v, counts ? c + rw.sc : -1, wt[2] * yi);
            wave_add(v, counts ? c + rw.sb + rw.sc : -1, wt[3] * yi);
        }
    }
}

// the solver's rays: weight = w where p and w are finite and w > 0, else 0; wp = weight p (0 at weight 0); counts the rays
// of positive weight that cross the grid
__global__ __launch_bounds__(kThreads) void tomo_rays_kernel(Grid g, const double *__restrict__ p, const double *__restrict__ w,
                                                             const double *__restrict__ origins, const double *__restrict__ dirs,
                                                             long long n_rays, double *__restrict__ weight, double *__restrict__ wp,
                                                             unsigned long long *__restrict__ rays_used) {
    __shared__ double red[kThreads / 64];
    double count = 0.0;
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < n_rays; ray += (long long)gridDim.x * kThreads) {
        const double pi = p[ray], wi = w ? w[ray] : 1.0;
        const bool ok = isfinite(pi) && isfinite(wi) && wi > 0.0;
        weight[ray] = ok ? wi : 0.0;
        wp[ray] = ok ? wi * pi : 0.0;
        RayWalk rw;
        bool used = false;
        if (ok && rw.init(g, origins, dirs, ray)) {
            int c;
            double wt[4];
            for (int kappa = 0; kappa < rw.na && !used; kappa++) used = rw.plane(kappa, c, wt);
        }
        count += used ? 1.0 : 0.0;
    }
    count = block_sum(count, red);                              // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0 && count > 0.0) atomicAdd(rays_used, (unsigned long long)count);
}

// ---- section 10: the derivative of the projector under a parallel shift of the ray ----------------------------------------
// Per ray and vector tau: how fast the crossing point (u, v) of every plane moves under the shift, times scale.
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

// g1 = D_t1 f, g2 = D_t2 f; with `weight` (the solver): weight (D f), 0 where the weight is 0
__global__ __launch_bounds__(kThreads) void tomo_deflect_kernel(Grid g, const double *__restrict__ f, const double *__restrict__ origins,
                                                                const double *__restrict__ dirs, const double *__restrict__ t1,
                                                                const double *__restrict__ t2, long long n_rays,
                                                                const double *__restrict__ weight, double *__restrict__ g1,
                                                                double *__restrict__ g2) {
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < n_rays; ray += (long long)gridDim.x * kThreads) {
        const double w = weight ? weight[ray] : 1.0;
        double acc1 = 0.0, acc2 = 0.0;
        RayWalk rw;
        ShiftRates s1, s2;
        if (w > 0.0 && rw.init(g, origins, dirs, ray) && s1.init(rw, t1, ray) && s2.init(rw, t2, ray)) {
            for (int kappa = 0; kappa < rw.na; kappa++) {
                int c;
                double fb, fc, w1[4], w2[4];
                if (!rw.cell(kappa, c, fb, fc)) continue;
                s1.weights(fb, fc, w1);
                s2.weights(fb, fc, w2);
                const double f0 = f[c], f1 = f[c + rw.sb], f2 = f[c + rw.sc], f3 = f[c + rw.sb + rw.sc];
                acc1 += w1[0] * f0;
                acc1 += w1[1] * f1;
                acc1 += w1[2] * f2;
                acc1 += w1[3] * f3;
                acc2 += w2[0] * f0;
                acc2 += w2[1] * f1;
                acc2 += w2[2] * f2;
                acc2 += w2[3] * f3;
            }
        }
        g1[ray] = weight ? (w > 0.0 ? w * acc1 : 0.0) : acc1;
        g2[ray] = weight ? (w > 0.0 ? w * acc2 : 0.0) : acc2;
    }
}

// v += D_t1^T y1 + D_t2^T y2, one add per tap: w1 y1 + w2 y2.  The lanes of a wave walk together as in
// tomo_backproject_kernel.
__global__ __launch_bounds__(kThreads) void tomo_deflect_adjoint_kernel(Grid g, const double *__restrict__ y1, const double *__restrict__ y2,
                                                                        const double *__restrict__ origins, const double *__restrict__ dirs,
                                                                        const double *__restrict__ t1, const double *__restrict__ t2,
                                                                        long long n_rays, double *__restrict__ v) {
    for (long long base = (long long)blockIdx.x * kThreads; base < n_rays; base += (long long)gridDim.x * kThreads) {
        const long long ray = base + threadIdx.x;
        const double ya = ray < n_rays ? y1[ray] : 0.0, yb = ray < n_rays ? y2[ray] : 0.0;
        RayWalk rw;
        ShiftRates s1, s2;
        // a ray whose y1 and y2 are 0 adds nothing
        const bool live = (ya != 0.0 || yb != 0.0) && rw.init(g, origins, dirs, ray) && s1.init(rw, t1, ray) && s2.init(rw, t2, ray);
        const int mine = live ? rw.na : 0;
        int planes = 0;                                         // the wave's maximum of `mine`: one of the three extents
        if (__ballot(mine == g.nx)) planes = g.nx;
        if (__ballot(mine == g.ny)) planes = max(planes, g.ny);
        if (__ballot(mine == g.nz)) planes = max(planes, g.nz);
        for (int kappa = 0; kappa < planes; kappa++) {
            int c = 0;
            double fb = 0.0, fc = 0.0, w1[4] = {0.0, 0.0, 0.0, 0.0}, w2[4] = {0.0, 0.0, 0.0, 0.0};
            const bool counts = kappa < mine && rw.cell(kappa, c, fb, fc);
            if (counts) {
                s1.weights(fb, fc, w1);
                s2.weights(fb, fc, w2);
            }
            wave_add(v, counts ? c : -1, w1[0] * ya + w2[0] * yb);
            wave_add(v, counts ? c + rw.sb : -1, w1[1] * ya + w2[1] * yb);
            wave_add(v, counts ? c + rw.sc : -1, w1[2] * ya + w2[2] * yb);
            wave_add(v, counts ? c + rw.sb + rw.sc : -1, w1[3] * ya + w2[3] * yb);
        }
    }
}

// the deflection solver's rays: weight = w where g1, g2 and w are finite and w > 0, else 0; wg = weight g (0 at weight 0);
// counts the rays of positive weight that are no miss (their vectors included) and cross the grid
__global__ __launch_bounds__(kThreads) void tomo_deflect_rays_kernel(Grid g, const double *__restrict__ g1, const double *__restrict__ g2,
                                                                     const double *__restrict__ w, const double *__restrict__ origins,
                                                                     const double *__restrict__ dirs, const double *__restrict__ t1,
                                                                     const double *__restrict__ t2, long long n_rays,
                                                                     double *__restrict__ weight, double *__restrict__ wg1,
                                                                     double *__restrict__ wg2, unsigned long long *__restrict__ rays_used) {
    __shared__ double red[kThreads / 64];
    double count = 0.0;
    for (long long ray = (long long)blockIdx.x * kThreads + threadIdx.x; ray < n_rays; ray += (long long)gridDim.x * kThreads) {
        const double ga = g1[ray], gb = g2[ray], wi = w ? w[ray] : 1.0;
        const bool ok = isfinite(ga) && isfinite(gb) && isfinite(wi) && wi > 0.0;
        weight[ray] = ok ? wi : 0.0;
        wg1[ray] = ok ? wi * ga : 0.0;
        wg2[ray] = ok ? wi * gb : 0.0;
        RayWalk rw;
        ShiftRates s1, s2;
        bool used = false;
        if (ok && rw.init(g, origins, dirs, ray) && s1.init(rw, t1, ray) && s2.init(rw, t2, ray)) {
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

// |r|^2 for the host's check: one block
__global__ __launch_bounds__(kThreads) void tomo_sum_parts_kernel(const double *__restrict__ part, int n_parts, double *__restrict__ out) {
    __shared__ double red[kThreads / 64];
    const double s = sum_parts(part, n_parts, red);
    if (threadIdx.x == 0) *out = s;
}

// what all three entry points refuse about the grid and the rays
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

int launch_project(const Grid &g, const double *d_f, const double *d_origins, const double *d_dirs, long long n_rays, const double *d_weight,
                   double *d_p, hipStream_t stream) {
    hipLaunchKernelGGL(tomo_project_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_f, d_origins, d_dirs, n_rays,
                       d_weight, d_p);
    PH_CHECK(hipGetLastError());
    return 0;
}

int launch_backproject(const Grid &g, const double *d_y, const double *d_origins, const double *d_dirs, long long n_rays, double *d_v,
                       hipStream_t stream) {
    hipLaunchKernelGGL(tomo_backproject_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_y, d_origins, d_dirs, n_rays, d_v);
    PH_CHECK(hipGetLastError());
    return 0;
}

int launch_deflect(const Grid &g, const double *d_f, const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2,
                   long long n_rays, const double *d_weight, double *d_g1, double *d_g2, hipStream_t stream) {
    hipLaunchKernelGGL(tomo_deflect_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_f, d_origins, d_dirs, d_t1, d_t2,
                       n_rays, d_weight, d_g1, d_g2);
    PH_CHECK(hipGetLastError());
    return 0;
}

int launch_deflect_adjoint(const Grid &g, const double *d_y1, const double *d_y2, const double *d_origins, const double *d_dirs,
                           const double *d_t1, const double *d_t2, long long n_rays, double *d_v, hipStream_t stream) {
    hipLaunchKernelGGL(tomo_deflect_adjoint_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_y1, d_y2, d_origins, d_dirs,
                       d_t1, d_t2, n_rays, d_v);
    PH_CHECK(hipGetLastError());
    return 0;
}

// the device work vectors of one solve: r, q, s over the voxels; weight, t (and t2: the second component of section 10) over
// the rays; parts: 3 kMaxBlocks + 1; 2 counters
struct Work {
    double *r, *q, *s, *weight, *t, *t2, *parts;
    unsigned long long *counters;
};

// The operator pair of a solve.  An Op knows the grid, the rays and the data, and has
//   prepare(w, stream):  weight and the weighted data over the rays (w.weight, w.t[, w.t2]), the used rays in w.counters[0]
//   forward(q, w, stream):  w.t[, w.t2] = weight (Op q)
//   adjoint(w, v, stream):  v += Op^T (w.t[, w.t2])
// Section 9: the projector and the backprojector on the projections d_p.
struct ProjectionOp {
    Grid g;
    const double *d_p, *d_w, *d_origins, *d_dirs;
    long long n_rays;

    int prepare(const Work &w, hipStream_t stream) const {
        hipLaunchKernelGGL(tomo_rays_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_p, d_w, d_origins, d_dirs, n_rays,
                           w.weight, w.t, w.counters);
        PH_CHECK(hipGetLastError());
        return 0;
    }
    int forward(const double *q, const Work &w, hipStream_t stream) const {
        return launch_project(g, q, d_origins, d_dirs, n_rays, w.weight, w.t, stream);
    }
    int adjoint(const Work &w, double *v, hipStream_t stream) const { return launch_backproject(g, w.t, d_origins, d_dirs, n_rays, v, stream); }
};

// Section 10: the two shift derivatives on the deflections d_g1, d_g2.
struct DeflectionOp {
    Grid g;
    const double *d_g1, *d_g2, *d_w, *d_origins, *d_dirs, *d_t1, *d_t2;
    long long n_rays;

    int prepare(const Work &w, hipStream_t stream) const {
        hipLaunchKernelGGL(tomo_deflect_rays_kernel, dim3(ray_blocks(n_rays)), dim3(kThreads), 0, stream, g, d_g1, d_g2, d_w, d_origins, d_dirs,
                           d_t1, d_t2, n_rays, w.weight, w.t, w.t2, w.counters);
        PH_CHECK(hipGetLastError());
        return 0;
    }
    int forward(const double *q, const Work &w, hipStream_t stream) const {
        return launch_deflect(g, q, d_origins, d_dirs, d_t1, d_t2, n_rays, w.weight, w.t, w.t2, stream);
    }
    int adjoint(const Work &w, double *v, hipStream_t stream) const {
        return launch_deflect_adjoint(g, w.t, w.t2, d_origins, d_dirs, d_t1, d_t2, n_rays, v, stream);
    }
};

// CG on  m (Op^T W Op + reg G^T G) m x = m Op^T W data  from x = 0 (the iteration of section 9)
template <typename Op>
int solve(hipStream_t stream, const Op &op, const unsigned char *d_support, double reg, double tol, int max_iter, double *x, const Work &w,
          photon_tomo_stats_t *stats) {
    const Grid &g = op.g;
    const unsigned N = (unsigned)g.nx * (unsigned)g.ny * (unsigned)g.nz;
    const int blocks = (int)std::min<unsigned>(kMaxBlocks, (N + kThreads - 1) / kThreads);
    double *rho_part[2] = {w.parts, w.parts + kMaxBlocks};
    double *qs_part = w.parts + 2 * kMaxBlocks, *d_scalar = w.parts + 3 * kMaxBlocks;

    PH_CHECK(hipMemsetAsync(w.counters, 0, 2 * sizeof(unsigned long long), stream));
    PH_CHECK(hipMemsetAsync(w.r, 0, (size_t)N * sizeof(double), stream));
    PH_TRY(op.prepare(w, stream));
    PH_TRY(op.adjoint(w, w.r, stream));
    hipLaunchKernelGGL(cg_init_kernel, dim3(blocks), dim3(kThreads), 0, stream, N, d_support, x, w.r, w.q, rho_part[0], w.counters + 1);
    PH_CHECK(hipGetLastError());

    auto residual_sq = [&](const double *part, double *out) -> int {
        hipLaunchKernelGGL(tomo_sum_parts_kernel, dim3(1), dim3(kThreads), 0, stream, part, blocks, d_scalar);
        PH_CHECK(hipGetLastError());
        PH_CHECK(hipMemcpyAsync(out, d_scalar, sizeof(double), hipMemcpyDeviceToHost, stream));
        PH_CHECK(hipStreamSynchronize(stream));
        return 0;
    };
    double rr = 0.0;
    PH_TRY(residual_sq(rho_part[0], &rr));
    const double bnorm = std::sqrt(rr);

    int it = 0;
    if (bnorm > 0.0) {
        for (;;) {
            const int cur = it & 1, old = cur ^ 1;               // rho_part[cur] holds r.r after `it` iterations
            if (it % PHOTON_TOMO_CHECK_EVERY == 0) {
                if (it > 0) PH_TRY(residual_sq(rho_part[cur], &rr));
                if (tol > 0.0 && std::sqrt(rr) <= tol * bnorm) break;
            }
            if (it == max_iter) {
                if (it % PHOTON_TOMO_CHECK_EVERY != 0) PH_TRY(residual_sq(rho_part[cur], &rr));    // a run that stops between checks
                break;
            }
            PH_TRY(op.forward(w.q, w, stream));
            PH_CHECK(hipMemsetAsync(w.s, 0, (size_t)N * sizeof(double), stream));
            PH_TRY(op.adjoint(w, w.s, stream));
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

// what both solvers refuse about lambda, tol and max_iter
const char *solver_refusal(double lambda, double tol, int max_iter) {
    if (!(lambda >= 0.0)) return "lambda must be >= 0";
    if (!(tol >= 0.0)) return "tol must be >= 0";
    if (max_iter < 0) return "max_iter must be >= 0";
    return nullptr;
}

void refuse(const char *what, const char *bad, int nx, int ny, int nz, long long n_rays) {
    fprintf(stderr, "photon: %s: %s (%d x %d x %d voxels, %lld rays)\n", what, bad, nx, ny, nz, n_rays);
}

}  // namespace

extern "C" int photon_tomo_project(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                   const double *d_origins, const double *d_dirs, long long n_rays, double *d_p, void *stream) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad && (!d_f || !d_origins || !d_dirs || !d_p)) bad = "null d_f, d_origins, d_dirs or d_p";
    if (bad) {
        refuse("photon_tomo_project", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return launch_project(make_grid(nx, ny, nz, spacing, origin), d_f, d_origins, d_dirs, n_rays, nullptr, d_p, (hipStream_t)stream);
}

extern "C" int photon_tomo_backproject(const double *d_y, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                       const double *d_origins, const double *d_dirs, long long n_rays, double *d_v, void *stream) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad && (!d_y || !d_origins || !d_dirs || !d_v)) bad = "null d_y, d_origins, d_dirs or d_v";
    if (bad) {
        refuse("photon_tomo_backproject", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return launch_backproject(make_grid(nx, ny, nz, spacing, origin), d_y, d_origins, d_dirs, n_rays, d_v, (hipStream_t)stream);
}

extern "C" int photon_tomo_reconstruct(const double *d_p, const double *d_w, const unsigned char *d_support, int nx, int ny, int nz,
                                       const double spacing[3], const double origin[3], const double *d_origins, const double *d_dirs,
                                       long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                                       photon_tomo_stats_t *stats, void *stream_p) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad) bad = solver_refusal(lambda, tol, max_iter);
    if (!bad && (!d_p || !d_origins || !d_dirs || !d_f)) bad = "null d_p, d_origins, d_dirs or d_f";
    if (bad) {
        refuse("photon_tomo_reconstruct", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return guarded("photon_tomo_reconstruct", [&]() -> int {
        hipStream_t stream = (hipStream_t)stream_p;
        const size_t N = (size_t)nx * ny * nz;
        PoolBuffer<double> r, q, s, weight, t, parts;
        PoolBuffer<unsigned long long> counters;
        PH_CHECK(r.alloc(N));
        PH_CHECK(q.alloc(N));
        PH_CHECK(s.alloc(N));
        PH_CHECK(weight.alloc((size_t)n_rays));
        PH_CHECK(t.alloc((size_t)n_rays));
        PH_CHECK(parts.alloc(3 * kMaxBlocks + 1));
        PH_CHECK(counters.alloc(2));
        const double h = std::min(spacing[0], std::min(spacing[1], spacing[2]));
        const ProjectionOp op{make_grid(nx, ny, nz, spacing, origin), d_p, d_w, d_origins, d_dirs, n_rays};
        const int rc = solve(stream, op, d_support, lambda * (h * h), tol, max_iter, d_f,
                             Work{r.p, q.p, s.p, weight.p, t.p, nullptr, parts.p, counters.p}, stats);
        if (rc) (void)hipStreamSynchronize(stream);          // the blocks go back to the cache: nothing may still use them
        return rc;
    });
}

// ---- section 10 --------------------------------------------------------------------------------------------------------------
extern "C" int photon_tomo_deflect(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                   const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2, long long n_rays,
                                   double *d_g1, double *d_g2, void *stream) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad && (!d_f || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_g1 || !d_g2)) bad = "null d_f, d_origins, d_dirs, d_t1, d_t2, d_g1 or d_g2";
    if (bad) {
        refuse("photon_tomo_deflect", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return launch_deflect(make_grid(nx, ny, nz, spacing, origin), d_f, d_origins, d_dirs, d_t1, d_t2, n_rays, nullptr, d_g1, d_g2,
                          (hipStream_t)stream);
}

extern "C" int photon_tomo_deflect_adjoint(const double *d_y1, const double *d_y2, int nx, int ny, int nz, const double spacing[3],
                                           const double origin[3], const double *d_origins, const double *d_dirs, const double *d_t1,
                                           const double *d_t2, long long n_rays, double *d_v, void *stream) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad && (!d_y1 || !d_y2 || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_v)) bad = "null d_y1, d_y2, d_origins, d_dirs, d_t1, d_t2 or d_v";
    if (bad) {
        refuse("photon_tomo_deflect_adjoint", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return launch_deflect_adjoint(make_grid(nx, ny, nz, spacing, origin), d_y1, d_y2, d_origins, d_dirs, d_t1, d_t2, n_rays, d_v,
                                  (hipStream_t)stream);
}

extern "C" int photon_tomo_reconstruct_deflections(const double *d_g1, const double *d_g2, const double *d_w, const unsigned char *d_support,
                                                   int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                                   const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2,
                                                   long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                                                   photon_tomo_stats_t *stats, void *stream_p) {
    const char *bad = grid_refusal(nx, ny, nz, spacing, origin, n_rays);
    if (!bad) bad = solver_refusal(lambda, tol, max_iter);
    if (!bad && (!d_g1 || !d_g2 || !d_origins || !d_dirs || !d_t1 || !d_t2 || !d_f)) bad = "null d_g1, d_g2, d_origins, d_dirs, d_t1, d_t2 or d_f";
    if (bad) {
        refuse("photon_tomo_reconstruct_deflections", bad, nx, ny, nz, n_rays);
        return 1;
    }
    return guarded("photon_tomo_reconstruct_deflections", [&]() -> int {
        hipStream_t stream = (hipStream_t)stream_p;
        const size_t N = (size_t)nx * ny * nz;
        PoolBuffer<double> r, q, s, weight, t, t2, parts;
        PoolBuffer<unsigned long long> counters;
        PH_CHECK(r.alloc(N));
        PH_CHECK(q.alloc(N));
        PH_CHECK(s.alloc(N));
        PH_CHECK(weight.alloc((size_t)n_rays));
        PH_CHECK(t.alloc((size_t)n_rays));
        PH_CHECK(t2.alloc((size_t)n_rays));
        PH_CHECK(parts.alloc(3 * kMaxBlocks + 1));
        PH_CHECK(counters.alloc(2));
        const DeflectionOp op{make_grid(nx, ny, nz, spacing, origin), d_g1, d_g2, d_w, d_origins, d_dirs, d_t1, d_t2, n_rays};
        // no h^2: D carries 1 / length against A, so lambda weighs G^T G as it does in section 9
        const int rc = solve(stream, op, d_support, lambda, tol, max_iter, d_f,
                             Work{r.p, q.p, s.p, weight.p, t.p, t2.p, parts.p, counters.p}, stats);
        if (rc) (void)hipStreamSynchronize(stream);          // the blocks go back to the cache: nothing may still use them
        return rc;
    });
}
