// photon_flow.hip - a steady velocity field on a grid in HBM, and the PIV particle field of photon_sources_piv advected
// through it: frame 2 (3, ...) of a PIV pair with the particles of frame 1 moved by a known flow.
//
// The field is one float4 {u, v, w, 0} per node.  A trilinear sample reads 8 nodes: as float4 that is 8 16-byte loads
// (global_load_dwordx4), all three components of a node in one; as three f32 arrays it would be 24 4-byte loads and three
// times the address arithmetic.  The fourth word costs a third more bytes, which a 128^3 field (32 MiB) spends in the
// last-level cache anyway.
#include <algorithm>
#include <cmath>
#include <vector>

#include "photon_internal.hpp"
#include "piv_field.hpp"

using namespace photon;

struct photon_flow {
    int n[3] = {0, 0, 0};               // nodes along x, y, z
    double spacing[3] = {0, 0, 0}, origin[3] = {0, 0, 0};
    DeviceBuffer<float4> uvw;           // [nz][ny][nx], x fastest
};

struct FlowDev {
    const float4 *__restrict__ uvw;
    int n[3];
    double spacing[3], origin[3];
};

// One axis of the trilinear sample, in the order include/parallel_ray_tracing.h spells out: f = (p - origin) / spacing,
// cell c = floor(f) clamped to [0, n - 2] (a NaN goes to 0), weight f - c clamped to [0, 1] (a NaN to 0).
static __device__ inline int flow_axis(double p, double origin, double spacing, int n, double &t) {
    const double f = (p - origin) / spacing;
    double c = floor(f);
    c = c >= 0.0 ? c : 0.0;
    c = c <= (double)(n - 2) ? c : (double)(n - 2);
    t = f - c;
    t = t > 0.0 ? t : 0.0;
    t = t < 1.0 ? t : 1.0;
    return (int)c;
}

static __device__ inline double lerp64(double a, double b, double t) { return a + t * (b - a); }

// velocity at (x, y, z): lerps along x (corner rows j, k = 00, 10, 01, 11), then along y, then along z
static __device__ inline void flow_sample(const FlowDev &g, double x, double y, double z, double &u, double &v, double &w) {
    double tx, ty, tz;
    const int i = flow_axis(x, g.origin[0], g.spacing[0], g.n[0], tx);
    const int j = flow_axis(y, g.origin[1], g.spacing[1], g.n[1], ty);
    const int k = flow_axis(z, g.origin[2], g.spacing[2], g.n[2], tz);
    const long long sy = g.n[0], sz = (long long)g.n[0] * g.n[1];
    const float4 *p = g.uvw + (long long)k * sz + (long long)j * sy + i;
    const float4 c000 = p[0], c100 = p[1], c010 = p[sy], c110 = p[sy + 1];
    const float4 c001 = p[sz], c101 = p[sz + 1], c011 = p[sz + sy], c111 = p[sz + sy + 1];
#define PH_TRILERP(m)                                                                               \
    lerp64(lerp64(lerp64(c000.m, c100.m, tx), lerp64(c010.m, c110.m, tx), ty),                      \
           lerp64(lerp64(c001.m, c101.m, tx), lerp64(c011.m, c111.m, tx), ty), tz)
    u = PH_TRILERP(x);
    v = PH_TRILERP(y);
    w = PH_TRILERP(z);
#undef PH_TRILERP
}

// One classical RK4 step of h through the steady field (the order the header gives):
//   k1 = V(p), k2 = V(p + (h/2) k1), k3 = V(p + (h/2) k2), k4 = V(p + h k3), p += (h/6) (((k1 + 2 k2) + 2 k3) + k4)
static __device__ inline void rk4_step(const FlowDev &g, double h, double &X, double &Y, double &Z) {
    const double hh = 0.5 * h, h6 = h / 6.0;
    double u1, v1, w1, u2, v2, w2, u3, v3, w3, u4, v4, w4;
    flow_sample(g, X, Y, Z, u1, v1, w1);
    flow_sample(g, X + hh * u1, Y + hh * v1, Z + hh * w1, u2, v2, w2);
    flow_sample(g, X + hh * u2, Y + hh * v2, Z + hh * w2, u3, v3, w3);
    flow_sample(g, X + h * u3, Y + h * v3, Z + h * w3, u4, v4, w4);
    X = X + h6 * (u1 + 2.0 * u2 + 2.0 * u3 + u4);
    Y = Y + h6 * (v1 + 2.0 * v2 + 2.0 * v3 + v4);
    Z = Z + h6 * (w1 + 2.0 * w2 + 2.0 * w3 + w4);
}

// NaN-propagating max / min: the extent of a field with a NaN particle is NaN, and then left unset
static __host__ __device__ inline float pmax(float a, float b) { return (a != a || a > b) ? a : b; }
static __host__ __device__ inline float pmin(float a, float b) { return (a != a || a < b) ? a : b; }

static constexpr int kBlock = 256;

// Particle i of photon_sources_piv, moved by `steps` RK4 steps of h, stored like that generator stores it.  Each block also
// writes {max |x|, max |y|, min z, max z} of the f32 coordinates it stored to partial[blockIdx.x] (the sources' extent).
__global__ __launch_bounds__(kBlock) void sources_piv_advected_kernel(unsigned long long seed, long long n, PivFieldDev f,
                                                                      const double *__restrict__ diameter_cdf, FlowDev g, double h,
                                                                      int steps, float *sx, float *sy, float *sz, double *srad,
                                                                      int *sdia, double *world, float4 *partial) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float4 e = make_float4(0.f, 0.f, INFINITY, -INFINITY);
    if (i < n) {
        double X, Y, Z, ud;
        piv_draw(seed, i, f, X, Y, Z, ud);
        for (int s = 0; s < steps; s++) rk4_step(g, h, X, Y, Z);
        piv_store(i, f, X, Y, Z, ud, diameter_cdf, sx, sy, sz, srad, sdia);
        if (world) {
            world[3 * i] = X;
            world[3 * i + 1] = Y;
            world[3 * i + 2] = Z;
        }
        const float z = (float)(Z + f.z_object);
        e = make_float4(fabsf((float)X), fabsf((float)Y), z, z);
    }
    __shared__ float4 red[kBlock];
    red[threadIdx.x] = e;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off /= 2) {
        if ((int)threadIdx.x < off) {
            const float4 a = red[threadIdx.x], b = red[threadIdx.x + off];
            red[threadIdx.x] = make_float4(pmax(a.x, b.x), pmax(a.y, b.y), pmin(a.z, b.z), pmax(a.w, b.w));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

extern "C" {

int photon_flow_from_grid(const float *u, const float *v, const float *w, int nx, int ny, int nz, const double spacing[3],
                          const double origin[3], photon_flow_t **out) {
    bool ok = out && u && v && w && spacing && origin && nx >= 2 && ny >= 2 && nz >= 2 &&
              (long long)nx * ny * nz <= 0x7fffffffLL;
    for (int a = 0; ok && a < 3; a++) ok = std::isfinite(spacing[a]) && spacing[a] > 0 && std::isfinite(origin[a]);
    if (!ok) {
        fprintf(stderr, "photon: photon_flow_from_grid: bad arguments\n");
        return 1;
    }
    return guarded("photon_flow_from_grid", [&]() -> int {
        const size_t nodes = (size_t)nx * ny * nz;
        std::vector<float4> host(nodes);
        for (size_t q = 0; q < nodes; q++) host[q] = make_float4(u[q], v[q], w[q], 0.f);
        std::unique_ptr<photon_flow> flow(new photon_flow());
        flow->n[0] = nx; flow->n[1] = ny; flow->n[2] = nz;
        for (int a = 0; a < 3; a++) { flow->spacing[a] = spacing[a]; flow->origin[a] = origin[a]; }
        if (flow->uvw.alloc(nodes) != hipSuccess) {
            fprintf(stderr, "photon: photon_flow_from_grid: device allocation failed\n");
            return 3;
        }
        if (hipMemcpy(flow->uvw.p, host.data(), nodes * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess) return 4;
        *out = flow.release();
        return 0;
    });
}

void photon_flow_free(photon_flow_t *flow) { delete flow; }

int photon_sources_piv_advected(uint64_t seed, long long n, const double box_min[3], const double box_max[3], double z_object,
                                double beam_fwhm, double irradiance_constant, const double *diameter_cdf, int n_diameters,
                                const photon_flow_t *flow, double t, int steps, double *world_xyz, photon_sources_t **out) {
    if (!out || n < 0 || n > 0x7fffffffLL || !box_min || !box_max || !(beam_fwhm > 0) || n_diameters < 0 ||
        (n_diameters > 0 && !diameter_cdf) || steps < 1 || !std::isfinite(t) || (t != 0 && !flow)) {
        fprintf(stderr, "photon: photon_sources_piv_advected: bad arguments\n");
        return 1;
    }
    const auto alloc_failed = [](const char *what) {
        fprintf(stderr, "photon: photon_sources_piv_advected: device allocation failed (%s)\n", what);
        return 3;
    };
    return guarded("photon_sources_piv_advected", [&]() -> int {
        std::unique_ptr<photon_sources> src;
        PH_TRY(sources_alloc(n, &src));
        const PivFieldDev f = piv_field_setup(box_min, box_max, z_object, beam_fwhm, irradiance_constant, n_diameters);
        FlowDev g{};
        const bool moving = flow && t != 0;             // flow == NULL or t == 0: the frame of photon_sources_piv itself
        if (moving) {
            g.uvw = flow->uvw.p;
            for (int a = 0; a < 3; a++) { g.n[a] = flow->n[a]; g.spacing[a] = flow->spacing[a]; g.origin[a] = flow->origin[a]; }
        }
        const double h = moving ? t / steps : 0.0;
        const int run_steps = moving ? steps : 0;
        const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
        DeviceBuffer<double> d_cdf, d_world;
        DeviceBuffer<float4> d_partial;
        if (n_diameters > 0) {
            if (d_cdf.alloc((size_t)n_diameters) != hipSuccess) return alloc_failed("diameter table");
            if (hipMemcpy(d_cdf.p, diameter_cdf, n_diameters * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 4;
        }
        std::vector<float4> partial(blocks);
        if (n) {
            if (d_partial.alloc(blocks) != hipSuccess) return alloc_failed("extent partials");
            if (world_xyz && d_world.alloc((size_t)n * 3) != hipSuccess) return alloc_failed("world positions");
            hipLaunchKernelGGL(sources_piv_advected_kernel, dim3(blocks), dim3(kBlock), 0, 0, (unsigned long long)seed, n, f, d_cdf.p,
                               g, h, run_steps, src->x.p, src->y.p, src->z.p, src->radiance.p, src->diameter_index.p, d_world.p, d_partial.p);
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
            if (hipMemcpy(partial.data(), d_partial.p, blocks * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return 4;
            if (world_xyz &&
                hipMemcpy(world_xyz, d_world.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 4;
        }
        // the extent of the particles as stored -- not the box they were drawn from, which they may have left
        if (n) {
            float4 e = partial[0];
            for (unsigned b = 1; b < blocks; b++)
                e = make_float4(pmax(e.x, partial[b].x), pmax(e.y, partial[b].y), pmin(e.z, partial[b].z), pmax(e.w, partial[b].w));
            sources_set_extent(src.get(), e.x, e.y, e.z, e.w);
        }
        *out = src.release();
        return 0;
    });
}

}  // extern "C"
