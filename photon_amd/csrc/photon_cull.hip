// photon_cull.hip - what a launch may leave out and the plan a trace makes of it: the lens samples that cannot reach the first
// aperture, the sources whose image cannot fall on the sensor, the doomed rays of a march, lens-major order.  The geometry
// behind each cull, the rules for when it may be used (make_trace_plan: once per trace) and the ranges a trace is cut into
// (next_launch).  Host code but for source_cull_kernel, which runs once per scene.
#include <algorithm>
#include <cmath>

#include "photon_internal.hpp"

using namespace photon;

// The lens samples that CAN reach the aperture of the first element from some source of this scene.  The reference kills a
// ray whose hit on that element's front surface (a sphere, 'l', or a plane, 't') lies more than pitch / 2 from the axis
// (.cu:447, 560-566), and aims ray k of every source at the SAME point P_k = (x_lens, y_lens) of the plane z = image_distance
// (.cu:123-141: x(z) = x_s + tan(theta) (z_s - z) with tan(theta) = -(x_lens - x_s) / (image_distance - z_s)), with
// |P_k| up to ratio x pitch: a full-aperture cone loses half its rays there, the same ones for every source.  A ray through P_k
// that hit the surface at axis distance rho <= pitch / 2 and height z_h would have |P_k| <= rho + |z_h - z_a| slope, its slope
// at most (|P_k| + R) / D (R: largest axis distance of a source, D: smallest source-plane distance along z) and z_h within dz
// of the plane (the element's vertex plane +- its sag at pitch / 2).  So sample k is DEAD for every source when
//     |P_k| (1 - dz / D) - dz R / D > pitch / 2 + slack        (slack: a thousandth of the pitch, for the f32 rounding of the aim)
// and only the others are launched where nothing else needs the dead rays (make_trace_plan: no volume, no dumps, reference element
// path).  Everything in double, from the caller's arrays -- or, for sources generated on the device, from the box the generator
// drew them from; geometries this does not cover (tilted or off-axis element, generated BOS patterns, a degenerate sphere)
// return every sample.
std::vector<int> photon::live_lens_samples(const std::vector<float> &lx, const std::vector<float> &ly, const lightfield_source_t *lsp,
                                           const photon_sources *generated, size_t n_sources, float image_distance, int num_elements,
                                           const element_data_t *edp, const double (*center)[3], const double (*plane)[4]) {
    std::vector<int> all(lx.size());
    for (size_t k = 0; k < all.size(); k++) all[k] = (int)k;
    if ((generated && !generated->have_extent) || n_sources == 0 || num_elements < 1 || lx.size() < 2) return all;
    const char type = edp[0].element_type;
    const double pitch = edp[0].element_geometry.pitch;
    if ((type != 'l' && type != 't') || !(pitch > 0)) return all;
    // (the dz bound below puts the front vertex on the +z side of the centre: plane normal c > 0, what the reference's Python always
    // emits, perform_ray_tracing_03.py:49; a flipped normal moves the front sphere, .cu:557 -- leave that to the kernels)
    if (plane[0][0] != 0.0 || plane[0][1] != 0.0 || !(plane[0][2] > 0.0) || center[0][0] != 0.0 || center[0][1] != 0.0) return all;
    const double za = image_distance;
    double dz;
    if (type == 't') {
        dz = fabs(-plane[0][3] / plane[0][2] - za);
    } else {
        const double R = fabs((double)edp[0].element_geometry.front_surface_radius), t = fabs(edp[0].element_geometry.vertex_distance);
        if (!(R > pitch / 2) || !(t == t)) return all;
        const double sag = R - sqrt(R * R - pitch * pitch / 4);
        dz = fabs(center[0][2] - za) + t / 2 + sag;
    }
    double rmax = 0, dmin = HUGE_VAL;
    if (generated) {                                                    // sources made on the device: the generator's box stands in for them
        rmax = generated->rmax;
        dmin = za < generated->zmin ? generated->zmin - za : (za > generated->zmax ? za - generated->zmax : 0.0);
    } else
    {                                                                   // (one sqrt at the end: this loop runs per start_ray_tracing call)
        double r2max = 0, nan_probe = 0;
        for (size_t i = 0; i < n_sources; i++) {
            const double x = lsp->x[i], y = lsp->y[i], r2 = x * x + y * y, dd = fabs(za - (double)lsp->z[i]);
            nan_probe += r2 * 0.0 + dd * 0.0;                           // NaN (or infinity) anywhere -> NaN
            r2max = r2 > r2max ? r2 : r2max;
            dmin = dd < dmin ? dd : dmin;
        }
        if (!(nan_probe == 0.0)) return all;                           // a NaN source: leave everything to the kernels
        rmax = sqrt(r2max);
    }
    if (!(dz == dz) || !(dmin > 16 * dz)) return all;
    std::vector<int> live;
    for (size_t k = 0; k < lx.size(); k++) {
        const double r = sqrt((double)lx[k] * lx[k] + (double)ly[k] * ly[k]);
        const bool dead = r * (1 - dz / dmin) - dz * rmax / dmin > pitch / 2 + 1e-3 * pitch + 1e-4 * r;
        if (!dead) live.push_back((int)k);
    }
    if (live.empty()) live.push_back(0);                                // a launch of zero rays per source is nobody's friend
    return live;
}

// The sources whose image CANNOT fall on the sensor, whatever lens sample the ray is aimed at: they need not be launched on the
// volume-free path.  photon's sample PIV frame draws its particles over a field 1.5 x wider than the camera sees
// (run_simulation_02.py:956-958): more than half of them image beside the sensor.
//
// One biconvex thick lens ('l', on the z axis, normal +z) -- or one thin lens ('t': lens_cull_setup) --, then the sensor plane z = z_sensor.  Everything a surviving ray
// does is, in the xy plane, a linear combination of two vectors -- its aim point P on the plane z = image_distance (.cu:123-141)
// and its source's S = (x_s, y_s) -- with SCALAR coefficients, because the lens is rotationally symmetric and every surface
// normal's xy part is the hit point's over the radius:
//     H1 = (1 + e) P - e S                     front hit;  e = (z_H1 - z_a) / (z_a - z_s), z_H1 within the front sag of the vertex
//     n v = u - a1 H1,   u = q (P - S)         Snell in vector form (.cu:652-682); q = 1 / |P - S| (3-D), a1 = G1 / R1,
//                                              G1 = n cos(t') - cos(t) = sqrt(n^2 - sin^2 t) - cos t: n - 1 at normal incidence, growing with t
//     H2 = H1 + s2 v                           back hit; s2 = glass path = (z_H1 - z_H2) / |v_z|
//     w  = n v - a2 H2                         a2 = G2 / |R2|, G2 = n cos(t) - cos(t') likewise from n - 1 upwards (.cu:797-827)
//     h  = H2 + tau w                          sensor hit; tau = (z_H2 - z_sensor) / |w_z|
// so h = A P + B S with A, B polynomials in (e, q, a1, a2, s2, tau).  Each of the six lies in an interval that follows from the
// aperture tests alone (both hits within pitch / 2 of the axis, .cu:560-566, 737-743: a ray that fails one is dead anyway):
// sin(incidence) <= |u_xy| + (pitch / 2) / R, the sags of the two caps, |v_xy| and |w_xy| from the same sums.  A and B are
// evaluated in interval arithmetic; |P| <= the largest lens sample, and for a ray that passes the front aperture also
// <= (pitch / 2 + |e| r_s) / (1 - |e|).  The source is OFF when the box  B S +- |A|max |P|max +- slack  misses the rectangle of
// sensor hits that reach a pixel (.cu:1440-1452, 1803-1815: half a pixel beyond the array either side; one more pixel here).
// slack: 10 um + 1e-5 of the ray's length for the kernels' f32 arithmetic (its cancellation in the sphere intersection is worth
// 1.5 um along the ray, tests/test_oracle_golden.py).  Held against exact f64 ray tracing of every ray of every culled source in
// tests/test_parity_gpu.py::test_culled_sources_against_exact_geometry; geometries this does not cover keep every source.
namespace {
#define PH_HD __host__ __device__ inline
PH_HD double dmin2(double a, double b) { return a < b ? a : b; }
PH_HD double dmax2(double a, double b) { return a > b ? a : b; }
struct Ivl {
    double lo, hi;
};
PH_HD Ivl iv(double a) { return Ivl{a, a}; }
PH_HD Ivl iv(double a, double b) { return a <= b ? Ivl{a, b} : Ivl{b, a}; }
PH_HD Ivl operator+(Ivl a, Ivl b) { return Ivl{a.lo + b.lo, a.hi + b.hi}; }
PH_HD Ivl operator-(Ivl a) { return Ivl{-a.hi, -a.lo}; }
PH_HD Ivl operator-(Ivl a, Ivl b) { return a + (-b); }
PH_HD Ivl operator*(Ivl a, Ivl b) {
    const double c0 = a.lo * b.lo, c1 = a.lo * b.hi, c2 = a.hi * b.lo, c3 = a.hi * b.hi;
    return Ivl{dmin2(dmin2(c0, c1), dmin2(c2, c3)), dmax2(dmax2(c0, c1), dmax2(c2, c3))};
}
PH_HD Ivl operator*(Ivl a, double b) { return a * iv(b); }
PH_HD double mag(Ivl a) { return dmax2(fabs(a.lo), fabs(a.hi)); }

}  // namespace

photon::LensCull photon::lens_cull_setup(const std::vector<float> &lx, const std::vector<float> &ly, float image_distance, float beam_wavelength,
                                         int num_elements, const element_data_t *edp, const double (*center)[3], const double (*plane)[4],
                                         const int *sys_index, const camera_design_t *cam) {
    photon::LensCull c;
    if (num_elements < 1 || (edp[0].element_type != 'l' && edp[0].element_type != 't')) return c;
    // the reference's element path sends the ray through element 0 once per single-member group (.cu:1331-1333): exactly once here
    {
        const int n = std::min(num_elements, kMaxElements);
        int seq = 0, applications = 0;
        for (int k = 0; k < n; k++) seq = std::max(seq, sys_index[k]);
        for (int idx = 0; idx < seq; idx++) {
            int count = 0;
            for (int k = 0; k < n; k++) count += (seq - sys_index[k] == idx);
            applications += count == 1;
        }
        if (applications != 1) return c;
    }
    if (plane[0][0] != 0.0 || plane[0][1] != 0.0 || !(plane[0][2] > 0.0) || center[0][0] != 0.0 || center[0][1] != 0.0) return c;
    const element_data_t &e = edp[0];
    if (e.element_type == 't') {
        // Thin lens: the ray meets the element's plane at H, within pitch / 2 of the axis, and leaves along u - (H - C) / f
        // (.cu:447-503).  With the centre ON the plane the z component of that is u's, so the sensor hit is
        //     h = H (1 - s / f) + s u_xy,   s = (z_plane - z_sensor) / |u_z|,   H = (1 + e) P - e S,  e = (z_plane - z_a) / (z_a - z_s):
        // exact up to the one quantity that depends on P, |P - S| in s / f (source_misses_sensor: an interval again).
        c.thin = true;
        c.focal = (double)(float)e.element_properties.thin_lens_focal_length;
        c.hp = (double)(float)e.element_geometry.pitch / 2.0;
        const double z_plane = -plane[0][3] / plane[0][2];
        if (!(c.focal > 0) || !(c.hp > 0) || !(fabs(z_plane - center[0][2]) <= 1e-9 * fabs(z_plane) + 1e-9)) return c;
        c.za = image_distance;
        c.zf = c.zb = z_plane;
        c.z_sen = cam->z_sensor;
        c.t = c.sag1 = c.sag2 = 0; c.R1 = c.R2a = 0; c.n = 1;
        if (!(c.zb > c.z_sen) || !(cam->pixel_pitch > 0)) return c;
        double rp = 0;
        for (size_t k = 0; k < lx.size(); k++) rp = std::max(rp, sqrt((double)lx[k] * lx[k] + (double)ly[k] * ly[k]));
        c.rp_all = rp * (1 + 1e-6);
        c.half_x = (double)cam->pixel_pitch * (cam->x_pixel_number + 1) / 2.0 + cam->pixel_pitch;
        c.half_y = (double)cam->pixel_pitch * (cam->y_pixel_number + 1) / 2.0 + cam->pixel_pitch;
        c.ok = c.za == c.za && c.zf == c.zf && c.half_x == c.half_x && c.half_y == c.half_y;
        return c;
    }
    c.R1 = e.element_geometry.front_surface_radius;
    c.R2a = -(double)e.element_geometry.back_surface_radius;
    c.hp = (double)(float)e.element_geometry.pitch / 2.0;                // the kernels compare against the f32 pitch
    c.t = e.element_geometry.vertex_distance;
    double n = e.element_properties.refractive_index;
    const double abbe = (float)e.element_properties.abbe_number;
    if (abbe == abbe) {                                                 // .cu:622-636: the index at the beam's wavelength
        const double lD = 589.3, lF = 486.1, lC = 656.3, w = beam_wavelength;
        n = n + (1.0 / (w * w) - 1.0 / (lD * lD)) * ((n - 1) / (abbe * (1 / (lF * lF) - 1 / (lC * lC))));
    }
    c.n = n;
    if (!(c.R1 > 0) || !(c.R2a > 0) || !(n > 1.0) || !(n < 4.0) || !(c.hp > 0) || !(c.t >= 0)) return c;
    if (!(c.hp < 0.95 * c.R1) || !(c.hp < 0.95 * c.R2a)) return c;
    c.za = image_distance;
    c.zf = center[0][2] + c.t / 2;
    c.zb = center[0][2] - c.t / 2;
    c.z_sen = cam->z_sensor;
    c.sag1 = c.R1 - sqrt(c.R1 * c.R1 - c.hp * c.hp);
    c.sag2 = c.R2a - sqrt(c.R2a * c.R2a - c.hp * c.hp);
    if (!(c.zb > c.z_sen) || !(cam->pixel_pitch > 0)) return c;
    // the two caps must not meet inside the aperture (the glass path of a surviving ray is then >= 0, which the bound on H2 uses);
    // photon's own lens has t = sag1 + sag2 exactly (run_simulation_02.py: zero edge thickness), hence the tolerance
    if (!(c.t >= 0.999 * (c.sag1 + c.sag2))) return c;
    double rp = 0;
    for (size_t k = 0; k < lx.size(); k++) rp = std::max(rp, sqrt((double)lx[k] * lx[k] + (double)ly[k] * ly[k]));
    c.rp_all = rp * (1 + 1e-6);
    c.half_x = (double)cam->pixel_pitch * (cam->x_pixel_number + 1) / 2.0 + cam->pixel_pitch;
    c.half_y = (double)cam->pixel_pitch * (cam->y_pixel_number + 1) / 2.0 + cam->pixel_pitch;
    c.ok = c.za == c.za && c.zf == c.zf && c.half_x == c.half_x && c.half_y == c.half_y;
    return c;
}

// true: no ray of the source (xs, ys, zs) that passes both apertures of the lens can reach a pixel
__host__ __device__ static bool source_misses_sensor(const photon::LensCull &c, double xs, double ys, double zs) {
    const double Ds = zs - c.za;
    if (!(Ds > 0) || !(zs > c.zf + (c.zf - c.zb))) return false;
    const double rs = sqrt(xs * xs + ys * ys);
    if (!(rs == rs)) return false;
    if (c.thin) {
        if (!(zs > c.zf + 1e-3 * Ds)) return false;
        const double e = -(c.zf - c.za) / Ds;                           // exact: the hit lies ON the plane
        if (!(fabs(e) < 0.25)) return false;
        const double rp = dmin2(c.rp_all, (c.hp + fabs(e) * rs) / (1 - fabs(e)));
        const double gmax = rs + rp, gmin = dmax2(0.0, rs - rp);
        // s / f = (z_plane - z_sensor) |P - S| / ((z_s - z_a) f): the flight to the sensor in units of the focal length
        const double k0 = (c.zf - c.z_sen) / (Ds * c.focal);
        const Ivl sig = iv(k0 * sqrt(gmin * gmin + Ds * Ds), k0 * sqrt(gmax * gmax + Ds * Ds));
        const double m1 = (c.zf - c.z_sen) / Ds;                        // s u_xy = m1 (P - S), exactly
        const Ivl one_sig = iv(1.0) - sig;
        const Ivl A = one_sig * (1 + e) + iv(m1), B = one_sig * (-e) - iv(m1);
        const double blur = mag(A) * rp + 1e-5 * (Ds + (c.zf - c.z_sen)) + 10.0;
        if (!(blur == blur)) return false;
        const Ivl bx = B * xs, by = B * ys;
        return bx.lo - blur > c.half_x || bx.hi + blur < -c.half_x || by.lo - blur > c.half_y || by.hi + blur < -c.half_y;
    }
    const Ivl e = iv(-(c.zf - c.za) / Ds, -(c.zf - c.sag1 - c.za) / Ds);
    const double em = mag(e);
    if (!(em < 0.25)) return false;
    const double rp = dmin2(c.rp_all, (c.hp + em * rs) / (1 - em));
    const double gmax = rs + rp, gmin = dmax2(0.0, rs - rp);
    const double lmax = sqrt(gmax * gmax + Ds * Ds);
    const Ivl q = iv(1.0 / lmax, 1.0 / sqrt(gmin * gmin + Ds * Ds));
    const double su = gmax / lmax;                                      // |u_xy| at most
    const double s1 = su + c.hp / c.R1;                                 // sin(incidence at the front) at most
    if (!(s1 < 0.9)) return false;
    const Ivl a1 = iv(c.n - 1, sqrt(c.n * c.n - s1 * s1) - sqrt(1 - s1 * s1)) * (1.0 / c.R1);
    const double sv = (su + a1.hi * c.hp) / c.n;                        // |v_xy| at most
    const double s2m = sv + c.hp / c.R2a;                               // sin(incidence at the back, in the glass) at most
    if (!(c.n * s2m < 0.9)) return false;
    const Ivl a2 = iv(c.n - 1, sqrt(c.n * c.n - c.n * c.n * s2m * s2m) - sqrt(1 - c.n * c.n * s2m * s2m)) * (1.0 / c.R2a);
    const Ivl s2 = iv(dmax2(0.0, c.t - c.sag1 - c.sag2), c.t / sqrt(1 - sv * sv));
    const double sw = c.n * sv + a2.hi * c.hp;                          // |w_xy| at most
    if (!(sw < 0.9)) return false;
    const Ivl tau = iv(c.zb - c.z_sen, (c.zb + c.sag2 - c.z_sen) / sqrt(1 - sw * sw));
    const Ivl one_e = iv(1.0) + e;
    const Ivl cP = q - a1 * one_e, cS = a1 * e - q;                     // n v = cP P + cS S
    const Ivl hP = one_e + s2 * cP * (1.0 / c.n), hS = s2 * cS * (1.0 / c.n) - e;      // H2 = hP P + hS S
    const Ivl k = iv(1.0) - tau * a2;
    const Ivl A = k * hP + tau * cP, B = k * hS + tau * cS;
    const double blur = mag(A) * rp + 1e-5 * (Ds + tau.hi) + 10.0;
    if (!(blur == blur)) return false;
    const Ivl bx = B * xs, by = B * ys;
    return bx.lo - blur > c.half_x || bx.hi + blur < -c.half_x || by.lo - blur > c.half_y || by.hi + blur < -c.half_y;
}

// One thread per source: the same bound on the device, over the scene's uploaded (or generated) source arrays -- 120 000 sources
// cost the host 5 ms per start_ray_tracing call (more than the BOS sample image's trace), the device a few microseconds.
__global__ __launch_bounds__(256) void source_cull_kernel(photon::LensCull c, const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ z, long long n, unsigned char *__restrict__ off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) off[i] = source_misses_sensor(c, x[i], y[i], z[i]) ? 1 : 0;
}

// The bound behind photon_scene_live_sources on its own, host only (no device call): off[i] = 1 when source i cannot reach the
// sensor through lens samples (lens_x[k], lens_y[k]).  Returns 0, or 1 when the geometry is not covered (off is all zeros).
extern "C" int photon_sources_missing_sensor(const float *lens_x, const float *lens_y, int n_samples, float image_distance, float beam_wavelength,
                                             int num_elements, const element_data_t *edp, const double (*element_center)[3],
                                             const double (*element_plane_parameters)[4], const int *element_system_index,
                                             const camera_design_t *cam, const float *x, const float *y, const float *z, long long n,
                                             unsigned char *off) {
    if (!lens_x || !lens_y || n_samples < 1 || !edp || !element_center || !element_plane_parameters || !element_system_index || !cam ||
        n < 0 || (n > 0 && (!x || !y || !z || !off))) return 2;
    for (long long i = 0; i < n; i++) off[i] = 0;
    const std::vector<float> lx(lens_x, lens_x + n_samples), ly(lens_y, lens_y + n_samples);
    const photon::LensCull cull = lens_cull_setup(lx, ly, image_distance, beam_wavelength, num_elements, edp, element_center,
                                                  element_plane_parameters, element_system_index, cam);
    if (!cull.ok) return 1;
    for (long long i = 0; i < n; i++) off[i] = source_misses_sensor(cull, x[i], y[i], z[i]) ? 1 : 0;
    return 0;
}

// The sources whose image can fall on the sensor (source_misses_sensor), decided ONCE per scene, with its first volume-free
// launch (a scene that only ever marches through a volume -- C3, C5, every shard of a PHOTON_DEVICES call -- never pays the
// kernel and the two small copies): flags on the device (null stream; the sources were uploaded when the scene was created),
// back to the host, compacted there (ascending: launches take slices of the list), the list up again.
int photon::ensure_live_sources(photon_scene *s) {
    if (s->live_sources_tried) return 0;
    s->live_sources_tried = true;
    s->live_sources_known = false;
    const size_t ns = (size_t)s->dev.num_sources;
    if (!s->source_cull.ok || ns == 0) return 0;
    DeviceScope on_scene_device(s->device);
    // The cull only saves work: without room for it every source is launched, and the trace is as right as with it.
    const auto skipped = [] {
        fprintf(stderr, "photon: no device memory for the source cull: it is skipped and every source is launched\n");
        return 0;
    };
    PoolBuffer<unsigned char> d_off;
    if (d_off.alloc(ns) != hipSuccess) return skipped();
    hipLaunchKernelGGL(source_cull_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, nullptr, s->source_cull, s->dev.sx, s->dev.sy, s->dev.sz,
                       (long long)ns, d_off.p);
    std::vector<unsigned char> off(ns);
    PH_CHECK(hipGetLastError());
    PH_CHECK(hipMemcpy(off.data(), d_off.p, ns, hipMemcpyDeviceToHost));
    d_off.reset();                                                      // back to the cache before the list below asks it for a block
    std::vector<int> keep;
    keep.reserve(ns);
    for (size_t i = 0; i < ns; i++)
        if (!off[i]) keep.push_back((int)i);
    if (keep.size() == ns) return 0;
    if (keep.empty()) keep.push_back(0);                                // a launch of zero rays is nobody's friend
    PoolBuffer<char> list;                                              // the scene's once it is filled
    if (list.alloc(keep.size() * sizeof(int)) != hipSuccess) return skipped();
    int *d_keep = reinterpret_cast<int *>(list.p);
    PH_CHECK(hipMemcpy(d_keep, keep.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice));
    s->allocs.push_back(std::move(list));
    s->d_live_sources = d_keep;
    s->live_sources = std::move(keep);
    s->live_sources_known = true;
    return 0;
}

// =============================================================================================
// when a cull may be used: one plan per trace
// =============================================================================================
// the reference's element path (optical_system without the working train) applies element 0 once per single-member group of
// the sequence: is there one, and is element 0 a lens with an aperture test?
static bool first_aperture_applies(const photon_scene *s) {
    if (s->dev.train_mode != 0) return false;
    const char type = s->dev.elems[0].element_type;
    if (type != 'l' && type != 't') return false;
    bool applied = false;
    const int n = std::min(s->dev.num_elements, kMaxElements);
    int seq = 0;
    for (int k = 0; k < n; k++) seq = std::max(seq, s->dev.sys_index[k]);
    for (int idx = 0; idx < seq && !applied; idx++) {
        int count = 0;
        for (int k = 0; k < n; k++) count += (seq - s->dev.sys_index[k] == idx);
        applied = count == 1;
    }
    return applied;
}

// Rays that cannot reach the sensor need not be marched.  The reference kills a ray whose intersection with the
// first element's front surface lies more than pitch/2 from the axis (.cu:447, 560-566) -- for a full-aperture
// cone that is half of all rays, because the lens-sample radius goes up to pitch, not pitch/2 (.cu:123-124).
// The volume only bends a ray by a bounded angle: |d(n t)/ds| = |grad n| <= G, so after a path of length L inside
// the volume its direction is off by at most G L / n_min, and its footprint on the lens by at most that angle times
// the distance still to go (plus the walk-off inside the volume).  Returns that bound, times a safety factor
// that also covers the tricubic sampler's overshoot and the integrator's error, plus a thousandth of the
// aperture; 0 when it is not finite or the element has no pitch.
static float doom_margin(const photon_scene *s, const photon_volume *vol) {
    const VolumeDev &v = vol->dev;
    const double ex = (double)v.max_bound.x - v.min_bound.x, ey = (double)v.max_bound.y - v.min_bound.y,
                 ez = (double)v.max_bound.z - v.min_bound.z;
    const double L = sqrt(ex * ex + ey * ey + ez * ez);
    const double n_min = 1.0 + std::min(0.0, (double)v.data_min);
    const double angle = (double)vol->grad_max * L / n_min;
    const double z_obj = (double)s->dev.object_distance + s->dev.z_offset;
    const double to_lens = fabs(z_obj - s->lens_z) + L;                 // generous: the whole object-lens distance
    const double pitch = s->dev.elems[0].element_geometry.pitch;
    const double margin = 8.0 * angle * (to_lens + L) + 1e-3 * pitch;
    if (!(margin == margin) || !(pitch > 0)) return 0.f;
    return (float)margin;
}

// Which order a launch uses.  Lens-major pays off when the ray cone of a source is wider than the volume's
// texels where it crosses the volume (then the 64 rays of ONE source fan out over many texel blocks, while
// 64 neighbouring sources aimed at one lens point stay together); source-major otherwise (BOS: the cone is a
// micron wide) and whenever something indexes rays by the reference's launch order (ray dumps) or the march
// needs per-ray ids (gradient noise): make_trace_plan.  Here: what photon_scene_set_ray_order asked for, the cone
// against the texels when it left the choice open.
static bool use_lens_major(const photon_scene *s, const photon_volume *vol) {
    if (s->ray_order_mode != 2) return s->ray_order_mode == 1;
    const double z_obj = (double)s->dev.object_distance + s->dev.z_offset;             // camera frame
    const double z_face = (double)vol->dev.min_bound.z + s->dev.z_offset + 750e3;      // the volume's lens-side face
    const double span = z_obj - s->lens_z;
    if (!(span > 0)) return false;
    double frac = (z_obj - z_face) / span;
    frac = frac < 0 ? 0 : (frac > 1 ? 1 : frac);
    const double cone = (double)s->dev.ratio * s->dev.lens_pitch * frac;               // cone diameter at that face
    const photon_volume_info_t &i = vol->info;
    const double texel = std::min((double)i.grid_spacing[0], std::min((double)i.grid_spacing[1], (double)i.grid_spacing[2]));
    return cone > texel;
}

// The decisions every launch of a trace shares, taken once per trace -- and not kept: photon_scene_set_skip_doomed,
// _set_ray_order, _set_noise and _set_element_train may be called between two traces of one scene.  dumping: something
// indexes the rays by the reference's launch order (ray dumps), so every ray is launched, in that order.
TracePlan photon::make_trace_plan(photon_scene *s, const photon_volume *vol, int algorithm, bool dumping, bool with_moments) {
    TracePlan p{};
    const int rps = s->dev.rays_per_source;
    const bool ngrad = s->dev.noise.add_ngrad != 0;
    // every cull leaves out rays that the first element's aperture test would drop
    const bool cull = s->skip_doomed && !dumping && first_aperture_applies(s);
    // Without a volume only the lens samples that can reach the first aperture are launched (live_lens_samples): the dead ones
    // would be generated, meet the element's front surface and be dropped -- half of a full-aperture PIV cone
    p.live_samples_only = cull && !vol && s->d_live && s->live_count < rps;
    // ... and only the sources whose image can fall on the sensor (source_misses_sensor): no sensor-position noise (unbounded),
    // the scene's source list as it was created.  The scene's first volume-free trace decides the list; a failure: everything is launched
    p.listed_sources = cull && !vol && !s->dev.noise.add_pos && ensure_live_sources(s) == 0 && s->live_sources_known;
    p.doom_margin = cull && vol && (algorithm == 1 || algorithm == 2) && !ngrad ? doom_margin(s, vol) : 0.f;
    p.lens_major = vol && !dumping && !ngrad && rps >= 2 && use_lens_major(s, vol);
    // a launch holds at most kMaxRaysPerLaunch rays: of those it really launches (the sample PIV frame's 5e8 rays go in two launches,
    // not eight); with moments, also a moments block of at most as many entries, and that is indexed by lens sample, not by slot
    p.slot_rays = p.live_samples_only ? s->live_count : rps;
    p.max_sources = std::max<long long>(1, kMaxRaysPerLaunch / (unsigned)(with_moments ? rps : p.slot_rays));
    p.march = march_knobs(s->march_segments);
    return p;
}

// The next launch of a trace that has come to source `begin` and ends at `limit`: up to max_sources sources -- or up to
// max_sources LISTED sources, the range ending before the next listed one -- and the slice of the scene's list they are.
LaunchRange photon::next_launch(const photon_scene *s, const TracePlan &plan, long long begin, long long limit) {
    LaunchRange r{begin, std::min(limit, begin + plan.max_sources), 0, nullptr};
    r.n_sources = r.end - r.begin;
    if (!plan.listed_sources) return r;
    const auto &ls = s->live_sources;
    const auto lo = std::lower_bound(ls.begin(), ls.end(), (int)begin);
    r.end = (ls.end() - lo) > plan.max_sources ? std::min<long long>(lo[plan.max_sources], limit) : limit;     // (lo[max_sources] > *lo >= begin)
    r.n_sources = std::lower_bound(lo, ls.end(), (int)r.end) - lo;
    r.src_list = s->d_live_sources + (lo - ls.begin());
    return r;
}
