// photon_scene.hip - scene and source handles: what start_ray_tracing uploads before its launch loop
// (parallel_ray_tracing.cu:3132-3314) as a device-resident scene, the glibc srand(10) lens-sample table, and the
// on-device scene generators.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "photon_internal.hpp"
#include "piv_field.hpp"

using namespace photon;

// Light-field sources generated in HBM.
// BOS target (generate_bos_lightfield_data, run_simulation_02.py:1328-1551): source (dot g, point j) sits at
// (dot_x[g] + tmpl_x[j], dot_y[g] + tmpl_y[j], z); sums in double, cast to f32 like the ctypes marshalling.
__global__ __launch_bounds__(256) void sources_bos_kernel(const double *__restrict__ dot_x, const double *__restrict__ dot_y,
                                                          long long n_dots, const double *__restrict__ tx,
                                                          const double *__restrict__ ty, int n_tmpl, double z, double radiance,
                                                          float *sx, float *sy, float *sz, double *srad, int *sdia) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dots * n_tmpl) return;
    const long long g = i / n_tmpl;
    const int j = (int)(i % n_tmpl);
    sx[i] = (float)(dot_x[g] + tx[j]);
    sy[i] = (float)(dot_y[g] + ty[j]);
    sz[i] = (float)z;
    srad[i] = radiance;
    sdia[i] = 1;                                                        // run_simulation_02.py:1544
}

// PIV particle field (run_simulation_02.py:774-996): the draw and the store live in piv_field.hpp, shared with the
// advected field of photon_flow.hip.
__global__ __launch_bounds__(256) void sources_piv_kernel(unsigned long long seed, long long n, PivFieldDev f,
                                                          const double *__restrict__ diameter_cdf, float *sx, float *sy,
                                                          float *sz, double *srad, int *sdia) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double X, Y, Z, ud;
    piv_draw(seed, i, f, X, Y, Z, ud);
    piv_store(i, f, X, Y, Z, ud, diameter_cdf, sx, sy, sz, srad, sdia);
}

// A scene's small host arrays (tables, optics, a shard's sources) travel in ONE block and one host-to-device copy: a scene
// is built per start_ray_tracing call -- per device and call with PHOTON_DEVICES -- and thirteen synchronous copies of a
// few kilobytes each cost more than the bytes (measured: 0.15 ms of a call).  Arrays beyond kPackLimit are copied straight
// from the caller's memory (staging 24 MB of source coordinates through another host buffer would cost more than it saves).
constexpr size_t kPackLimit = 256 << 10, kPackAlign = 256;
struct UploadPack {
    struct Item { size_t offset; const void **slot; };
    std::vector<char> host;
    std::vector<Item> items;
};
template <typename T>
static int upload(photon_scene *s, UploadPack &pack, const T *host, size_t n, const T **dev_out) {
    const size_t bytes = n * sizeof(T);
    if (bytes > kPackLimit) {
        T *d = nullptr;
        PH_TRY(scene_block(s, bytes, &d));
        PH_CHECK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        *dev_out = d;
        return 0;
    }
    const size_t offset = (pack.host.size() + kPackAlign - 1) / kPackAlign * kPackAlign;
    pack.host.resize(offset + std::max<size_t>(bytes, sizeof(T)));           // an empty array still gets a valid address
    if (bytes) memcpy(pack.host.data() + offset, host, bytes);
    pack.items.push_back({offset, reinterpret_cast<const void **>(dev_out)});
    *dev_out = nullptr;
    return 0;
}
// a zeroed region of the block (the statistics counters, the work queues): no fill kernel, no second block
template <typename T>
static void reserve_zeroed(UploadPack &pack, size_t n, T **dev_out) {
    const size_t offset = (pack.host.size() + kPackAlign - 1) / kPackAlign * kPackAlign;
    pack.host.resize(offset + n * sizeof(T));                           // std::vector value-initialises: zeros
    pack.items.push_back({offset, reinterpret_cast<const void **>(const_cast<const T **>(dev_out))});
    *dev_out = nullptr;
}
static int flush_uploads(photon_scene *s, UploadPack &pack) {
    if (pack.items.empty()) return 0;
    char *d = nullptr;
    PH_TRY(scene_block(s, pack.host.size(), &d));
    PH_CHECK(hipMemcpy(d, pack.host.data(), pack.host.size(), hipMemcpyHostToDevice));
    for (const auto &it : pack.items) *it.slot = d + it.offset;
    return 0;
}

template <typename T>
static int copy_device(photon_scene *s, const T *dev_src, size_t n, const T **dev_out) {
    T *d = nullptr;
    PH_TRY(scene_block(s, std::max<size_t>(n, 1) * sizeof(T), &d));
    if (n) PH_CHECK(hipMemcpyAsync(d, dev_src, n * sizeof(T), hipMemcpyDeviceToDevice, nullptr));     // the caller waits for the null stream
    *dev_out = d;
    return 0;
}

// glibc rand()/srand() sequence (TYPE_3 additive-feedback generator r[i] = r[i-3] + r[i-31]),
// re-implemented so the lens-sample table of parallel_ray_tracing.cu:3228-3235 is reproduced
// without touching the caller's process-wide rand() state.
static void glibc_rand_sequence(unsigned seed, int count, std::vector<int> &out) {
    std::vector<int32_t> r(344 + count);
    r[0] = (int32_t)seed;
    for (int i = 1; i < 31; i++) {
        const int64_t hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
        int64_t word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (int32_t)word;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int i = 34; i < 344 + count; i++) r[i] = (int32_t)((uint32_t)r[i - 31] + (uint32_t)r[i - 3]);
    out.resize(count);
    for (int i = 0; i < count; i++) out[i] = (int)((uint32_t)r[344 + i] >> 1);
}

// =============================================================================================
// C-ABI: extension entry points
// =============================================================================================
extern "C" {

int photon_set_device(int device) {
    PH_CHECK(hipSetDevice(device));
    return 0;
}

int photon_device_pci_bus_id(char *buf, int len) {
    if (!buf || len < 16) return 1;
    int dev = 0;
    PH_CHECK(hipGetDevice(&dev));
    PH_CHECK(hipDeviceGetPCIBusId(buf, len, dev));
    return 0;
}

int photon_rand_table(int n, float *r1, float *r2) {
    if (n < 0) return 1;
    std::vector<int> seq;
    glibc_rand_sequence(10u, 2 * n, seq);
    for (int k = 0; k < n; k++) {                       // RAND_MAX = 2147483647
        r1[k] = (float)((double)seq[2 * k] / 2147483647);
        r2[k] = (float)((double)seq[2 * k + 1] / 2147483647);
    }
    return 0;
}

void photon_scene_free(photon_scene_t *s) {
    if (!s) return;
    photon::DeviceScope on_scene_device(s->device);             // the caller may have another device current: wait on, and free into, the scene's --
    delete s;                                                   // for the whole delete: the members go after the destructor's body
}

// ---------------------------------------------------------------------------------------------
// light-field sources generated on the device
// ---------------------------------------------------------------------------------------------
void photon_sources_free(photon_sources_t *src) { delete src; }

}  // extern "C"

int photon::sources_alloc(long long n, std::unique_ptr<photon_sources> *out) {
    std::unique_ptr<photon_sources> src(new photon_sources());
    src->n = n;
    const size_t m = (size_t)n;
    if (src->x.alloc(m) != hipSuccess || src->y.alloc(m) != hipSuccess || src->z.alloc(m) != hipSuccess ||
        src->radiance.alloc(m) != hipSuccess || src->diameter_index.alloc(m) != hipSuccess) {
        fprintf(stderr, "photon: sources: device allocation failed\n");
        return 3;
    }
    *out = std::move(src);
    return 0;
}

// The extent live_lens_samples trusts for generated sources: the largest |x|, |y| and the z range of the particles, a rounding
// to float wider.  A NaN anywhere leaves the extent unset (every lens sample is then launched).
void photon::sources_set_extent(photon_sources *src, double ax, double ay, double z0, double z1) {
    src->rmax = sqrt(ax * ax + ay * ay) * (1 + 1e-6);
    src->zmin = z0 - 1e-6 * fabs(z0) - 1e-3;
    src->zmax = z1 + 1e-6 * fabs(z1) + 1e-3;
    src->have_extent = src->rmax == src->rmax && src->zmin == src->zmin && src->zmax == src->zmax;
}

extern "C" {

int photon_sources_bos(const double *dot_x, const double *dot_y, int n_dots, const double *tmpl_x, const double *tmpl_y,
                       int n_tmpl, double z, double radiance, photon_sources_t **out) {
    if (!out || n_dots < 0 || n_tmpl < 1 || (n_dots && (!dot_x || !dot_y)) || !tmpl_x || !tmpl_y ||
        (long long)n_dots * n_tmpl > 0x7fffffffLL) {
        fprintf(stderr, "photon: photon_sources_bos: bad arguments\n");
        return 1;
    }
    return guarded("photon_sources_bos", [&]() -> int {
        const long long n = (long long)n_dots * n_tmpl;
        std::unique_ptr<photon_sources> src;
        PH_TRY(sources_alloc(n, &src));
        DeviceBuffer<double> d_in;                                          // dot_x | dot_y | tmpl_x | tmpl_y
        if (d_in.alloc(2 * (size_t)n_dots + 2 * (size_t)n_tmpl) != hipSuccess) {
            fprintf(stderr, "photon: photon_sources_bos: device allocation failed (dots and template)\n");
            return 3;
        }
        double *d_dx = d_in.p, *d_dy = d_dx + n_dots, *d_tx = d_dx + 2 * (size_t)n_dots, *d_ty = d_tx + n_tmpl;
        if ((n_dots && (hipMemcpy(d_dx, dot_x, n_dots * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(d_dy, dot_y, n_dots * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)) ||
            hipMemcpy(d_tx, tmpl_x, n_tmpl * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_ty, tmpl_y, n_tmpl * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 4;
        if (n) {
            hipLaunchKernelGGL(sources_bos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_dx, d_dy, (long long)n_dots,
                               d_tx, d_ty, n_tmpl, z, radiance, src->x.p, src->y.p, src->z.p, src->radiance.p, src->diameter_index.p);
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
        }
        *out = src.release();
        return 0;
    });
}

int photon_sources_piv(uint64_t seed, long long n, const double box_min[3], const double box_max[3], double z_object,
                       double beam_fwhm, double irradiance_constant, const double *diameter_cdf, int n_diameters,
                       photon_sources_t **out) {
    if (!out || n < 0 || n > 0x7fffffffLL || !box_min || !box_max || !(beam_fwhm > 0) || n_diameters < 0 ||
        (n_diameters > 0 && !diameter_cdf)) {
        fprintf(stderr, "photon: photon_sources_piv: bad arguments\n");
        return 1;
    }
    return guarded("photon_sources_piv", [&]() -> int {
        std::unique_ptr<photon_sources> src;
        PH_TRY(sources_alloc(n, &src));
        const PivFieldDev f = piv_field_setup(box_min, box_max, z_object, beam_fwhm, irradiance_constant, n_diameters);
        DeviceBuffer<double> d_cdf;
        if (n_diameters > 0) {
            if (d_cdf.alloc((size_t)n_diameters) != hipSuccess) {
                fprintf(stderr, "photon: photon_sources_piv: device allocation failed (diameter table)\n");
                return 3;
            }
            if (hipMemcpy(d_cdf.p, diameter_cdf, n_diameters * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 4;
        }
        if (n) {
            hipLaunchKernelGGL(sources_piv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (unsigned long long)seed, n, f,
                               d_cdf.p, src->x.p, src->y.p, src->z.p, src->radiance.p, src->diameter_index.p);
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
        }
        {   // the box the particles were drawn from (sources_piv_kernel: X, Y uniform in the box, z = Z + z_object)
            const double ax = std::max(fabs(box_min[0]), fabs(box_max[0])), ay = std::max(fabs(box_min[1]), fabs(box_max[1]));
            sources_set_extent(src.get(), ax, ay, std::min(box_min[2], box_max[2]) + z_object, std::max(box_min[2], box_max[2]) + z_object);
        }
        *out = src.release();
        return 0;
    });
}

long long photon_sources_count(const photon_sources_t *src) { return src ? src->n : -1; }

int photon_sources_download(const photon_sources_t *src, float *x, float *y, float *z, double *radiance,
                            int *diameter_index) {
    if (!src) return 1;
    const size_t n = (size_t)src->n;
    if (!n) return 0;
    if (x) PH_CHECK(hipMemcpy(x, src->x.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (y) PH_CHECK(hipMemcpy(y, src->y.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (z) PH_CHECK(hipMemcpy(z, src->z.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (radiance) PH_CHECK(hipMemcpy(radiance, src->radiance.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (diameter_index) PH_CHECK(hipMemcpy(diameter_index, src->diameter_index.p, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

static int scene_create_impl(float lens_pitch, float image_distance, const scattering_data_t *sdp,
                             const char *scattering_type_str, const lightfield_source_t *lsp,
                             const photon_sources *generated, int lightray_number_per_particle, float beam_wavelength,
                             float aperture_f_number, int num_elements, const double (*element_center)[3],
                             const element_data_t *edp, const double (*element_plane_parameters)[4],
                             const int *element_system_index, const camera_design_t *cam, float ray_cone_pitch_ratio,
                             photon_scene_t **out);

int photon_scene_create(float lens_pitch, float image_distance, const scattering_data_t *sdp,
                        const char *scattering_type_str, const lightfield_source_t *lsp,
                        int lightray_number_per_particle, float beam_wavelength, float aperture_f_number,
                        int num_elements, const double (*element_center)[3], const element_data_t *edp,
                        const double (*element_plane_parameters)[4], const int *element_system_index,
                        const camera_design_t *cam, float ray_cone_pitch_ratio, photon_scene_t **out) {
    return guarded("photon_scene_create", [&]() -> int {
        return scene_create_impl(lens_pitch, image_distance, sdp, scattering_type_str, lsp, nullptr,
                                 lightray_number_per_particle, beam_wavelength, aperture_f_number, num_elements, element_center,
                                 edp, element_plane_parameters, element_system_index, cam, ray_cone_pitch_ratio, out);
    });
}

int photon_scene_create_from_sources(float lens_pitch, float image_distance, const scattering_data_t *sdp,
                                     const char *scattering_type_str, const lightfield_source_t *lsp,
                                     const photon_sources_t *sources, int lightray_number_per_particle,
                                     float beam_wavelength, float aperture_f_number, int num_elements,
                                     const double (*element_center)[3], const element_data_t *edp,
                                     const double (*element_plane_parameters)[4], const int *element_system_index,
                                     const camera_design_t *cam, float ray_cone_pitch_ratio, photon_scene_t **out) {
    if (!sources) {
        fprintf(stderr, "photon: photon_scene_create_from_sources: null sources\n");
        return 1;
    }
    return guarded("photon_scene_create_from_sources", [&]() -> int {
        return scene_create_impl(lens_pitch, image_distance, sdp, scattering_type_str, lsp, sources,
                                 lightray_number_per_particle, beam_wavelength, aperture_f_number, num_elements, element_center,
                                 edp, element_plane_parameters, element_system_index, cam, ray_cone_pitch_ratio, out);
    });
}

static int scene_create_impl(float lens_pitch, float image_distance, const scattering_data_t *sdp,
                             const char *scattering_type_str, const lightfield_source_t *lsp,
                             const photon_sources *generated, int lightray_number_per_particle, float beam_wavelength,
                             float aperture_f_number, int num_elements, const double (*element_center)[3],
                             const element_data_t *edp, const double (*element_plane_parameters)[4],
                             const int *element_system_index, const camera_design_t *cam, float ray_cone_pitch_ratio,
                             photon_scene_t **out) {
    if (!sdp || !scattering_type_str || !lsp || !edp || !cam || !out || !element_center || !element_plane_parameters ||
        !element_system_index) {
        fprintf(stderr, "photon: photon_scene_create: null argument\n");
        return 1;
    }
    if (num_elements < 1 || num_elements > 65536) {
        fprintf(stderr, "photon: %d optical elements given, 1..65536 supported\n", num_elements);
        return 1;
    }
    const long long n_sources = generated ? generated->n : (long long)lsp->num_particles;
    if (lightray_number_per_particle < 1 || n_sources < 0 || n_sources > 0x7fffffffLL) {
        fprintf(stderr, "photon: bad ray / source counts\n");
        return 1;
    }
    std::unique_ptr<photon_scene> owner(new photon_scene());   // the caller's device is current and stays so: a failure path frees into its block cache
    photon_scene *s = owner.get();
    (void)hipGetDevice(&s->device);
    SceneDev &d = s->dev;
    UploadPack pack;
    d.lens_pitch = lens_pitch; d.image_distance = image_distance; d.beam_wavelength = beam_wavelength;
    d.f_number = aperture_f_number; d.ratio = ray_cone_pitch_ratio;
    d.scattering_type = strcmp(scattering_type_str, "mie") == 0 ? 1 : 0;       // .cu:3192
    d.rays_per_source = lightray_number_per_particle;
    const size_t ns = (size_t)n_sources;
    d.num_sources = (int)ns;
    if (generated) {                                    // already in HBM: device-to-device, no host arrays
        s->launched = true;                             // copies in flight: a failure below must not hand their blocks to the cache unwaited
        PH_TRY(copy_device<float>(s, generated->x.p, ns, &d.sx));
        PH_TRY(copy_device<float>(s, generated->y.p, ns, &d.sy));
        PH_TRY(copy_device<float>(s, generated->z.p, ns, &d.sz));
        PH_TRY(copy_device<double>(s, generated->radiance.p, ns, &d.sradiance));
        PH_TRY(copy_device<int>(s, generated->diameter_index.p, ns, &d.sdia));
        if (hipStreamSynchronize(nullptr) != hipSuccess) return 4;        // complete before the scene is handed out: its launches may use any stream
    } else {
        PH_TRY(upload(s, pack, lsp->x, ns, &d.sx));
        PH_TRY(upload(s, pack, lsp->y, ns, &d.sy));
        PH_TRY(upload(s, pack, lsp->z, ns, &d.sz));
        PH_TRY(upload(s, pack, lsp->radiance, ns, &d.sradiance));
        PH_TRY(upload(s, pack, lsp->diameter_index, ns, &d.sdia));
    }
    d.z_offset = lsp->z_offset; d.object_distance = lsp->object_distance;
    memcpy(d.mie_inv_rot, sdp->inverse_rotation_matrix, sizeof d.mie_inv_rot);
    memcpy(d.beam, sdp->beam_propagation_vector, sizeof d.beam);
    d.num_angles = sdp->num_angles; d.num_diameters = sdp->num_diameters;
    if (d.scattering_type) {
        if (sdp->num_angles < 2 || sdp->num_diameters < 1 || !sdp->scattering_angle || !sdp->scattering_irradiance) {
            fprintf(stderr, "photon: \"mie\" scattering needs an angle/irradiance table\n");
            return 1;
        }
        PH_TRY(upload(s, pack, sdp->scattering_angle, (size_t)sdp->num_angles, &d.mie_angle));
        PH_TRY(upload(s, pack, sdp->scattering_irradiance, (size_t)sdp->num_angles * sdp->num_diameters, &d.mie_irr));
    }
    photon::LensCull source_cull;
    std::vector<float> r1(lightray_number_per_particle), r2(lightray_number_per_particle);
    photon_rand_table(lightray_number_per_particle, r1.data(), r2.data());
    // x_lens = ratio * 1.0 * pitch * r1 * cos(2 pi r2), the whole product in double, then to float (.cu:123-124): the same for
    // every source (the table is indexed by the ray's number within its source, .cu:2006), so it is evaluated HERE, once per
    // lens sample, with the function the kernels used per ray (photon_det_sincos: the same bits on host and device, which is
    // what the CPU oracle relies on) -- a double-precision sincos and six double multiplies per ray less: ray generation
    // 0.205 -> 0.184 ms per 1e7 rays (135 -> 121 M VALU instructions per launch), the volume-free PIV frame 25.9 -> 25.5 ms
    {
        std::vector<float> lx(r1.size()), ly(r1.size());
        for (size_t k = 0; k < r1.size(); k++) {
            double sn, cs;
            photon_det_sincos(2 * M_PI * r2[k], &sn, &cs);
            lx[k] = (float)(d.ratio * 1.0 * d.lens_pitch * r1[k] * cs);
            ly[k] = (float)(d.ratio * 1.0 * d.lens_pitch * r1[k] * sn);
        }
        PH_TRY(upload(s, pack, lx.data(), lx.size(), &d.lens_x));
        PH_TRY(upload(s, pack, ly.data(), ly.size(), &d.lens_y));
        // Which lens samples can reach the first element's aperture at all (photon_cull.hip, live_lens_samples): the rest need not be
        // launched on the volume-free path -- half of a full-aperture cone.
        std::vector<int> live = live_lens_samples(lx, ly, lsp, generated, ns, image_distance, num_elements, edp, element_center,
                                                  element_plane_parameters);
        s->live_count = (int)live.size();
        s->live_host = live;
        if (live.size() < lx.size()) PH_TRY(upload(s, pack, live.data(), live.size(), &s->d_live));
        // ... and which SOURCES can reach the sensor at all (photon_cull.hip, source_misses_sensor): decided on the device once the sources are there
        s->live_sources_known = false;
        if (ns > 0 && lx.size() >= 2)
            source_cull = lens_cull_setup(lx, ly, image_distance, beam_wavelength, num_elements, edp, element_center,
                                          element_plane_parameters, element_system_index, cam);
    }
    d.num_elements = num_elements;
    {
        std::vector<float> centers(3 * (size_t)num_elements), planes(4 * (size_t)num_elements);
        for (int k = 0; k < num_elements; k++) {                               // .cu:3256-3260 (f64 -> f32)
            for (int j = 0; j < 3; j++) centers[3 * k + j] = (float)element_center[k][j];
            for (int j = 0; j < 4; j++) planes[4 * k + j] = (float)element_plane_parameters[k][j];
            if (k < kMaxElements) {                                            // the reference path reads these
                d.elems[k] = edp[k];
                for (int j = 0; j < 3; j++) d.centers[k][j] = centers[3 * k + j];
                for (int j = 0; j < 4; j++) d.planes[k][j] = planes[4 * k + j];
                d.sys_index[k] = element_system_index[k];
            }
        }
        d.train_mode = 0;
        d.source_base = 0;                                      // (slot_rays, slot_map, src_list, src_perm, ray_order, doom_margin: per launch, launch_chunk)
        s->lens_z = (float)element_center[0][2];
        PH_TRY(upload(s, pack, edp, (size_t)num_elements, &d.all_elems));
        PH_TRY(upload(s, pack, centers.data(), centers.size(), &d.all_centers));
        PH_TRY(upload(s, pack, planes.data(), planes.size(), &d.all_planes));
        PH_TRY(upload(s, pack, element_system_index, (size_t)num_elements, &d.all_sys_index));
    }
    // The statistics counters (the march's error word among them: scene_error_word) and the work queues start at zero --
    // every march launch leaves the queues so -- and are zeroed HERE, as part of the one host-to-device copy, which is
    // complete when hipMemcpy returns.  hipMemset is not: it returns as soon as its fill kernel is queued on the null
    // stream (9 us, with the fill itself 200 ms away behind a full chip: tools/ubench/null_stream_memset.hip), and a march
    // launched on a non-blocking stream is not ordered behind the null stream -- with eight shards side by side on one device
    // the fill of one shard's queues waited for wave slots next to that shard's own march and, once in a dozen calls, ran
    // AFTER the march had started handing out groups (pieces handed out again: 3 of 60 C4 calls refused with hand-off errors, one
    // image off by 6e-5 with none).
    reserve_zeroed(pack, kCounterBytes / sizeof(unsigned long long), &s->d_counters);
    reserve_zeroed(pack, (size_t)kQueues * kQueueStride, &s->d_queue);
    PH_TRY(flush_uploads(s, pack));
    s->source_cull = source_cull;                               // the device pass runs with the first volume-free trace (photon_cull.hip, ensure_live_sources)
    d.cam = *cam;
    d.noise = NoiseDev{0, 0, 0.f, 0.f, 0ull};
    if (cam->x_pixel_number < 1 || cam->y_pixel_number < 1) {
        fprintf(stderr, "photon: sensor needs at least one pixel\n");
        return 1;
    }
    hipError_t e = s->acc.alloc((size_t)cam->x_pixel_number * cam->y_pixel_number);
    if (e != hipSuccess) { fprintf(stderr, "photon: hipMalloc failed: %s\n", hipGetErrorString(e)); return (int)e; }
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            s->num_cus = cus;
    }
    for (auto &ev : s->ev) {
        e = ev.create();
        if (e != hipSuccess) { fprintf(stderr, "photon: hipEventCreate failed: %s\n", hipGetErrorString(e)); return (int)e; }
    }
    *out = owner.release();
    return 0;
}

int photon_scene_set_noise(photon_scene_t *scene, int add_pos_noise, float pos_noise_std, int add_ngrad_noise,
                           float ngrad_noise_std, uint64_t seed) {
    if (!scene) return 1;
    scene->dev.noise = NoiseDev{add_pos_noise ? 1 : 0, add_ngrad_noise ? 1 : 0, pos_noise_std, ngrad_noise_std,
                                (unsigned long long)seed};
    return 0;
}

int photon_scene_set_source_base(photon_scene_t *s, int64_t first_source) {
    if (!s || first_source < 0) return 1;
    s->dev.source_base = (long long)first_source;
    return 0;
}

int photon_scene_set_element_train(photon_scene_t *s, int mode) {
    if (!s || (mode != 0 && mode != 1)) return 1;
    s->dev.train_mode = mode;
    return 0;
}

int photon_scene_set_ray_order(photon_scene_t *s, int mode) {
    if (!s || mode < 0 || mode > 2) return 1;
    s->ray_order_mode = mode;
    return 0;
}

int photon_scene_live_rays(const photon_scene_t *s) { return s ? s->live_count : -1; }
int photon_scene_live_samples(const photon_scene_t *s, int *out, int capacity) {
    if (!s || !out || capacity < s->live_count) return -1;
    for (int k = 0; k < s->live_count; k++) out[k] = s->live_host[(size_t)k];
    return s->live_count;
}

// The sources the volume-free path launches (ascending indices), or -1 when every source is (nothing could be ruled out)
long long photon_scene_live_sources(const photon_scene_t *s, int *out, long long capacity) {
    if (!s) return -2;
    if (photon::ensure_live_sources(const_cast<photon_scene_t *>(s))) return -2;
    if (!s->live_sources_known) return -1;
    const long long n = (long long)s->live_sources.size();
    if (out) {
        if (capacity < n) return -2;
        memcpy(out, s->live_sources.data(), (size_t)n * sizeof(int));
    }
    return n;
}

int photon_scene_set_skip_doomed(photon_scene_t *s, int on) {
    if (!s) return 1;
    s->skip_doomed = on != 0;
    return 0;
}

}  // extern "C"

namespace photon {

void scene_quiesce(photon_scene *s) {
    if (!s->launched) return;
    DeviceScope on_scene_device(s->device);                     // hipDeviceSynchronize waits for the CURRENT device
    (void)hipDeviceSynchronize();
    s->launched = false;
}

// What a segmented march keeps per ray between segments (MarchResume) and the per-group flags; allocated with the first
// segmented launch of a workspace size (ensure_workspace drops both blocks when it regrows).  The flags carry the launch's
// epoch: epoch 0 = not zeroed yet (launch_march does it, on the launch's stream).
int ensure_resume_state(photon_scene *s, bool linear) {
    const size_t rays = s->ws_rays, groups = (rays + 63) / 64;
    if (!s->resume.p) {
        PH_CHECK(s->resume.alloc(2 * rays + groups));
        unsigned *u = s->resume.p;
        s->ws.ctr = u; s->ws.spins = u + rays; s->ws.seg_flag = u + 2 * rays;
        s->march_epoch = 0;
    }
    if (linear && !s->vprev.p) PH_CHECK(s->vprev.alloc(4 * rays));
    s->ws.vprev = s->vprev.p;
    return 0;
}

int ensure_workspace(photon_scene *s, size_t rays) {
    if (s->ws_rays >= rays) return 0;
    s->ws_rays = 0;
    PH_TRY(scene_reserve(s, s->ray_state, rays * 6));           // a smaller launch of this scene may still be using the old blocks
    s->resume.reset(); s->vprev.reset();                        // sized by the workspace: the next segmented launch makes them anew
    s->ws.ctr = s->ws.spins = s->ws.seg_flag = nullptr; s->ws.vprev = nullptr;
    PH_TRY(scene_reserve(s, s->radiance, rays));
    float *f = s->ray_state.p;
    s->ws.px = f; s->ws.py = f + rays; s->ws.pz = f + 2 * rays;
    s->ws.dx = f + 3 * rays; s->ws.dy = f + 4 * rays; s->ws.dz = f + 5 * rays;
    s->ws.radiance = s->radiance.p;
    s->ws_rays = rays;
    s->ws.stride = (unsigned)rays;
    return 0;
}

}  // namespace photon

// The scene's blocks go back to the CACHE, not to the runtime (whose free would wait for the device): the next scene of the
// same shape may be handed them at once and overwrite them with copies on the null stream, which does not wait for kernels
// of this scene still running on a non-blocking stream.  So wait here (microseconds on an idle device); the members then
// release themselves.
photon_scene::~photon_scene() { photon::scene_quiesce(this); }
