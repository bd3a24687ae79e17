/*
 * parallel_ray_tracing.h - C-ABI of libparallel_ray_tracing.so (MI355X / gfx950 build)
 *
 * Drop-in boundary for photon's ray-tracing core.  photon's Python driver loads the
 * library with ctypes (python_codes/perform_ray_tracing_03.py:1888) and binds exactly
 * one symbol, `start_ray_tracing` (argtypes at :1914-1921, restype None at :1925).
 * The struct layouts below are the wire format of that call: they must agree byte for
 * byte with the ctypes.Structure classes the reference builds at
 * perform_ray_tracing_03.py:1651-1659 (scattering), :1708-1720 (source),
 * :1751-1786 (element), :1838-1852 (camera), which in turn mirror
 * cuda_codes/parallel_ray_tracing.h:17-191.  tests/test_abi.py checks sizeof/offsetof
 * against fixtures captured from the reference's marshalling code.
 *
 * Everything is plain C: pointers, sizes, PODs.  No torch / HIP types appear in a
 * signature (streams and device pointers travel as void*).
 *
 * Section 1  = the reference's ABI (what photon binds today).
 * Section 2  = `photon_*` extension entry points (device-resident scene / volume /
 *              image handles) that bench.py and the parity tests bind; the reference
 *              has no counterpart, each cites the part of start_ray_tracing it factors out.
 */
#ifndef PHOTON_AMD_PARALLEL_RAY_TRACING_H_
#define PHOTON_AMD_PARALLEL_RAY_TRACING_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Section 1: wire structs (x86-64 SysV natural alignment; sizes in bytes in brackets)
 * ---------------------------------------------------------------------------------- */

/* Mie-scattering lookup data [72].  Replaces cuda_codes/parallel_ray_tracing.h:17-33.
 * scattering_irradiance is row-major [num_angles][num_diameters]; both pointers are
 * NULL and the float fields NaN when scattering_type_str != "mie"
 * (perform_ray_tracing_03.py:1685-1701). */
typedef struct scattering_data_t {
    float inverse_rotation_matrix[9];   /* @0  camera -> world */
    float beam_propagation_vector[3];   /* @36 unit vector of the laser sheet */
    float *scattering_angle;            /* @48 [num_angles], radians, uniform spacing */
    float *scattering_irradiance;       /* @56 [num_angles*num_diameters] */
    int num_angles;                     /* @64 */
    int num_diameters;                  /* @68 */
} scattering_data_t;

/* Light-field sources = particles / dot-pattern points [64].
 * Replaces cuda_codes/parallel_ray_tracing.h:36-60. */
typedef struct lightfield_source_t {
    int lightray_number_per_particle;   /* @0  */
    int source_point_number;            /* @4  sources per launch chunk (10000 in photon) */
    int *diameter_index;                /* @8  [num_particles] column of the Mie table */
    double *radiance;                   /* @16 [num_particles] */
    float *x;                           /* @24 [num_particles] microns, camera frame */
    float *y;                           /* @32 */
    float *z;                           /* @40 */
    int num_particles;                  /* @48 */
    float z_offset;                     /* @52 z_object - object_distance */
    float object_distance;              /* @56 */
} lightfield_source_t;

/* [32] cuda_codes/parallel_ray_tracing.h:115-131 */
typedef struct element_geometry_t {
    float front_surface_radius;         /* @0  */
    bool front_surface_spherical;       /* @4  */
    float back_surface_radius;          /* @8  */
    bool back_surface_spherical;        /* @12 */
    float pitch;                        /* @16 clear aperture diameter */
    double vertex_distance;             /* @24 centre thickness */
} element_geometry_t;

/* [24] cuda_codes/parallel_ray_tracing.h:134-141 */
typedef struct element_properties_t {
    float abbe_number;                  /* @0  NaN = no dispersion */
    float absorbance_rate;              /* @4  */
    double refractive_index;            /* @8  */
    float thin_lens_focal_length;       /* @16 */
    float transmission_ratio;           /* @20 */
} element_properties_t;

/* One optical element [120].  cuda_codes/parallel_ray_tracing.h:144-162.
 * element_type: 'l' thick spherical lens, 't' thin lens, 'n' apparent image (no lens),
 * anything else = aperture stop (parallel_ray_tracing.cu:416,507,868; :2143). */
typedef struct element_data_t {
    double axial_offset_distances[2];   /* @0  */
    element_geometry_t element_geometry;/* @16 */
    float element_number;               /* @48 */
    element_properties_t element_properties; /* @56 */
    char element_type;                  /* @80 */
    float elements_coplanar;            /* @84 */
    double rotation_angles[3];          /* @88 */
    float z_inter_element_distance;     /* @112 */
} element_data_t;

/* Sensor description [112].  cuda_codes/parallel_ray_tracing.h:165-191. */
typedef struct camera_design_t {
    int pixel_bit_depth;                /* @0  */
    float pixel_gain;                   /* @4  */
    float pixel_pitch;                  /* @8  microns */
    float x_camera_angle;               /* @12 */
    float y_camera_angle;               /* @16 */
    int x_pixel_number;                 /* @20 image width  W */
    int y_pixel_number;                 /* @24 image height H */
    float z_sensor;                     /* @28 */
    float diffraction_diameter;         /* @32 pixels */
    bool implement_diffraction;         /* @36 true: erf splat, false: 4-pixel splat */
    float rotation_matrix[9];           /* @40 world -> camera */
    float inverse_rotation_matrix[9];   /* @76 camera -> world */
} camera_design_t;

/*
 * start_ray_tracing - render one sensor image.
 * Replaces cuda_codes/parallel_ray_tracing.cu:3078-3775 (declared
 * cuda_codes/parallel_ray_tracing.h:303-307).  Argument meaning is unchanged:
 *   image_array        f32[H*W], row-major row*W+col, READ-MODIFY-WRITE (accumulates on
 *                      the caller's contents, .cu:3309,3675)
 *   element_center     f64[num_elements][3]; element_plane_parameters f64[num_elements][4]
 *   ray_tracing_algorithm  1 euler, 2 rk4, 3 rk45, 4 adams-bashforth; any other value leaves the ray
 *                      straight (the reference's `default: break`, trace_rays_...h:1537).  3 and 4
 *                      are restated literally, trilinear on the raw volume whatever PHOTON_INTERP
 *   density_grad_filename  NRRD (type float, dimension 3; encoding raw, gzip or ascii; either byte order), "" when unused
 *   save_lightrays     writes <pos_path>/pos_%04d.bin, <dir_path>/dir_%04d.bin per chunk
 * All pointers are borrowed for the duration of the call.  No error channel (void):
 * on failure a message goes to stderr and image_array is left unmodified.
 * Environment knobs (the ABI has no room for new arguments):
 *   PHOTON_INTERP=linear|cubic   volume sampler (default linear = the reference's
 *                                hard-coded interpolation_scheme 1, .cu:3330)
 *   PHOTON_TEX_WEIGHTS=fixed8|exact   trilinear weights: 8 fractional bits like the texture unit the reference's
 *                                tex3D() runs on (default) or exact f32 (photon_volume_set_weight_bits)
 *   PHOTON_VERBOSE=1             progress / timing on stdout
 *   PHOTON_NOISE_SEED=u64        seed of the add_pos_noise / add_ngrad_noise generators (the
 *                                reference seeds cuRAND with time(NULL); default 0x5eed)
 *   PHOTON_ELEMENT_TRAIN=reference|sequential   element-group walk (photon_scene_set_element_train)
 *   PHOTON_SKIP_DOOMED=0|1       1 (default): rays that provably die on the first aperture are not marched; without a volume
 *                                the lens samples no source can get through it and the sources whose image cannot fall on the
 *                                sensor are not launched (photon_scene_set_skip_doomed); the image is the same bit for bit
 *   PHOTON_RAY_ORDER=source|lens|auto           lane order of a launch (photon_scene_set_ray_order)
 *   PHOTON_DEVICES=all|0,1,..    shard the sources of one call over several GPUs: one host thread per
 *                                device uploads only its block of the sources, the NRRD is parsed once, the
 *                                private f64 accumulators are summed on the first device (peer copies +
 *                                a kernel) and folded into image_array once; default: the calling
 *                                thread's current device (which is restored on return in every case)
 */
void start_ray_tracing(float lens_pitch, float image_distance,
                       scattering_data_t *scattering_data_p, char *scattering_type_str,
                       lightfield_source_t *lightfield_source_p,
                       int lightray_number_per_particle, float beam_wavelength,
                       float aperture_f_number, int num_elements,
                       double (*element_center)[3], element_data_t *element_data_p,
                       double (*element_plane_parameters)[4], int *element_system_index,
                       camera_design_t *camera_design_p, float *image_array,
                       bool simulate_density_gradients, char *density_grad_filename,
                       bool save_lightrays, char *lightray_position_save_path,
                       char *lightray_direction_save_path, int num_lightrays_save,
                       int ray_tracing_algorithm, bool add_pos_noise, float pos_noise_std,
                       bool add_ngrad_noise, float ngrad_noise_std,
                       float ray_cone_pitch_ratio, bool save_intermediate_ray_data,
                       int num_intermediate_positions_save);

/* ------------------------------------------------------------------------------------
 * Section 2: device-resident extension API (what bench.py / tests bind)
 * Return value: 0 on success, non-zero HIP / argument error (message on stderr).
 * ---------------------------------------------------------------------------------- */

typedef struct photon_volume photon_volume_t;   /* refractive-index gradient volume in HBM */
typedef struct photon_scene photon_scene_t;     /* sources, tables, optics, camera in HBM  */

/* Host-visible description of a loaded volume (mirrors density_grad_params_t,
 * cuda_codes/parallel_ray_tracing.h:213-252, minus the pointers). */
typedef struct photon_volume_info_t {
    float min_bound[3];
    float max_bound[3];
    int nx, ny, nz;
    float grid_spacing[3];
    float step_size;
    float data_min;         /* min over the volume of n-1 */
    int interpolation;      /* 1 trilinear, 2 tricubic B-spline */
} photon_volume_info_t;

/* Per-trace counters (filled from device atomics; for roofline accounting).  LAYOUT FROZEN at 72 bytes (round 3): the
 * library writes sizeof(photon_trace_stats_t) bytes through the caller's pointer, so the struct never grows again -- later
 * measurements come through structs that carry their own size (photon_march_profile_t). */
typedef struct photon_trace_stats_t {
    uint64_t rays_launched;
    uint64_t rays_on_sensor;        /* rays that reached the splat stage inside the sensor */
    uint64_t rk_iterations;         /* completed integrator iterations, summed over rays */
    uint64_t volume_samples;        /* sampler invocations, summed over rays */
    uint64_t sensor_taps;           /* atomic adds issued */
    float march_ms;                 /* HIP-event time of the volume-march kernel(s) */
    float total_ms;                 /* HIP-event time of the whole trace */
    uint64_t rays_marched;          /* rays that entered the volume march: rays_launched minus those dropped before it
                                       because they provably die on the first aperture (photon_scene_set_skip_doomed);
                                       0 without a volume */
    float shader_clock_mhz;         /* clock the march kernel actually ran at: s_memtime / s_memrealtime ticks summed over its
                                       waves x 100 MHz (the chip lowers its clock under load, differently from device to
                                       device); 0 without a volume */
    uint32_t traces;                /* photon_trace calls these numbers cover (1, or the calls of a statistics window) */
    float march_wave_ms;            /* mean time a march wave spends on one 64-ray group, from the same stamps: a launch of G
                                       groups lasts about G / (waves resident on the chip) of these */
} photon_trace_stats_t;

/* Select the GPU this thread's subsequent photon_* calls use (hipSetDevice). */
int photon_set_device(int device);

/* PCI bus id ("0000:c1:00.0") of the calling thread's current device: names its sysfs node
 * (/sys/bus/pci/devices/<id>/hwmon/...: board power, cap) for measurement scripts. */
int photon_device_pci_bus_id(char *buf, int len);

/* glibc-compatible lens-sample table, factored out of parallel_ray_tracing.cu:3216-3243
 * (srand(10); r1[k]=rand()/RAND_MAX; r2[k]=rand()/RAND_MAX, interleaved).  Host arrays. */
int photon_rand_table(int n, float *r1, float *r2);

/* NRRD load + n-1 / grad(n) volume build (+ B-spline prefilter when interpolation==2).
 * Replaces readDatafromFile/loadNRRD/setData/Host_Init,
 * cuda_codes/trace_rays_through_density_gradients.h:1612-2105. */
int photon_volume_load_nrrd(const char *path, int interpolation, photon_volume_t **out);
/* Same, from a density field already on the host (x fastest), for synthetic volumes.
 * origin is the NRRD "space origin" BEFORE the reference's -750e3 z shift (.h:1704). */
int photon_volume_from_density(const float *rho, int nx, int ny, int nz,
                               const double spacing[3], const double origin[3],
                               int interpolation, photon_volume_t **out);
int photon_volume_info(const photon_volume_t *vol, photon_volume_info_t *info);
/* Trilinear interpolation weights: bits = 8 (default) rounds them to 8 fractional bits, the 9-bit fixed-point
 * weights CUDA's linear texture filter uses (CUDA C Programming Guide, "Linear Filtering") -- i.e. what the
 * reference's tex3D() fetches (trace_rays_through_density_gradients.h:1052 ...) compute with on NVIDIA
 * hardware; bits = 0 keeps them exact f32.  Takes effect for every later sample / trace of this volume; the
 * tricubic sampler (always the exact 64-tap sum) is unaffected.  start_ray_tracing reads
 * PHOTON_TEX_WEIGHTS=fixed8|exact. */
int photon_volume_set_weight_bits(photon_volume_t *vol, int bits);
/* Copy the float4 texels (grad x,y,z, n-1) -- or the B-spline coefficients when
 * interpolation==2 and coefficients!=0 -- back to the host: f32[nz*ny*nx*4]. */
int photon_volume_download(const photon_volume_t *vol, int coefficients, float *out);
/* Sample at n unnormalised texel coordinates (the argument of tex3D / cubicTex3D,
 * trace_rays_through_density_gradients.h:1052,1216): coords f32[n][3] -> out f32[n][4].
 * Host arrays; used by the sampler parity tests. */
int photon_volume_sample(const photon_volume_t *vol, int n, const float *coords, float *out);
void photon_volume_free(photon_volume_t *vol);

/* Upload everything start_ray_tracing copies to the device before its launch loop
 * (parallel_ray_tracing.cu:3132-3314): same arguments, same meaning. */
int photon_scene_create(float lens_pitch, float image_distance,
                        const scattering_data_t *scattering_data_p,
                        const char *scattering_type_str,
                        const lightfield_source_t *lightfield_source_p,
                        int lightray_number_per_particle, float beam_wavelength,
                        float aperture_f_number, int num_elements,
                        const double (*element_center)[3], const element_data_t *element_data_p,
                        const double (*element_plane_parameters)[4],
                        const int *element_system_index,
                        const camera_design_t *camera_design_p, float ray_cone_pitch_ratio,
                        photon_scene_t **out);
/* Waits for the scene's device first when a trace of this scene may still be running (its device blocks go back to the
 * library's block cache, see photon_trim_caches, and may be handed to the next scene at once): freeing a scene right after an
 * asynchronous photon_trace is safe on any stream.  A scene belongs to the device that was current when it was created;
 * photon_trace, photon_scene_free and the statistics calls make that device current for their duration and restore the
 * caller's, so they may be called with any device current. */
void photon_scene_free(photon_scene_t *scene);

/* Noise hooks of start_ray_tracing (its add_pos_noise / pos_noise_std / add_ngrad_noise /
 * ngrad_noise_std arguments, parallel_ray_tracing.cu:3405-3445): Gaussian jitter of the sensor hit
 * (sigma in pixels) and of dn/dx, dn/dy in the Euler march.  Counter-based generator keyed by
 * `seed` (include/photon_philox.h); off by default. */
int photon_scene_set_noise(photon_scene_t *scene, int add_pos_noise, float pos_noise_std, int add_ngrad_noise,
                           float ngrad_noise_std, uint64_t seed);

/* How element groups are walked (propagate_rays_through_optical_system, parallel_ray_tracing.cu:1274-1381).
 * mode 0 (default) = the reference as it runs: every single-member group goes through element 0
 * (:1331-1333), groups of simultaneous elements reach an empty stub (:1049-1272).  mode 1 = the working
 * train: each group through its own element(s), simultaneous elements (lenslet arrays, any number)
 * chosen per ray by nearest centre on the element plane (design: perform_ray_tracing_03.py:1254-1485).
 * start_ray_tracing reads it from PHOTON_ELEMENT_TRAIN=reference|sequential. */
int photon_scene_set_element_train(photon_scene_t *scene, int mode);

/* The partition of a march launch over its work queues (host restatement of the kernel's own functions, for tests).
 * photon_march_queue_count() queues -- 8 XCDs x (count / 8) sub-queues, 32 in the shipped build; consecutive groups form
 * CHUNKS of groups (photon_march_queue_chunk(interpolation): 16 for the tricubic kernels in source-major launches through
 * volumes of up to 256^3 texels, 128 for the trilinear kernels -- and for every lens-major launch or larger volume), and
 * queue (xcd, sub) owns the chunks c with c % count == sub * 8 + xcd.  photon_march_queue_group: index of the k-th 64-ray
 * group that queue hands out (grows with k); photon_march_queue_size: how many of a launch's n_groups groups it owns.
 * Every group of a launch belongs to exactly one queue.  An xcd >= 8, a sub >= count / 8 or a groups_per_chunk that is
 * not a power of two up to 65536 returns UINT_MAX.
 * A launch whose marches are cut into S segments (photon_scene_set_march_segments) hands out size * S items per queue,
 * segment-major: item k is segment k / size of the queue's (k % size)-th group. */
unsigned photon_march_queue_count(void);
unsigned photon_march_queue_chunk(int interpolation);
unsigned photon_march_queue_group(unsigned k, unsigned xcd, unsigned sub, unsigned groups_per_chunk);
unsigned photon_march_queue_size(unsigned n_groups, unsigned xcd, unsigned sub, unsigned groups_per_chunk);

/* Segments per march (speed only; the image does not depend on it, nor do the marched rays: tests).  A 64-ray group marches
 * for ~2 ms and a launch ends when its last group does, so the chip idles for most of a group time at the end of every
 * launch; a launch of several chip fills therefore cuts every march into `segments` pieces of equal trip count, handed out
 * breadth-first, and a ray's loop state travels with it from piece to piece.  -1 (default) = the library's choice
 * (at most PHOTON_MARCH_SEGMENTS, 32, in launches of at least 1.25 chip fills: more pieces the shorter the launch and the
 * longer a march), 1 = whole marches, 2..64 = that many in every
 * launch, whatever its size (tests).  Launches that write intermediate ray dumps or use gradient noise are never segmented.
 * start_ray_tracing reads PHOTON_MARCH_SEGMENTS=<n> (the library's choice) or force:<n> (every launch). */
int photon_scene_set_march_segments(photon_scene_t *scene, int segments);
/* The library's own choice for a launch of n_rays through a volume whose longest axis has `depth` texels, on a device of
 * num_cus compute units: returns the number of pieces (1 = whole marches), *halving (may be NULL) = 1 when their lengths
 * halve (1/2, 1/4, ... of the depth) rather than being equal.  The planner every march launch goes through (a cost model
 * fitted to a sweep on C3: DESIGN.md section 4.1), asked about a source-major launch without dumps or noise, with no scene
 * setting and PHOTON_MARCH_SEGMENTS ignored; pure host arithmetic, 0 for integrators other than 1 and 2. */
int photon_march_segments_plan(unsigned n_rays, int depth, int ray_tracing_algorithm, int interpolation, int num_cus, int *halving);
/* Everything the library decides about one march launch before it enqueues it, from the same planner, as a trace would
 * decide it (PHOTON_MARCH_SEGMENTS and PHOTON_MARCH_SEGMENT_SHAPE are read): n_rays through an nx x ny x nz volume on a
 * device of num_cus compute units.  scene_segments: what photon_scene_set_march_segments holds (-1 = not set).  flags:
 * bit 0 intermediate ray dumps are asked for, bit 1 gradient noise, bit 2 a lens-major launch.  Pure host arithmetic.
 * The caller sets struct_size = sizeof(photon_march_plan_t); returns 0, or 1 for arguments no launch can have. */
typedef struct photon_march_plan_t {
    uint32_t struct_size;
    int segments;               /* pieces per march; piece s covers the trips [seg_begin[s], seg_begin[s + 1]) */
    int shape;                  /* 0 equal pieces, 1 halving, 2 tapered */
    unsigned seg_begin[65];
    unsigned groups_per_chunk;  /* consecutive 64-ray groups a work queue owns as one chunk */
    unsigned grid_blocks, block_threads;
    int persistent;             /* 1: a grid that fills the chip once and serves the work queues (integrators 1, 2); 0: one thread per ray */
    int save, noise, segmented; /* the kernel variant: records intermediate dumps, draws gradient noise, marches in pieces */
    int generates_rays;         /* 1: the march generates its rays itself, no ray-generation kernel runs before it */
} photon_march_plan_t;
int photon_march_launch_plan(unsigned n_rays, int nx, int ny, int nz, int ray_tracing_algorithm, int interpolation, int num_cus,
                             int scene_segments, int flags, photon_march_plan_t *out);

/* A scene that holds only a SLICE of a job's source list (one rank of a multi-GPU job uploads just its shard): the
 * index, in the job's list, of this scene's first source.  Only the noise hooks read it -- their generator is keyed by the
 * ray's place in the whole job, so a sharded render draws the numbers the unsharded one draws.  Default 0. */
int photon_scene_set_source_base(photon_scene_t *scene, int64_t first_source);

/* Order in which a launch lays its rays over the GPU's lanes (results are a sum: the image does not depend
 * on it beyond f64 summation order).  0 = source-major, the reference's thread order (.cu:1988-2006): best
 * when a source's ray cone is narrower than a volume texel (BOS).  1 = lens-major over spatially sorted
 * sources: a wave carries 64 neighbouring sources aimed at one lens point -- best when the cone is as wide as
 * the aperture (PIV through a volume).  2 = choose per launch from the cone width at the volume and the
 * texel size (default).  Launches that write ray dumps or use gradient noise are always source-major; with
 * mode 1 or 2 the [src_begin, src_end) of photon_trace counts sources in the sorted order.
 * start_ray_tracing reads PHOTON_RAY_ORDER=source|lens|auto. */
int photon_scene_set_ray_order(photon_scene_t *scene, int mode);

/* Rays that cannot reach the sensor need not be marched (default on).  The reference kills a ray that meets the
 * first element's front surface more than pitch/2 from the axis (thin lens .cu:447, thick lens .cu:560-566) --
 * half of a full-aperture cone, whose lens samples reach out to a radius of one pitch (.cu:123-124) -- but only
 * after marching it through the volume.  With the switch on, a ray whose UNDEFLECTED path misses the aperture by
 * more than the largest footprint shift the volume can cause (bounded from the volume's largest |grad n|) is dropped
 * before the march: same image, same rays_on_sensor; rk_iterations / volume_samples count only the rays marched.
 * Off automatically for launches that write ray dumps, use gradient noise, integrators 3 / 4 or the element
 * train.  start_ray_tracing reads PHOTON_SKIP_DOOMED=0|1.
 * WITHOUT a volume the same switch keeps the dead LENS SAMPLES from being launched at all: ray k of every source is aimed at
 * the same point of the lens plane (.cu:123-141), so which samples miss the aperture is decided once per scene, from the
 * caller's source arrays, with a bound that holds for every source (photon_cull.hip, live_lens_samples); the volume-free
 * PIV frame of the reference's sample data (5e8 rays) 25.6 -> 15.5 ms, the image bit for bit.  rays_launched keeps counting
 * sources x rays_per_source.  photon_scene_live_rays: how many lens samples per source such a launch keeps (rays_per_source
 * when none can be ruled out: narrow cones, tilted or off-axis first element, BOS patterns generated on the device; PIV fields
 * generated on the device are bounded by the generator's box). */
int photon_scene_set_skip_doomed(photon_scene_t *scene, int on);
int photon_scene_live_rays(const photon_scene_t *scene);
/* the kept lens samples themselves, ascending (out: room for `capacity` >= photon_scene_live_rays entries); returns their number, -1 on a bad argument */
int photon_scene_live_samples(const photon_scene_t *scene, int *out, int capacity);
/* The same switch also leaves out, on the volume-free path, the SOURCES whose image cannot fall on the sensor (one biconvex
 * thick lens or one thin lens on the axis, no sensor-position noise, no dumps: photon_cull.hip, source_misses_sensor --
 * an interval bound on where the lens can put the source's rays; photon's sample PIV frame draws particles over a field 1.5 x
 * wider than the camera sees, run_simulation_02.py:956-958).  The image is unchanged.  The list is made once per scene, by its
 * first volume-free photon_trace (or by the query below): one small kernel and two small copies on the null stream, for which
 * that call waits -- a scene that only marches through a volume never pays them.  photon_scene_live_sources: the sources
 * that are launched, ascending (out may be NULL to ask for the count); -1 when nothing could be ruled out (all are), -2 on a
 * bad argument. */
long long photon_scene_live_sources(const photon_scene_t *scene, int *out, long long capacity);
/* The bound itself, host arithmetic only (no device call, usable without a GPU): off[i] = 1 when source (x, y, z)[i] cannot
 * reach a pixel through any of the lens samples (lens_x, lens_y)[k] on the plane z = image_distance.  Returns 0; 1 when the
 * geometry is not covered (off all zeros); 2 on a bad argument. */
int photon_sources_missing_sensor(const float *lens_x, const float *lens_y, int n_samples, float image_distance, float beam_wavelength,
                                  int num_elements, const element_data_t *element_data_p, const double (*element_center)[3],
                                  const double (*element_plane_parameters)[4], const int *element_system_index,
                                  const camera_design_t *camera_design_p, const float *x, const float *y, const float *z,
                                  long long n, unsigned char *off);

/* The launch loop (parallel_ray_tracing.cu:3515-3672) for sources [src_begin, src_end)
 * with everything resident in HBM.  d_image: device f32[H*W], accumulated into.
 * vol may be NULL (= simulate_density_gradients false).  stream: hipStream_t as void*
 * (NULL = default stream).  Asynchronous unless stats != NULL (stats forces a sync).
 * The traces of ONE scene share its ray-state workspace, work queues and f64 accumulator (which every trace leaves zeroed for
 * the next): issue them on one stream, or order them yourself when you change streams; different scenes are independent.
 * Hand-off errors of a segmented march (a wave gave up waiting for the previous piece of its group, or read a stale ray
 * state: never observed, and then the render is incomplete) are counted on the device and REPORTED where the host reads the
 * statistics -- photon_trace with stats, photon_scene_stats_end -- which zero the count when they start and fail (non-zero
 * return, message on stderr) when it is set.  A caller of plain asynchronous traces (stats = NULL, no window) learns of them
 * from photon_scene_check. */
int photon_trace(photon_scene_t *scene, const photon_volume_t *vol, int ray_tracing_algorithm,
                 int64_t src_begin, int64_t src_end, float *d_image, void *stream,
                 photon_trace_stats_t *stats);

/* Per-source sensor moments: photon_trace plus one RECORD of 8 doubles per traced source -- the ground truth of a synthetic
 * BOS / PIV pair (how far each dot moved, by what angle its rays were bent) without ray dumps.
 *   record[0]    n         rays of the source that reached the sensor: whose final position (all three components) is a
 *                          number -- exactly the rays whose pos_ dump entry is one (an off-sensor hit is NaN)
 *   record[1..3] sum x, y, z        final sensor-plane position, camera frame, microns (what pos_ dumps hold)
 *   record[4..6] sum acos(dx, dy, dz)  of the direction dir_ dumps hold (radians: the angles the reference's reader
 *                          works in, light_ray_processing.py:120-140)
 *   record[7]    sum x^2 + y^2     second radial moment (rms spot radius of the dot's image)
 * Records are additive (merge consecutive sources into a dot, concatenate shards and launches); a source with no arriving
 * ray has an all-zero record.  Fixed summation order: every f32 is widened to f64 (exact); lane l of 64 adds the values of
 * the rays j = l (mod 64), j < rays_per_source, in increasing j, from +0.0 -- j is the ray's OWN lens-sample index, never its
 * slot in a launch; a ray that did not arrive adds nothing -- and the 64 partials are folded by halves (off = 32, 16, .., 1:
 * p[l] += p[l + off] for l < off); the record is p[0].  So a record has the same bits whatever the ray order, the doomed-ray,
 * lens-sample and live-source culls (they only drop rays that provably never reach the sensor), march segments, launch
 * boundaries, [src_begin, src_end) splits or PHOTON_DEVICES sharding; photon_amd/deflections.py (moments_from_dumps)
 * reproduces it on the host bit for bit, up to an ulp of f64 acos in fields 4-6.
 * Cost: per launch a moments block of 24 B per (launched source x rays_per_source) -- at most kMaxRaysPerLaunch (2^26)
 * entries, 1.5 GiB: with moments a launch takes at most 2^26 / rays_per_source sources even where the volume-free path
 * launches only the live lens samples -- written by the sensor stage, read once by a reduction kernel.
 *
 * photon_trace_moments: photon_trace (same image up to f64 summation order, asynchronous, same rules for sharing a scene,
 * no stats) that also writes the records of sources [src_begin, src_end) to d_records[source][8] (device memory, indexed by
 * the source's place in the scene's list, num_sources records) and leaves every other record untouched.  A null d_records
 * or a bad range: non-zero return, nothing written. */
int photon_trace_moments(photon_scene_t *scene, const photon_volume_t *vol, int ray_tracing_algorithm,
                         int64_t src_begin, int64_t src_end, float *d_image, double *d_records, void *stream);

/* photon_start_ray_tracing_moments: start_ray_tracing (same 29 arguments, same PHOTON_* settings, the same image) plus the
 * records of every source in source_moments, a HOST f64[num_particles][8].  With save_lightrays it also writes the dumps
 * (records from the dump chunks); with PHOTON_DEVICES naming several devices each shard's records land in their own slice.
 * Returns 0, or non-zero with the reason on stderr (then image and records are not to be used). */
int photon_start_ray_tracing_moments(float lens_pitch, float image_distance,
                                     scattering_data_t *scattering_data_p, char *scattering_type_str,
                                     lightfield_source_t *lightfield_source_p,
                                     int lightray_number_per_particle, float beam_wavelength,
                                     float aperture_f_number, int num_elements,
                                     double (*element_center)[3], element_data_t *element_data_p,
                                     double (*element_plane_parameters)[4], int *element_system_index,
                                     camera_design_t *camera_design_p, float *image_array,
                                     bool simulate_density_gradients, char *density_grad_filename,
                                     bool save_lightrays, char *lightray_position_save_path,
                                     char *lightray_direction_save_path, int num_lightrays_save,
                                     int ray_tracing_algorithm, bool add_pos_noise, float pos_noise_std,
                                     bool add_ngrad_noise, float ngrad_noise_std,
                                     float ray_cone_pitch_ratio, bool save_intermediate_ray_data,
                                     int num_intermediate_positions_save, double *source_moments);

/* Statistics over a WINDOW of photon_trace calls with no host synchronisation inside it (a timed loop): _begin zeroes
 * the counters on the stream; every photon_trace(..., stats = NULL) of this scene up to _end records its HIP events on
 * its stream and lets the counters run; _end waits for the stream and returns the SUMS over the window's traces
 * (march_ms, total_ms, the counters; shader_clock_mhz over all march waves; traces = number of calls).  The reference
 * prints one wall-clock time per call instead (parallel_ray_tracing.cu:3498-3503, 3678-3684). */
/* The window belongs to the stream it was opened on: a photon_trace of this scene on another stream, or more than 65536
 * traces in one window, is refused. */
int photon_scene_stats_begin(photon_scene_t *scene, void *stream);
int photon_scene_stats_end(photon_scene_t *scene, void *stream, photon_trace_stats_t *stats);
/* Waits for `stream` and returns 0 when no trace of this scene since the count was last zeroed (photon_trace with stats,
 * photon_scene_stats_begin, a previous photon_scene_check) had a hand-off error, 1 (and a message on stderr) otherwise;
 * zeroes the count. */
int photon_scene_check(photon_scene_t *scene, void *stream);

/* Wave timing of the march launches (measurement; off by default, costs a handful of atomics per wave when on).  With
 * it on, every march launch after the statistics counters were last zeroed (photon_trace with stats, or
 * photon_scene_stats_begin) records -- on the device's constant 100 MHz clock -- when its first wave entered, when each
 * wave started its first 64-ray group and when it left; photon_scene_march_profile returns the means over those launches
 * (the first 64 of them), all times counted from the first wave's entry:
 *   span_ms          until the last wave left (the launch as the chip saw it)
 *   start_mean/max   until a wave started its first group (dispatch ramp, argument loads, first queue access)
 *   end_min/mean     until a wave left; span_ms - end_mean_ms = the DRAIN, the average time a wave slot stood empty at the
 *                    end of the launch while the last groups finished
 * The caller sets struct_size = sizeof(photon_march_profile_t) (the library refuses a smaller struct than it knows). */
typedef struct photon_march_profile_t {
    uint32_t struct_size;
    uint32_t launches;              /* march launches the means cover (0: profile off, or no launch since the reset) */
    uint32_t waves;                 /* waves that served at least one group, mean per launch */
    float span_ms;
    float start_mean_ms, start_max_ms;
    float end_min_ms, end_mean_ms;
} photon_march_profile_t;
int photon_scene_set_march_profile(photon_scene_t *scene, int on);
int photon_scene_march_profile(photon_scene_t *scene, photon_march_profile_t *out);
/* The raw stamps of profiled launch `launch` (0 = the first since the reset): out[64][8] = per workgroup-index-mod-64 slot
 * {~min entry, ~min first-group start, sum of starts, max start, ~min exit, sum of exits, max exit, waves} in ticks of the
 * 100 MHz clock (slot & 7 = the XCD); for tools/tail_by_xcd.py. */
int photon_scene_march_profile_raw(photon_scene_t *scene, unsigned launch, unsigned long long *out);

/* March-only entry point for parity tests: n rays (host arrays pos/dir f32[n][3], world
 * frame) through trace_rays_through_density_gradients (.h:1455-1544); results in place,
 * steps (optional) receives the per-ray completed iteration count. */
int photon_trace_volume_rays(const photon_volume_t *vol, int ray_tracing_algorithm, int n,
                             float *pos, float *dir, int *steps);

/* The same march for arbitrary rays, but THROUGH the render path's march launch -- persistent waves over the work queues,
 * marches cut into `segments` pieces (-1 the library's choice, 1 whole, 2..64 forced): what the adversarial parity tests
 * drive (rays from every side, tiny grids, the below-minimum repair) to hold the segmented march to the oracle's bits.
 * ray_tracing_algorithm 1 or 2.  Results in place. */
int photon_trace_volume_rays_queued(const photon_volume_t *vol, int ray_tracing_algorithm, int n, float *pos, float *dir,
                                    int segments);

/* ------------------------------------------------------------------------------------
 * Section 3: scene generation on the device (the step right before the
 * hot path).  photon builds its source arrays and its synthetic density files in Python
 * (run_simulation_02.py, nrrd_functions.py) and ships them through start_ray_tracing; for
 * 1e6-source / 512^3 configurations these entry points build the same data directly in HBM.
 * ---------------------------------------------------------------------------------- */

typedef struct photon_sources photon_sources_t; /* light-field sources (x, y, z, radiance, diameter index) in HBM */

/* BOS target, generate_bos_lightfield_data (run_simulation_02.py:1328-1551): every dot centre
 * (dot_x[g], dot_y[g]) is expanded by the point template (tmpl_x[j], tmpl_y[j]) -- the sunflower
 * disc of calculate_sunflower_coordinates (:999-1056) -- into source g*n_tmpl + j at
 * (dot_x[g] + tmpl_x[j], dot_y[g] + tmpl_y[j], z); sums in double, stored as f32 (what the ctypes
 * marshalling does, perform_ray_tracing_03.py:1730-1745); radiance constant, diameter index 1. */
int photon_sources_bos(const double *dot_x, const double *dot_y, int n_dots, const double *tmpl_x,
                       const double *tmpl_y, int n_tmpl, double z, double radiance,
                       photon_sources_t **out);
/* PIV particle field, run_simulation_02.py:774-996: X, Y, Z uniform in [box_min, box_max),
 * radiance = irradiance_constant / (sigma sqrt(2 pi)) * exp(-Z^2 / (2 sigma^2)) with
 * sigma = beam_fwhm / (2 sqrt(2 ln 2)) (the laser sheet, :961-962), z = Z + z_object.  The reference
 * draws from numpy's unseeded generator; here particle i takes the four 32-bit words of
 * Philox4x32-10(seed, i) (include/photon_philox.h, stream PHOTON_STREAM_SCENE): reproducible, and any
 * particle can be regenerated on its own.  diameter_cdf (may be NULL): cumulative distribution over
 * n_diameters table columns, index = first d with u < cdf[d]; NULL = index 1 like the reference (:992). */
int photon_sources_piv(uint64_t seed, long long n, const double box_min[3], const double box_max[3],
                       double z_object, double beam_fwhm, double irradiance_constant,
                       const double *diameter_cdf, int n_diameters, photon_sources_t **out);

/* PIV frame pairs (time series): the particles of photon_sources_piv moved by a steady velocity field.
 *
 * photon_flow_t: u, v, w are host f32 [nz][ny][nx] (x fastest, like the density volume), velocity in microns per unit
 * of t, on the nodes origin + (i, j, k) * spacing of the WORLD frame of photon_sources_piv (X, Y, Z, before the z_object
 * shift).  Each axis needs n >= 2; spacing finite and > 0, origin finite.  Stored in HBM as one float4 {u, v, w, 0} per
 * node, on the current device.
 *
 * Operation order (all f64, no fused multiply-add; photon_amd/piv_pairs.py follows it bit for bit):
 *   sample V(p), per axis a:  f = (p_a - origin_a) / spacing_a;  c = floor(f);  c = c >= 0 ? c : 0;
 *                             c = c <= n_a - 2 ? c : n_a - 2;  t_a = f - c;  t_a = t_a > 0 ? t_a : 0;  t_a = t_a < 1 ? t_a : 1
 *                             (outside the grid: the boundary value; a NaN coordinate takes cell 0 and weight 0)
 *     with lerp(a, b, t) = a + t * (b - a) on the node values widened to f64, per component:
 *       V = lerp(lerp(lerp(v000, v100, tx), lerp(v010, v110, tx), ty), lerp(lerp(v001, v101, tx), lerp(v011, v111, tx), ty), tz)
 *       (v_ijk: the node at cell + (i, j, k))
 *   one RK4 step of h = t / steps:  k1 = V(p);  k2 = V(p + (0.5 h) k1);  k3 = V(p + (0.5 h) k2);  k4 = V(p + h k3);
 *                                   p = p + (h / 6) * (((k1 + 2 k2) + 2 k3) + k4)      (per component, left to right)
 *
 * photon_sources_piv_advected: the frame at time t of the photon_sources_piv field with the same (seed, n, box, z_object,
 * beam_fwhm, irradiance_constant, diameter_cdf).  Particle i starts at the f64 (X, Y, Z) photon_sources_piv draws for
 * it, moves through `flow` by `steps` RK4 steps, and is stored as photon_sources_piv stores it: x = (float)X,
 * y = (float)Y, z = (float)(Z + z_object), radiance = the laser-sheet profile at the NEW Z, diameter index unchanged (the
 * same Philox word).  flow == NULL or t == 0: bit-identical to photon_sources_piv.  Every frame is counter-based: a time
 * series is t = k dt with one seed, and any particle of any frame can be regenerated alone.
 * world_xyz (host f64 [n][3], may be NULL): the particles' (X, Y, Z) at time t, before the cast -- the ground truth.
 * The static skip of dead lens samples trusts a generated field's extent: it is taken from the positions stored (a device
 * reduction), not from the box, which advected particles may have left.
 * Refused (1, one stderr line, *out untouched): the arguments photon_sources_piv refuses, steps < 1, a non-finite t,
 * t != 0 with flow == NULL. */
typedef struct photon_flow photon_flow_t;
int photon_flow_from_grid(const float *u, const float *v, const float *w, int nx, int ny, int nz,
                          const double spacing[3], const double origin[3], photon_flow_t **out);
void photon_flow_free(photon_flow_t *flow);
int photon_sources_piv_advected(uint64_t seed, long long n, const double box_min[3], const double box_max[3],
                                double z_object, double beam_fwhm, double irradiance_constant,
                                const double *diameter_cdf, int n_diameters, const photon_flow_t *flow,
                                double t, int steps, double *world_xyz, photon_sources_t **out);

long long photon_sources_count(const photon_sources_t *sources);
/* Copy back to host arrays (any of them may be NULL). */
int photon_sources_download(const photon_sources_t *sources, float *x, float *y, float *z, double *radiance,
                            int *diameter_index);
void photon_sources_free(photon_sources_t *sources);

/* photon_scene_create with the sources taken from `sources` (device-to-device copy; the scene does not
 * keep a reference).  lightfield_source_p supplies the scalars only (z_offset, object_distance,
 * source_point_number): its arrays and num_particles are ignored. */
int photon_scene_create_from_sources(float lens_pitch, float image_distance,
                                     const scattering_data_t *scattering_data_p, const char *scattering_type_str,
                                     const lightfield_source_t *lightfield_source_p,
                                     const photon_sources_t *sources, int lightray_number_per_particle,
                                     float beam_wavelength, float aperture_f_number, int num_elements,
                                     const double (*element_center)[3], const element_data_t *element_data_p,
                                     const double (*element_plane_parameters)[4], const int *element_system_index,
                                     const camera_design_t *camera_design_p, float ray_cone_pitch_ratio,
                                     photon_scene_t **out);

/* Synthetic density field evaluated on the device instead of written to / read from an NRRD file
 * (nrrd_functions.py:14-57 is the writer it replaces): rho = rho0 + amp * exp(-|r - centre|^2 / (2 sigma^2))
 * on the grid origin + i * spacing, then the same volume build as photon_volume_load_nrrd.  origin is the
 * NRRD "space origin" (before the -750e3 z shift), centre in the same frame. */
int photon_volume_gaussian(int nx, int ny, int nz, const double spacing[3], const double origin[3],
                           double rho0, double amp, const double centre[3], double sigma,
                           int interpolation, photon_volume_t **out);

/* The same Gaussian density field written as an NRRD file (type float, dimension 3, raw, little endian, sizes /
 * spacings / space origin: what nrrd_functions.py:14-57 writes and loadNRRD reads), evaluated on the device. */
int photon_density_gaussian_write_nrrd(const char *path, int nx, int ny, int nz, const double spacing[3],
                                       const double origin[3], double rho0, double amp,
                                       const double centre[3], double sigma);

/* The library keeps freed scene-lifetime device blocks (ray-state workspace, source arrays, accumulators: what every
 * start_ray_tracing call allocates anew) in a cache and hands them to the next scene of the same shape, per device, up to
 * PHOTON_POOL_MAX_MB (default 4096; 0 = no cache): photon's unchanged Python pays ~1 ms of hipFree per call otherwise.
 * photon_trim_caches returns all cached blocks to the runtime (the library does so itself when one of ITS allocations finds
 * the device out of memory; another user of the device -- a framework's caching allocator -- should call it before a large
 * allocation of its own). */
void photon_trim_caches(void);

/* Library / build identification string (static storage): "photon-amd <version> (gfx950, HIP) <git commit>[-dirty] <flags>",
 * <flags> = "default" or "variant[...]" with the non-default -DPHOTON_* compile-time switches of this build. */
const char *photon_version(void);

/* Self-test hook: quot[i] = a[i] / b[i], rcp[i] = 1 / b[i], root[i] = sqrt(a[i]) (host arrays of n floats) evaluated with the
 * march loops' normal-range forms -- the compiler's correctly rounded division / square-root sequences without their range
 * scaling (photon_amd/csrc/device_vec.hpp) -- which return the IEEE results bit for bit whenever operands and results lie
 * within [2^-96, 2^96] in magnitude (a marching ray's sit within a few binades of 1); tests hold them against numpy. */
int photon_selftest_normal_range_math(int n, const float *a, const float *b, float *quot, float *rcp, float *root);

/* Self-test hook: perm_out[k] = index (in [first, first + n)) of the k-th of the sources first .. first + n - 1 of the host
 * arrays x, y (n_total entries) in the spatial order lens-major launches use -- Morton order on a 2^16 x 2^16 grid over the
 * range's bounding box, one scale for both axes, ties in the caller's order -- computed by the device path (bounding box,
 * keys, the library's own stable radix sort: photon_amd/csrc/photon_sort.hip); tests hold it against numpy's stable argsort. */
int photon_selftest_morton_order(const float *x, const float *y, long long n_total, long long first, long long n, int *perm_out);

/* Test hook: make device allocations of the library fail, without memory pressure.  Every block of the library is asked
 * for in one place; a REQUEST is one such asking (a block of the cache, or a block outside it), numbered per process.
 * Requests number first .. first + count - 1, counted from this call (1 = the next one), fail: count = 1 one request,
 * LLONG_MAX "the device stays full" until disarmed; first = 0 disarms.  first_attempt_only = 0: the request returns
 * hipErrorOutOfMemory, the runtime is not called and no cached block is handed out.  first_attempt_only = 1: the request
 * passes the cache by and only its first hipMalloc is replaced by hipErrorOutOfMemory -- the library then empties its block
 * cache and asks the runtime again, for real.  Disarmed the hook costs one atomic increment per request.  Thread safe.
 * Returns 0, or 1 for first < 0 or count < 1 (message on stderr). */
int photon_selftest_fail_alloc(long long first, long long count, int first_attempt_only);

/* Test hook: the allocation counters of this process.  outstanding: blocks handed out and not yet given back, of the cache
 * and outside it alike; idle: what the block cache holds. */
typedef struct photon_alloc_stats {
    long long requests;                 /* requests so far */
    long long injected_failures;        /* requests photon_selftest_fail_alloc made fail (either mode) */
    long long oom_retries;              /* times an allocation found the device full, emptied the cache and asked again */
    long long retry_blocks_returned;    /* cached blocks those retries handed back to the runtime */
    long long idle_blocks, idle_bytes;
    long long outstanding_blocks, outstanding_bytes;
} photon_alloc_stats_t;
int photon_selftest_alloc_stats(photon_alloc_stats_t *out);

/* Device-to-device float4 streaming copy of `bytes` bytes, `reps` times: read + write rate in GB/s -- the HBM rate a
 * trivial kernel reaches on this GPU, which bench.py prints next to the 8 TB/s specification. */
int photon_measure_copy_gbs(size_t bytes, int reps, double *gbs_out);

/* ------------------------------------------------------------------------------------
 * Section 4: sensor post-processing on the device (the step right after the
 * hot path).  Replaces perform_ray_tracing_03.py:2190-2259 (noise -> clip -> 10^(gain/20) ->
 * normalise to the brightest pixel -> round to pixel_bit_depth -> stretch to 16 bit -> uint16 ->
 * optional centre crop), in f32 in numpy's evaluation order, so that the raw image stays in HBM and
 * only the uint16 picture crosses the bus.
 *   d_image   device f32[height*width], row-major; rewritten only when image_noise > 0 (the reference adds the
 *             noise to I_raw itself, :2196-2206; here N(0, 100 image_noise) from Philox(noise_seed, pixel))
 *   crop_rows / crop_cols   0 = no crop; otherwise the reference's window rows [H/2 - r/2, H/2 + r/2 - 1) (integer
 *             division; one row / column fewer than asked, as its slice has it) -- *out_rows / *out_cols receive
 *             the size of the result (may be NULL)
 *   d_out     device uint16[out_rows*out_cols]
 * Synchronises `stream` before returning. */
int photon_postprocess_u16(float *d_image, int width, int height, float pixel_gain, int pixel_bit_depth,
                           int intensity_rescaling, float image_noise, uint64_t noise_seed, int crop_rows, int crop_cols,
                           uint16_t *d_out, int *out_rows, int *out_cols, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 5: windowed direct cross-correlation of an image pair on the device (PIV / BOS displacement
 * fields): the measurement a PIV or BOS user runs on the two images, on images already in HBM.  Host
 * model: photon_amd/piv_correlation.py (correlate_model, f64).
 *   d_im1, d_im2  device f32[height*width], row-major (the library's images)
 *   win           16, 32 or 64 (square windows);  step >= 1;  radius R in [1, win/2]
 *   window (i, j) rows [i step, i step + win), columns [j step, j step + win); n_rows = (height - win)/step + 1,
 *             n_cols = (width - win)/step + 1 (integer division), window k = i n_cols + j; centre at
 *             (i step + (win-1)/2, j step + (win-1)/2) (row, column)
 *   d_offset  device int[n][2] (ox, oy) integer predictor per window, or NULL (0)
 * For every shift s = (sx, sy) in [-R, R]^2, with a = im1 over the window, b(p) = im2(p + o):
 *   C(s) = sum_p (a(p) - mean a)(b(p + s) - mean b) over the win^2 pixels of the window, mean b over the window at
 *   zero shift (its in-image pixels); pixels of im2 outside the image read as mean b (contribute 0).  Every shift
 *   sums the same win^2 products: direct correlation over an enlarged region, no wrap-around, no zero-padding bias.
 *   Cn = C / sqrt(sum (a - mean a)^2 * sum (b - mean b)^2), the second sum at zero shift.
 * Peak s* = argmax C, ties to the first shift in row-major order (sy, then sx).  Subpixel, per axis, from C-, C0, C+
 * through s*, in f64: Gaussian delta = (ln C- - ln C+) / (2 (ln C- - 2 ln C0 + ln C+)); parabolic
 * (C- - C+) / (2 (C- - 2 C0 + C+)) if any of the three is <= 0; 0 when the denominator is 0; 0 and flag 1 when s*
 * lies on the edge of the search square in that axis.
 *   d_vectors device f32[n][4]: dx = ox + sx* + delta_x (columns), dy = oy + sy* + delta_y (rows) -- im2(p + d) ~ im1(p),
 *             a pattern moving right / down gives positive values; peak = Cn(s*); ratio = C(s*) / max{C(s) :
 *             |s - s*|_inf >= 2}, +inf when there is no such shift or that maximum is <= 0
 *   d_flags   device int[n], bits: 1 peak on the search edge, 2 flat window (every output of the window, its plane
 *             included, NaN), 4 a pixel the window needs lies outside im2
 *             A window is flat when all win^2 pixels of a are equal, or when the in-image pixels of b at zero shift are
 *             all equal or there are none: for finite pixels, exactly when an energy of the definition is 0.  This is
 *             decided from the smallest and the largest pixel, not from the f32 energies (an f32 mean of equal pixels
 *             need not reproduce them).  A contrast too small for f32 -- either f32 energy not above 0 -- counts as
 *             flat as well.
 *   d_planes  device f32[n][(2R+1)^2] Cn, row-major (sy, then sx), or NULL
 * d_vectors == NULL: only *n_rows / *n_cols are written (ask for the size first); nothing is launched.
 * Refused (1, one stderr line, nothing written, no launch): win not 16 / 32 / 64, R out of range, step < 1, an
 * image smaller than one window, a null image pointer, d_vectors without d_flags.  f32 sums in a fixed order: two
 * calls on the same inputs return the same bits.  Asynchronous on `stream`. */
int photon_piv_correlate(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int radius,
                         const int *d_offset, float *d_vectors, int *d_flags, float *d_planes, int *n_rows, int *n_cols,
                         void *stream);

/* ------------------------------------------------------------------------------------
 * Section 6: weighted least-squares integration of a gradient field on the device (BOS: displacements -> projected
 * density).  Host model: photon_amd/bos_density.py (integrate_model, f64, the same iteration).
 *   grid        ny x nx nodes, row-major: node k = i nx + j (row i, column j); hx between columns, hy between rows
 *   d_gx, d_gy  device f64[ny*nx]: the gradient along +column and +row
 *   d_w         device f64[ny*nx] weights, or NULL (1)
 *   d_fixed     device u8[ny*nx] Dirichlet mask (nonzero = fixed), or NULL (the outer frame of the grid is fixed)
 *   d_value     device f64[ny*nx] the values of the fixed nodes, or NULL (0)
 * A node is valid when gx, gy and w are finite and w > 0.  Edge (i,j)->(i,j+1): weight w_e = min(w_k, w_k+1) when both
 * ends are valid and neither is a fixed node with a value that is not finite, else 0; target t_e = hx (gx_k + gx_k+1) / 2.
 * Edge (i,j)->(i+1,j): the same with hy and gy.  phi minimises E = sum_e w_e (phi_b - phi_a - t_e)^2 with the fixed
 * nodes held at their values: the normal equations are the weighted graph Laplacian on the unknown nodes, SPD on every
 * unknown node that reaches a fixed node through edges of positive weight (reachability: a BFS on the host).
 *   d_phi       device f64[ny*nx] out: fixed nodes their value; reachable unknown nodes the solution; every other node
 *               (no live edge, or an island without an anchor) NaN
 * Solver: Jacobi-preconditioned CG from x0 = 0 in f64 (z = r / diag; alpha = 0 when p.q = 0, beta = 0 when the old r.z
 * is 0).  ||r||_2 (the recursive, unpreconditioned residual; ||b|| over the reachable unknowns) is checked before the
 * first iteration and then every PHOTON_INTEGRATE_CHECK_EVERY iterations; with tol > 0 the solver stops at the first
 * check with ||r|| <= tol ||b||, else after exactly max_iter iterations (tol = 0: always max_iter).  ||b|| = 0: 0
 * iterations, converged.  Every reduction has a fixed order: two calls on the same inputs return the same bits.
 *   stats       iterations run; converged = final ||r|| <= tol ||b||; residual = final ||r|| / ||b|| (0 when ||b|| = 0);
 *               unknowns = nodes solved for; unreachable = unknown nodes left NaN.  May be NULL.
 * Refused (1, one stderr line, nothing written, no launch): nx or ny < 2, nx ny > INT_MAX, hx or hy not finite or not
 * > 0, tol < 0 or NaN, max_iter < 0, a null d_gx, d_gy or d_phi.  Runs on `stream` and synchronises it before it
 * returns. */
#define PHOTON_INTEGRATE_CHECK_EVERY 8

typedef struct photon_integrate_stats_t {
    int iterations, converged, unknowns, unreachable;
    double residual;
} photon_integrate_stats_t;

int photon_integrate_gradient(const double *d_gx, const double *d_gy, const double *d_w, const unsigned char *d_fixed,
                              const double *d_value, int nx, int ny, double hx, double hy, double tol, int max_iter,
                              double *d_phi, photon_integrate_stats_t *stats, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 7: iterative image-deformation correlation (Scarano 2002; Astarita & Cardone 2005): the three device steps
 * that, with section 5's correlation, measure a displacement that varies inside a window.  The vector field on the
 * window grid is interpolated to every pixel, both images are warped half-way towards each other with a cubic
 * B-spline, the warped pair is correlated for a small residual, and the residual is added, validated and smoothed.
 * Host model: photon_amd/piv_deformation.py (f64); driver: PhotonLibrary.correlate_deform.  All three are asynchronous
 * on `stream`, need no device scratch and return the same bits for the same inputs (every sum has a fixed order).
 *
 * Mirror.  An index i outside [0, n) reads the whole-sample mirror image ... c b | a b c ... y z | y x ... (period
 * 2 (n - 1); n = 1: always 0), numpy.pad(mode="reflect"), scipy.ndimage mode="mirror".
 *
 * a. Coefficients.  d_coef (f32[height*width], not d_im) is the cubic B-spline coefficient image of d_im: the spline
 *    S(y, x) = sum_kl c(k, l) B3(y - k) B3(x - l) over the mirrored coefficients equals the image at the pixel
 *    centres.  c = h *_rows (h *_columns im) on the mirrored image, h[j] = sqrt(3) z^|j|, z = sqrt(3) - 2 (two-sided,
 *    gain 1, sum |h| = 3).  The device truncates h at |j| <= 14 (|z|^15 = 2.6e-9) and sums in f32, along each row
 *    first and then along each column, acc = sum_{j = 14 .. 1} h[j] (x[-j] + x[+j]), then + h[0] x[0], in that order.
 *    Refused: width or height < 1, a null pointer, d_coef == d_im.
 *
 * b. Warp.  d_field: device f32, n_rows x n_cols vectors (dx, dy) `field_stride` floats apart (2, or 4: section 5's
 *    d_vectors as they are); n_rows, n_cols must be section 5's grid for (height, width, win, step).  A vector with a
 *    component that is not finite reads as (0, 0).  Dense displacement at pixel (row r, column q): bilinear in the
 *    window-centre coordinates, fy = clamp((r - (win-1)/2) / step, 0, n_rows - 1), fx = clamp((q - (win-1)/2) / step, 0,
 *    n_cols - 1): with i = min(floor(fy), n_rows - 2), wy = fy - i (i = 0, wy = 0 for one row; likewise j, wx),
 *    D = T + wy (U - T), T = F(i, j) + wx (F(i, j+1) - F(i, j)), U the same on row i + 1: constant beyond the outermost
 *    window centres.  The shift s = clamp(scale D, -2^24, 2^24) per component;
 *    d_out(r, q) = S(r + s_y, q + s_x) = sum_{u=0..3} wy_u sum_{t=0..3} wx_t c(mirror(r + floor(s_y) - 1 + u),
 *    mirror(q + floor(s_x) - 1 + t)), the weights from the fractions t = s - floor(s): ((1-t)^3, 4 - 3 t^2 (2 - t),
 *    4 - 3 (1-t)^2 (1 + t), t^3) / 6.  scale = 0 returns the image the coefficients came from.  The driver warps frame 1
 *    with scale -1/2 and frame 2 with +1/2: with the true field both outputs show the pattern half-way between the frames.
 *    Refused: section 5's rules for win, step and the image size, a side of more than 2^22 pixels, a grid that is not
 *    section 5's, field_stride not 2 or 4, a scale that is not finite, a null pointer, d_out == d_coef.
 *
 * c. Validate and update, per node k of the n_rows x n_cols grid, in f64, every step one IEEE operation in this order:
 *    1. total t = ((pred + d) + 0) per component, pred = d_pred[k] (f32[n][2]; NULL: 0), d = (dx, dy) of d_vectors[k]
 *       (f32[n][4]); both components NaN when d_flags[k] has bit 2 (flat) or either sum is not finite.  (+ 0: a total
 *       of -0 reads as +0.)
 *    2. the normalised median test (Westerweel & Scarano 2005; piv_correlation.normalized_median_test) over the 3 x 3
 *       neighbourhood: the neighbours are the up to 8 nodes inside the grid whose total is not NaN, m of them.  Per
 *       component: med = median of the neighbours' values, rm = median of |value - med|, r = |t - med| / (rm + eps).
 *       The median of m sorted values is (v[(m-1)/2] + v[m/2]) / 2 (integer division).  The node is an outlier when
 *       its total is NaN, or when m > 0 and r_x r_x + r_y r_y > threshold threshold (no square root; a NaN score, 0/0,
 *       is no outlier).
 *    3. an outlier takes, per component, the median of its neighbours that are not outliers themselves (and not NaN),
 *       (0, 0) where there is none (piv_correlation.predictor without the rounding); every other node keeps t.
 *    4. d_status int[n] = d_flags[k], bit 8 added on every outlier.
 *    5. d_field f32[n][2] = the result of step 3, rounded to f32 (what a caller reports).  d_smooth f32[n][2], or
 *       NULL: the 3 x 3 binomial filter of the f64 result of step 3, h(i, j) = ((v(i, j-1) + 2 v(i, j)) + v(i, j+1)) / 4
 *       along each row, then ((h(i-1, j) + 2 h(i, j)) + h(i+1, j)) / 4 along each column, indices clamped to the grid
 *       (edge values replicated), rounded once to f32: the predictor of the next iteration.
 *    The device returns the model's status bit for bit, and its field and smooth values bit for bit.  d_pred must
 *    not be one of the outputs (a node reads its neighbours' predictors).  Refused: n_rows or n_cols < 1, more than
 *    INT_MAX nodes, eps < 0 or not finite, threshold <= 0 or not finite, a null d_vectors, d_flags, d_field or
 *    d_status, d_pred == d_field or d_smooth.
 * Every refusal: 1, one stderr line, nothing written, no launch.
 *
 * Driver (PhotonLibrary.correlate_deform; piv_deformation.correlate_deform_model): the coefficients of both frames
 * once; pass 0 = photon_piv_correlate on the images with `radius`, validate with pred NULL -> F_1 = its d_smooth;
 * iteration k = 1 .. iterations: warp frame 1 by -F_k / 2 and frame 2 by +F_k / 2, correlate the warped pair with
 * residual_radius, validate with pred = F_k -> d_field the result of iteration k, d_smooth = F_k+1 (smooth off: d_field
 * is passed on).  Known limits: the median test's one-sided neighbourhoods flag most border nodes of a strongly
 * rotating field, which then take interior medians; a window whose warped footprint leaves the frame correlates
 * mirrored particles, and section 5's bit 4 is not raised for that. */
int photon_piv_bspline_coefficients(const float *d_im, int width, int height, float *d_coef, void *stream);
int photon_piv_deform(const float *d_coef, int width, int height, const float *d_field, int field_stride, int n_rows,
                      int n_cols, int win, int step, float scale, float *d_out, void *stream);
int photon_piv_validate(const float *d_pred, const float *d_vectors, const int *d_flags, int n_rows, int n_cols, double eps,
                        double threshold, float *d_field, float *d_smooth, int *d_status, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 8: dot tracking on an image pair (BOS dot patterns, particle tracking): find the dots of each image, locate
 * each to a fraction of a pixel, pair the dots of the two frames and report one shift per dot -- the measurement that
 * matches the per-dot truth of photon_trace_moments one to one, where sections 5 and 7 measure window averages.  Host
 * model: photon_amd/dot_tracking.py (f64); driver: PhotonLibrary.track_dots.  Coordinates are index coordinates as in
 * section 5: x = column, y = row, the centre of pixel (r, q) at (x, y) = (q, r).
 * Every entry point is asynchronous on `stream`, takes the capacities of its arrays from the caller and reads the number
 * of dots from device memory (a count below 0 reads as 0, one above the capacity as the capacity), so the chain
 * detect -> fit -> match -> window means runs without a host wait in between.  Device scratch comes from the CALLER
 * (d_scratch of at least photon_dots_*_scratch_bytes bytes, 16-byte aligned, not shared by calls that may overlap in
 * time; its contents afterwards are unspecified); the entry points allocate nothing.  d_dots, d_shift and d_vectors
 * (four floats per entry) must be 16-byte aligned.  Two calls on the same inputs
 * return identical bytes: every output order and every summation order is fixed, and where atomics are used (integer
 * counts, a maximum, the order of the cell lists inside the scratch) no output depends on the order in which they land.
 * Every refusal: 1, one stderr line, nothing written, no launch.
 *
 * photon_dots_image_max: *d_max = the largest finite pixel, 0 when there is none above 0 (so that a threshold can be a
 *    fraction of the maximum without a host wait).  Refused: width or height < 1, a null pointer.
 *
 * a. Detect.  The effective threshold is T = threshold * *d_scale, one f32 product (d_scale: a device f32, NULL = 1).
 *    Pixel (r, q) with 1 <= r <= height - 2, 1 <= q <= width - 2 is a peak when its value v is finite, v > T, v > each of
 *    the four neighbours that precede it in row-major order (NW, N, NE, W) and v >= each of the four that follow (E, SW,
 *    S, SE); a comparison with a NaN neighbour counts as passed (a plateau yields its first pixel in row-major order
 *    whose preceding neighbours are all lower).  d_peaks int[max_dots] receives the pixel indices r width + q in
 *    increasing order; *d_count the total number found, which may exceed max_dots, in which case the first max_dots are
 *    written.  Entries beyond the count are not written.  The device equals the model exactly.
 *    Refused: an image smaller than 3 x 3, more than INT_MAX pixels, max_dots < 1, a threshold that is not finite, a null
 *    d_im, d_peaks, d_count or d_scratch, a scratch smaller than photon_dots_detect_scratch_bytes(width, height).
 *
 * b. Locate.  Dot k < min(*d_count, max_dots) has its peak at pixel d_peaks[k] = r width + q.  With
 *    I(p) = max(im(p) - background, 0) in f64, pixels outside the image and non-finite pixels reading 0:
 *    1. start: per axis the 3-point fit of section 5 (Gaussian where all three of I-, I0, I+ are positive, parabolic
 *       otherwise, 0 for a zero denominator) through the peak pixel, in f64: (x, y) = (q + delta_x, r + delta_y).
 *    2. `iterations` rounds (0 .. 16) of the Gaussian-weighted centroid over the (2 box_radius + 1)^2 box centred on the
 *       PEAK PIXEL (box_radius 1 .. 7): w(p) = I(p) exp(-(p_x - x)^2 / (2 sigma_w^2)) exp(-(p_y - y)^2 / (2 sigma_w^2)),
 *       (x, y) <- sum w p / sum w, in f64.  The weight is separable: 2 (2 box_radius + 1) exponentials per round.  A round
 *       whose sum w is not > 0 leaves (x, y) alone and sets status bit 4.
 *    3. after the last round, with the final (x, y) and its weights: v = sum w ((p_x - x)^2 + (p_y - y)^2) / (2 sum w),
 *       the weighted variance per axis; the dot's own variance s2 = v sigma_w^2 / (sigma_w^2 - v) - 1/12 (pixel
 *       integration); diameter = 4 sqrt(s2) (the e^-2 diameter of piv_correlation.particle_image), NaN when iterations
 *       = 0, when sum w is not > 0, or when s2 is not finite or not > 0.
 *    d_dots f32[max_dots][4] = (x, y, I at the peak pixel, diameter), rounded once from f64; d_status int[max_dots] bits:
 *    1 the box leaves the image; 2 the final position lies more than 1 px from the peak pixel's centre in either axis (the
 *    position is reported as it is, the bit is a warning: a neighbour pulled the centroid); 4 as above; 8 d_peaks[k] is
 *    no pixel index of the image (the dot is NaN).  Entries k >= the count are not written.  The device sums in f64 in
 *    its own fixed order (each row of the box left to right, the rows folded pairwise): it agrees with the model to
 *    rounding, not bit for bit.
 *    Refused: width or height < 1, more than INT_MAX pixels, max_dots < 1, box_radius or iterations out of range,
 *    sigma_w not finite or <= 0, background not finite, a null pointer.
 *
 * c. Pair.  Dots and status of frame 1 and frame 2 (section 8b's arrays; d_status1 / d_status2 may be NULL) with their
 *    counts on the device.  A dot takes part when both coordinates are finite and (status & reject_mask) = 0.
 *    Predictor: d_field (NULL = none), field_stride, n_rows, n_cols, win, step exactly as section 7b takes them (win any
 *    size >= 1 here), evaluated at the dot's own continuous position (x, y) by 7b's bilinear rule in f32, one IEEE
 *    operation per step: fy = clamp((y - (win-1)/2) / step, 0, n_rows - 1), i = min(floor(fy), max(n_rows - 2, 0)),
 *    wy = fy - i, likewise fx, j, wx; T = F(i, j) + wx (F(i, j+1) - F(i, j)), U the same on row min(i + 1, n_rows - 1),
 *    pred = T + wy (U - T); a vector with a component that is not finite reads as (0, 0).
 *    Target of dot i of frame 1: t_i = p_i + pred(p_i) (f32; a target that is not finite takes no part).  For a target t
 *    and a dot p of frame 2, d2 = (p_x - t_x)(p_x - t_x) + (p_y - t_y)(p_y - t_y) in f32 without contraction.
 *    j*(i): the dot of frame 2 with the smallest d2 to t_i among those with d2 <= radius radius (one f32 product), ties
 *    to the smallest j; i*(j): the target with the smallest d2 to p_j under the same rule, ties to the smallest i.  Dot
 *    i is paired with j when j = j*(i) and i = i*(j).
 *    d_pair int[max1] = j or -1; d_shift f32[max1][4] = (x_mid, y_mid, dx, dy) with d = p2_j - p1_i and mid = p1_i +
 *    d / 2 (f32), NaN for an unpaired dot; *d_npaired the number of pairs.  Entries beyond the count of frame 1 are not
 *    written.  The device equals the brute-force model exactly.  The search runs on a uniform grid of cells of
 *    max(1.001 radius, 8, max(width, height) / 2048) pixels over the image (positions beyond it fall into the border
 *    cells) and visits 3 x 3 cells.
 *    Refused: width or height < 1, max1 or max2 < 1, radius not finite or <= 0, a null d_dots, d_count, d_pair, d_shift,
 *    d_npaired or d_scratch, with a field: field_stride not 2 or 4, win or step < 1, an image smaller than one window,
 *    a grid that is not section 5's; a scratch smaller than photon_dots_match_scratch_bytes(width, height, radius, max1, max2).
 *
 * d. Onto the window grid, so that tracked dots feed photon_piv_validate and photon_integrate_gradient unchanged.  For
 *    section 5's grid of (height, width, win, step) (win any size >= 1): window (i, j) owns a paired dot (d_pair >= 0,
 *    shift finite) when the pixel its anchor falls in, (floor(x + 1/2), floor(y + 1/2)) in f64, lies in the window
 *    (piv_correlation.window_truth's rule); anchor 0 = the frame-1 position d_dots1 (what section 5 measures), 1 = the
 *    midpoint of d_shift (what section 7 measures).  d_vectors f32[n][4] = (mean dx, mean dy, count, rms), in f64, the
 *    sums in increasing dot index: mean = sum / count, rms = sqrt(sum ((dx - mean dx)^2 + (dy - mean dy)^2) / count),
 *    each rounded once to f32; d_flags int[n] = 2 (section 5's "no data" bit; dx, dy and rms NaN, the count kept) when
 *    count < min_count, else 0.  The device equals the model bit for bit.
 *    Refused: win or step < 1, an image smaller than one window, max1 < 1, min_count < 1, anchor not 0 or 1, more than
 *    INT_MAX windows, a null pointer. */
size_t photon_dots_detect_scratch_bytes(int width, int height);                     /* 0 for arguments detect refuses */
size_t photon_dots_match_scratch_bytes(int width, int height, float radius, int max1, int max2);
int photon_dots_image_max(const float *d_im, int width, int height, float *d_max, void *stream);
int photon_dots_detect(const float *d_im, int width, int height, float threshold, const float *d_scale, int max_dots,
                       int *d_peaks, int *d_count, void *d_scratch, size_t scratch_bytes, void *stream);
int photon_dots_fit(const float *d_im, int width, int height, const int *d_peaks, const int *d_count, int max_dots,
                    int box_radius, double sigma_w, int iterations, double background, float *d_dots, int *d_status,
                    void *stream);
int photon_dots_match(const float *d_dots1, const int *d_status1, const int *d_count1, int max1, const float *d_dots2,
                      const int *d_status2, const int *d_count2, int max2, int reject_mask, const float *d_field,
                      int field_stride, int n_rows, int n_cols, int win, int step, float radius, int width, int height,
                      int *d_pair, float *d_shift, int *d_npaired, void *d_scratch, size_t scratch_bytes, void *stream);
int photon_dots_window_means(const float *d_dots1, const int *d_pair, const float *d_shift, const int *d_count1, int max1,
                             int width, int height, int win, int step, int min_count, int anchor, float *d_vectors,
                             int *d_flags, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 9: tomography -- the 3-D field f (rho - rho_0 on a voxel grid) from several views' projected density
 * P = int (rho - rho_0) ds (section 6's result): a ray-driven projector A, its exact adjoint, and a conjugate-gradient
 * solver of the regularised weighted normal equations.  Host model: photon_amd/tomography.py (numpy f64, the same
 * operations in the same order).
 *
 * Grid.  nx x ny x nz nodes of f64, voxel (i, j, k) at (k ny + j) nx + i (the order of the NRRD volumes); node position
 * origin + (i, j, k) spacing in world microns; every dimension >= 2, nx ny nz <= INT_MAX.
 * Rays.  n_rays infinite lines: d_origins f64[n_rays][3], d_dirs f64[n_rays][3] (need not be unit vectors).
 *
 * Projector (Joseph's method), per ray, every step one IEEE f64 operation in the order written (the library is built
 * without contraction):
 *   1. n2 = (dx dx + dy dy) + dz dz;  len = sqrt(n2);  e = (dx / len, dy / len, dz / len).  The ray is a miss when one of
 *      its six numbers is not finite, or when len is not finite or not > 0.
 *   2. Dominant axis a: a = x; a = y when |e_y| > |e_x|; a = z when |e_z| > |e_a| (ties keep the first axis).  b < c are
 *      the other two axes.  scale = spacing_a / |e_a|.
 *   3. For every plane kappa = 0 .. n_a - 1 in ascending order: plane = origin_a + kappa spacing_a;
 *      t = (plane - o_a) / e_a;  u = ((o_b + t e_b) - origin_b) / spacing_b;  v = ((o_c + t e_c) - origin_c) / spacing_c.
 *      The plane counts when 0 <= u <= n_b - 1 and 0 <= v <= n_c - 1 (closed; a NaN fails).
 *      i_b = min(floor(u), n_b - 2), f_b = u - i_b, g_b = 1 - f_b; likewise i_c, f_c, g_c.
 *   4. The four taps of a counted plane, in this order, with their weights:
 *      (i_b, i_c): (g_b g_c) scale;  (i_b + 1, i_c): (f_b g_c) scale;  (i_b, i_c + 1): (g_b f_c) scale;
 *      (i_b + 1, i_c + 1): (f_b f_c) scale, each at voxel kappa along a.
 *   5. P = sum of weight * f[tap], one product and one addition per tap, from 0, in the order of the planes and taps.
 *      A ray with no counted plane, and a miss, gives P = 0.
 * photon_tomo_project writes d_p f64[n_rays] = A f.  It equals the model bit for bit wherever the host's sqrt, floor and
 * division are correctly rounded.
 *
 * Adjoint.  photon_tomo_backproject ADDS A^T y into d_v f64[nx ny nz]: d_v[tap] += weight * d_y[ray] over exactly the
 * taps above (a ray whose y is 0 adds nothing).  The caller zeroes d_v when it wants A^T y alone.  The adds are f64
 * atomics: the order in which the terms of one voxel arrive is not fixed, so two calls may differ in the last bits.  No
 * bit-repeatability is claimed for photon_tomo_backproject or photon_tomo_reconstruct.
 * Both are asynchronous on `stream`; every pointer is a device pointer (spacing and origin are host arrays of three).
 * Refused (1, one stderr line, nothing written, no launch): a dimension < 2, nx ny nz > INT_MAX, n_rays < 1, a spacing
 * that is not finite or not > 0, an origin that is not finite, a null pointer.
 *
 * Solver.  photon_tomo_reconstruct minimises  sum_i w_i (A f - p)_i^2 + lambda h^2 |G f|^2  over f with f = 0 wherever
 * the support mask is 0: h = min(spacing); lambda >= 0 has no unit; G the forward first differences along the three
 * axes, unscaled, so that G^T G is the 6-neighbour graph Laplacian  (G^T G q)_c = sum over the neighbours n of c inside
 * the grid of (q_c - q_n), added in the order -x, +x, -y, +y, -z, +z.
 *   d_p        f64[n_rays] the measured projections
 *   d_w        f64[n_rays] weights, or NULL (1).  A ray whose p or w is not finite, or whose w <= 0, has weight 0 and its
 *              p reads as 0.
 *   d_support  u8[nx ny nz] (nonzero = unknown), or NULL (every voxel).  m below is the 0/1 mask.
 *   d_f        f64[nx ny nz] out: the solution, exactly 0 off the support
 * Conjugate gradients on the normal equations from x = 0, in f64:
 *   b = m (A^T (W p));  r = b;  q = r;  rho = r.r.   |b| = 0: 0 iterations, converged.
 *   per iteration:  s = m (A^T (W (A q)) + (lambda h h) G^T G q);  alpha = rho / (q.s), 0 when q.s = 0;  x += alpha q;
 *   r -= alpha s;  rho' = r.r;  beta = rho' / rho, 0 when rho = 0;  q = r + beta q.
 * |r| <= tol |b| is checked before the first iteration and then every PHOTON_TOMO_CHECK_EVERY iterations; with tol > 0
 * the solver stops at the first check that holds, else after exactly max_iter iterations (tol = 0: always max_iter).
 * alpha and beta stay on the device; the dot products are summed in an order the grid size alone fixes (the adjoint's
 * sums are not, see above).  Plain stream launches, no graph; `stream` is synchronised before the call returns.
 *   stats      iterations run; converged = final |r| <= tol |b|; residual = final |r| / |b| (0 when |b| = 0); unknowns =
 *              support voxels; rays_used = rays of weight > 0 with at least one counted plane.  May be NULL.
 * Refused as above, and: lambda < 0 or NaN, tol < 0 or NaN, max_iter < 0, a null d_p, d_origins, d_dirs or d_f. */
#define PHOTON_TOMO_CHECK_EVERY 8

typedef struct photon_tomo_stats_t {
    int iterations, converged;
    long long unknowns, rays_used;
    double residual;
} photon_tomo_stats_t;

int photon_tomo_project(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                        const double *d_origins, const double *d_dirs, long long n_rays, double *d_p, void *stream);
int photon_tomo_backproject(const double *d_y, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                            const double *d_origins, const double *d_dirs, long long n_rays, double *d_v, void *stream);
int photon_tomo_reconstruct(const double *d_p, const double *d_w, const unsigned char *d_support, int nx, int ny, int nz,
                            const double spacing[3], const double origin[3], const double *d_origins, const double *d_dirs,
                            long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                            photon_tomo_stats_t *stats, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 10: tomography from deflections -- the 3-D field f from the measured ray deflections themselves (section 6's
 * input, bos_density.gradients_from_displacements: int grad_perp (rho - rho_0) ds along each chief ray), without first
 * integrating every view to a projected density.  Host model: photon_amd/tomography.py (deflection_taps, deflect_model,
 * deflect_adjoint_model, reconstruct_deflections_model; the same operations in the same order).
 *
 * Grid and rays as in section 9.  Per ray two transverse vectors d_t1, d_t2 f64[n_rays][3] in world coordinates; they
 * need not be unit vectors and need not be perpendicular to the ray.  A zero vector is allowed: that component is then 0
 * for every f (single-component data).  A ray with an entry of t1 or t2 that is not finite is a miss.
 *
 * Operator.  D_tau is the exact derivative of section 9's projector under a parallel shift of the ray:
 *   (D_tau f)(o, d) = d/d delta  (A f)(o + delta tau, d)  at delta = 0.
 * Inside a cell A is bilinear in (u, v), so D_tau has the four taps of every plane that counts for A with differentiated
 * weights.  Steps 1 to 3 of section 9 are unchanged (the same planes count, the same i_b, f_b, g_b, i_c, f_c, g_c and
 * scale).  Then, every step one IEEE f64 operation in the order written:
 *   3a. per ray and vector tau, a the dominant axis:  r = tau_a / e_a;
 *       p_u = ((tau_b - r e_b) / spacing_b) scale;  p_v = ((tau_c - r e_c) / spacing_c) scale.
 *   4.  per counted plane  A = g_c p_u,  B = g_b p_v,  C = f_c p_u,  E = f_b p_v,  and the weights of section 9's taps in
 *       section 9's order:  (i_b, i_c): (-A) - B;  (i_b + 1, i_c): A - E;  (i_b, i_c + 1): B - C;  (i_b + 1, i_c + 1): C + E.
 *   5.  g = sum of weight * f[tap], one product and one addition per tap, from 0, in the order of the planes and taps.
 * The four weights of a plane sum to 0 (D_tau annihilates constants); only the part of tau perpendicular to the ray
 * matters (tau parallel to e gives 0 up to rounding); and for a ray whose shifted copies o +- delta tau stay in the cells
 * of the original, (A f(o + delta tau) - A f(o - delta tau)) / (2 delta) = D_tau f up to rounding, because A is quadratic
 * along a shift inside a cell.
 *
 * photon_tomo_deflect writes d_g1 = D_t1 f and d_g2 = D_t2 f, f64[n_rays] each (one walk per ray); 0 for a miss and for
 * a ray with no counted plane.  It equals the model bit for bit under section 9's condition.
 * photon_tomo_deflect_adjoint ADDS D_t1^T y1 + D_t2^T y2 into d_v f64[nx ny nz]: per tap ONE value,
 * weight1 y1 + weight2 y2 (two products, one addition), so the number of atomic adds is photon_tomo_backproject's, not
 * twice it.  A ray with y1 = y2 = 0 adds nothing.  As in section 9 the order in which a voxel's terms arrive is not fixed:
 * no bit-repeatability is claimed for photon_tomo_deflect_adjoint or photon_tomo_reconstruct_deflections.
 * Both are asynchronous on `stream`.  Refused as section 9's operators (1, one stderr line, nothing written, no launch),
 * a null d_t1, d_t2, d_g1, d_g2, d_y1 or d_y2 included.
 *
 * Solver.  photon_tomo_reconstruct_deflections minimises
 *   sum_i w_i ((D_t1 f - g1)_i^2 + (D_t2 f - g2)_i^2) + lambda |G f|^2
 * over f with f = 0 off the support; G as in section 9.  There is NO h^2 on the regulariser: D carries 1 / length against
 * A, so lambda stays without a unit and comparable to section 9's.  A ray whose g1, g2 or w is not finite, or whose
 * w <= 0, has weight 0 and its data read as 0.  The iteration is section 9's with
 *   b = m (D_t1^T (W g1) + D_t2^T (W g2));  s = m (D_t1^T (W (D_t1 q)) + D_t2^T (W (D_t2 q)) + lambda G^T G q),
 * both adjoints in one photon_tomo_deflect_adjoint; the check cadence, the stats (rays_used = rays of weight > 0 that are
 * no miss and have a counted plane), alpha and beta on the device and the single wait at the end are section 9's.
 * With d_support == NULL the constant of f is undetermined by the data (D annihilates constants, and so does G): CG from 0
 * stays orthogonal to the constants and returns the solution of zero mean.  A support whose border lies in the ambient
 * fluid (f = 0 off it) fixes the constant.
 * Refused as photon_tomo_reconstruct, and: a null d_g1, d_g2, d_t1 or d_t2. */
int photon_tomo_deflect(const double *d_f, int nx, int ny, int nz, const double spacing[3], const double origin[3],
                        const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2, long long n_rays,
                        double *d_g1, double *d_g2, void *stream);
int photon_tomo_deflect_adjoint(const double *d_y1, const double *d_y2, int nx, int ny, int nz, const double spacing[3],
                                const double origin[3], const double *d_origins, const double *d_dirs, const double *d_t1,
                                const double *d_t2, long long n_rays, double *d_v, void *stream);
int photon_tomo_reconstruct_deflections(const double *d_g1, const double *d_g2, const double *d_w, const unsigned char *d_support,
                                        int nx, int ny, int nz, const double spacing[3], const double origin[3],
                                        const double *d_origins, const double *d_dirs, const double *d_t1, const double *d_t2,
                                        long long n_rays, double lambda, double tol, int max_iter, double *d_f,
                                        photon_tomo_stats_t *stats, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 11: displacement uncertainty per vector from correlation statistics (Wieneke 2015): the a posteriori
 * uncertainty (sigma_x, sigma_y) in pixels of section 5's estimator, from the converged image pair alone.  Host model:
 * photon_amd/piv_uncertainty.py (uncertainty_model, f64); driver: PhotonLibrary.displacement_uncertainty.
 *   d_im1, d_im2  device f32[height*width], row-major: a MATCHED pair -- both frames warped by the field whose
 *             uncertainty is asked for (photon_piv_deform with scale -1/2 on frame 1 and +1/2 on frame 2), so that
 *             what is left between them is noise.  The call does not warp.
 *   win, step and the window grid (n_rows, n_cols, window k = i n_cols + j) are section 5's, at zero offset.
 *   reach     K in [0, 4]: the neighbourhood over which the covariance of the pixel contributions is summed.
 * All arithmetic is f64 on the f32 pixels.  Per window: a, b the win^2 pixels of im1, im2; ma, mb their means;
 * A = a - ma, B = b - mb.  The window is flat when all pixels of a are equal or all pixels of b are equal (decided from
 * the smallest and the largest pixel, as in section 5): flag 2, both sigma and all eight stats NaN.
 * Axis x, e = one column, pixel set P = {(r, q): q <= win - 2} (axis y: rows and columns swap roles, e = one row,
 * P = {(r, q): r <= win - 2}):
 *   d(p)  = A(p) B(p + e) - A(p + e) B(p)                       (the two products are separate IEEE multiplications: identical
 *                                                               frames give d = 0 exactly)
 *   C1    = 1/2 sum_P [A(p) B(p + e) + A(p + e) B(p)]            the correlation at shift +-e, symmetrised
 *   C0    = 1/2 sum_P [A(p) B(p) + A(p + e) B(p + e)]            the correlation at zero shift over the same pixels
 *   S(D)  = sum d(p) d(p + D) over the p with p and p + D both in P
 *   V     = S(0) + 2 sum_{D in H_K} S(D),  H_K = {(Dr, Dq): 0 <= Dr <= K, |Dq| <= K, Dr > 0 or Dq > 0}: S is symmetric
 *           in D, so this is the sum over the full (2K + 1)^2 neighbourhood -- the variance of C(+e) - C(-e) with the
 *           spatial covariance of its terms out to K pixels.
 *   V < 0 or NaN:  V = S(0), flag 32.
 *   s = sqrt(V), lo = C1 - s/2, hi = C1 + s/2.
 *   lo > 0 and C0 > 0:  num = ln hi - ln lo,  den = (4 ln C0 - 2 ln lo) - 2 ln hi    (section 5's three-point Gaussian
 *                       fit through (lo, C0, hi): the peak displaced by +-s/2)
 *   otherwise:          num = hi - lo,        den = 4 (C0 - C1)                      (the parabolic fit)
 *   sigma = num / den when den > 0; otherwise sigma = NaN, flag 16 (no maximum at zero shift: the pair is not matched).
 * The mean-subtracted products and the fit are section 5's on purpose: sigma is the uncertainty of that estimator.
 *   d_sigma   device f32[n][2] (sigma_x, sigma_y), each rounded once from f64
 *   d_flags   device int[n], bits: 2 flat window, 16 no maximum at zero shift (either axis), 32 V < 0 replaced by S(0)
 *             (either axis)
 *   d_stats   device f64[n][2][4] or NULL: (C0, C1, S(0), V) of axis x, then of axis y; V as summed, before the
 *             replacement of flag 32
 * d_sigma == NULL: only *n_rows / *n_cols are written; nothing is launched.
 * Refused (1, one stderr line, nothing written, no launch): win not 16 / 32 / 64, step < 1, reach outside [0, 4], an
 * image smaller than one window, a null image pointer, d_sigma without d_flags.  Asynchronous on `stream`, no device
 * scratch.  Every sum has a fixed order: two calls on the same inputs return the same bits.  The device sums V as
 * sum_p d(p) (d(p) + 2 sum_{H_K} d(p + D)) and need not agree with the model to the last bit: tests hold the stats to the
 * model within 1e-11 of the sums of the absolute terms.
 * Known limits: correlation statistics see the noise of the pair only -- not bias, peak locking, or the truncation
 * error of a field that varies inside a window; sigma underestimates the error where those dominate (low image noise,
 * win 16): DESIGN.md section 4.3h. */
int photon_piv_uncertainty(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int reach,
                           float *d_sigma, int *d_flags, double *d_stats, int *n_rows, int *n_cols, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 12: dense optical flow on an image pair (Horn & Schunck 1981; Brox et al. 2004; Atcheson et al. 2009 for BOS):
 * one displacement vector per pixel where sections 5, 7 and 8 report one per window or dot.  The flow refines a predictor
 * (a correlation's field) and has no image pyramid.  Host model: photon_amd/optical_flow.py; driver:
 * PhotonLibrary.optical_flow.  Every call is asynchronous on `stream`, allocates nothing (scratch comes from the caller)
 * and returns the same bits for the same inputs.  Inputs are finite f32; a pixel or a vector that is not finite is outside
 * the contract, except where section 7b's rule is inherited.  A dense field is f32[height*width][2] = (dx, dy) per pixel,
 * row-major.
 *
 * a. photon_piv_field_to_pixels.  d_dense = section 7b's dense displacement D of the grid field (d_field, field_stride,
 *    n_rows, n_cols, win, step as section 7b takes them) at every pixel, in exactly the f32 operations of photon_piv_deform
 *    (the same device function); a vector with a component that is not finite reads as (0, 0).
 *    Refused: section 7b's rules for win, step, the image size (a side of more than 2^22 pixels included) and the grid,
 *    field_stride not 2 or 4, a null pointer.
 *
 * b. photon_piv_deform_dense.  Section 7b's warp with D read per pixel from d_dense instead of interpolated:
 *    s = clamp(scale D, -2^24, 2^24), the same taps, weights and order (one kernel template over where D comes from):
 *    photon_piv_deform_dense of photon_piv_field_to_pixels(F) equals photon_piv_deform(F) bit for bit.
 *    Refused: width or height < 1 or larger than 2^22, a scale that is not finite, a null pointer, d_out == d_coef.
 *    Limit at a pedestal: the warp sums 16 f32 taps of coefficients as large as the image, so its error grows with the
 *    pedestal and not with the signal.  Frames in camera counts with a pedestal of 61000 under a signal of 4000 counts
 *    (uint16) move the flow of the optical-flow driver by 3.7e-5 px against the f64 model (measured on an MI355X; 4e-7 px
 *    at a pedestal of 64), where frames of amplitude 1 stay within 3e-5 px, and the sigma of the uncertainty driver (section
 *    11 behind this warp and section 7b's) by 1.2e-4 of itself against its f64 model (1e-6 at a pedestal of 64), where the
 *    kernel alone stays within 1e-5.  A caller who needs more subtracts the pedestal
 *    first (section 15); the flow does not depend on a constant.  tests/test_driver_inputs_gpu.py holds the figure.
 *
 * c. photon_optflow_terms.  d_w1, d_w2: a matched pair, frame 1 warped by -u0 / 2 and frame 2 by +u0 / 2; d_u0 the dense
 *    field u0 they were warped by, or NULL for a zero field.  d_terms f32[height*width][4] = (Ix, Iy, c, w) per pixel
 *    (row r, column q), every step one IEEE f32 operation in this order:
 *      a = gain w1, b = gain w2, m = (a + b) 0.5
 *      Ix = ((m(q-2) - m(q+2)) + 8 (m(q+1) - m(q-1))) / 12 along the row, Iy the same along the column, indices by
 *           section 7's whole-sample mirror
 *      It = b - a
 *      c  = (It - Ix u0x) - Iy u0y
 *      w  = 1 / ((alpha2 + Ix Ix) + Iy Iy)
 *    Refused: width or height < 1, gain or alpha2 not finite or not > 0, a null d_w1, d_w2 or d_terms.
 *
 * d. photon_optflow_iterate.  `iterations` Jacobi sweeps of Horn-Schunck on the total field, starting from d_u.  Per
 *    pixel, neighbour indices clamped to the image (Neumann boundary), all pixels updated from the previous sweep:
 *      ub = ((u(q-1) + u(q+1)) + (u(r-1) + u(r+1))) 0.25, vb likewise
 *      rho = ((Ix ub + Iy vb) + c) w
 *      u' = ub - Ix rho, v' = vb - Iy rho
 *    This relaxes the Euler-Lagrange equations of  sum (Ix du + Iy dv + It)^2 + alpha2 |grad (u0 + du)|^2  (du = u - u0;
 *    alpha2 counted per 4-neighbour average).  The result is always in d_out; iterations = 0 copies d_u.  One launch
 *    performs up to T = photon_optflow_iterations_per_launch() sweeps (a workgroup recomputes a halo of T pixels around
 *    its tile; the halo clamps by image coordinates, so the bits are those of single sweeps); d_tmp f32[height*width][2]
 *    is needed only when iterations > T and may be NULL otherwise.
 *    Refused: width or height < 1, iterations < 0, a null d_terms, d_u or d_out, d_out == d_u, d_tmp equal to either,
 *    iterations > T without d_tmp.
 *
 * e. photon_optflow_iterations_per_launch: T, a pure query (PHOTON_OPTFLOW_SWEEPS = 1 .. 8 overrides it for measurements).
 * Every refusal: 1, one stderr line, nothing written, no launch.
 *
 * Driver (PhotonLibrary.optical_flow; optical_flow.optical_flow_model): the coefficients of both frames once; the
 * predictor spread to pixels (a) -- None: one iteration of correlate_deform; gain = 1 / std(frame 1); per warp: (b) on
 * frame 1 with scale -1/2 and on frame 2 with +1/2, (c) with the current field, (d).
 * Known limits: quadratic penalties only (no robust norm: the field is smoothed across a discontinuity); no pyramid -- a
 * predictor off by more than about a particle diameter is not recovered; the field refers to the mid-point frame, as in
 * section 7.  DESIGN.md section 4.3i. */
int photon_piv_field_to_pixels(const float *d_field, int field_stride, int n_rows, int n_cols, int win, int step, int width,
                               int height, float *d_dense, void *stream);
int photon_piv_deform_dense(const float *d_coef, int width, int height, const float *d_dense, float scale, float *d_out,
                            void *stream);
int photon_optflow_terms(const float *d_w1, const float *d_w2, int width, int height, const float *d_u0, float gain, float alpha2,
                         float *d_terms, void *stream);
int photon_optflow_iterate(const float *d_terms, const float *d_u, int width, int height, int iterations, float *d_out,
                           float *d_tmp, void *stream);
int photon_optflow_iterations_per_launch(void);

/* ------------------------------------------------------------------------------------
 * Section 13: windowed FFT correlation of an image pair on the device: circular cross-correlation (mode 0) and robust
 * phase correlation (mode 1; Eckstein & Vlachos 2009).  Where section 5 correlates amplitudes -- whatever does not move
 * between the frames competes with the particles -- mode 1 keeps the phase of the cross spectrum only, weighted by the
 * spectrum of a particle image; and the cost does not grow with the search radius.  Host models: photon_amd/piv_phase.py
 * (correlate_phase_model_f32: this section operation by operation; correlate_phase_model: f64 on a library FFT).
 *
 * Grid, window numbering, d_offset, d_vectors [n][4] = dx, dy, peak, ratio, d_flags, the sign of a displacement and the
 * size query with d_vectors == NULL are section 5's; d_planes is f32[n][(2R+1)^2] in section 5's layout, the central crop
 * of the window's circular win x win plane.  photon_piv_validate, photon_piv_uncertainty, photon_piv_deform and every
 * driver take the result as they take section 5's.
 *   win 16, 32 or 64;  step >= 1;  radius R in [1, win/2 - 1] (a circular plane cannot tell +win/2 from -win/2)
 *   mode 0 / 1;  window_sigma >= 0 (0: no weighting);  diameter >= 0: the e^-2 particle diameter d in pixels (0: W = 1)
 *
 * Definition.  a = im1 over the window, b(p) = im2(p + o) over the window moved by the offset; a pixel of im2 outside the
 * image reads as the mean of the in-image ones (contributes 0) and sets flag 4.
 *   a' = (a - mean a) g(row) g(col),  b' likewise,  g(p) = exp(-(p - (win-1)/2)^2 / (2 window_sigma^2))
 *   A, B = the 2-D DFTs of a', b' (X(k) = sum_p x(p) exp(-2 pi i k p / win));  S = conj(A) B
 *   mode 0:  P(s) = sum_k S(k) exp(+2 pi i k s / win),  Cn = P / (win^2 sqrt(sum a'^2 sum b'^2))   (|Cn| <= 1)
 *   mode 1:  P(s) = sum_k W(k) S(k) / |S(k)| exp(+2 pi i k s / win),  Cn = P / sum_k W(k)         (1 for a pure shift)
 *            W(kx, ky) = w(kx) w(ky),  w(k) = exp(-(d^2 / 16) (2 pi f / win)^2),  f = k below win/2 and k - win from there
 *            on.  A bin with |S| = 0 contributes 0, and so does k = (0, 0) in every window: the means are subtracted, what
 *            rounding leaves there has no phase.  sum W runs over the other bins: (sum_k w(k))^2 - 1.
 * The plane holds Cn(s) for s in [-R, R]^2.  Integer peak with the row-major tie rule, the f64 three-point fit, the ratio
 * and flags 1 and 2 are section 5's on that plane.  Flag 2 (every output NaN): all pixels of a equal, all in-image pixels
 * of b equal or none -- decided from the smallest and the largest pixel -- or an f32 energy sum a'^2, sum b'^2 not above 0.
 *
 * The f32 order is part of the contract: the planes, peaks and ratios equal correlate_phase_model_f32's value for value
 * (dx, dy up to the f64 logarithm).  Every operation below is one IEEE f32 operation, nothing fused:
 *   sums       sum of win^2 values v = every row from its first column on (r = r + v), then the win row sums by halving:
 *              r_i = r_i + r_(i+h) for i < h, h = win/2, win/4 ... 1.  An outside pixel of b adds 0.
 *   means      mean a = sum a / win^2;  mean b = sum b / (number of in-image pixels)
 *   weights    a' = ((a - mean a) g(row)) g(col);  b' the same, 0 for an outside pixel;  energies = sums of a' a', b' b'
 *   forward    z = a' + i b'; radix-2 decimation in frequency along every row, then along every column, natural order in,
 *              bit-reversed order out: for h = win/2 ... 1, for every block of 2h elements and j < h, with u = x(j),
 *              v = x(j + h), t = twiddle(j win / (2h)):  x(j) = u + v,  x(j + h) = (u - v) t.
 *              A product (c + i d)(t_r + i t_i) is (c t_r - d t_i) + i (c t_i + d t_r).
 *   spectra    with Z- = Z(-k):  A_r = Z_r + Z-_r,  A_i = Z_i - Z-_i,  B_r = Z_i + Z-_i,  B_i = Z-_r - Z_r   (2 A, 2 B)
 *              S_r = A_r B_r + A_i B_i,  S_i = A_r B_i - A_i B_r                                                (4 S)
 *              mode 1:  m = sqrt(S_r S_r + S_i S_i);  q = (w(ky) w(kx)) / m;  T = (S_r q, S_i q), 0 where m is not > 0
 *              or k = (0, 0);  mode 0: T = S
 *   inverse    radix-2 decimation in time along every column, then along every row, bit-reversed in, natural out, with
 *              t* = (t_r, -t_i): for h = 1 ... win/2:  x(j) = u + v t*,  x(j + h) = u - v t*.  P = the real part.
 *   scale      in f64:  mode 0  inv = 1 / ((4 win^2) sqrt(energy_a energy_b));  mode 1  inv = 1 / ((sum_k w(k))^2 - 1), the
 *              sum in the order of k;  Cn = (float)(P inv), peak likewise, ratio = (float)(P* / P2) as in section 5
 * Tables: twiddle(k) = (cos, -sin)(2 pi k / win) for k < win/2, g and w are f32 values rounded once from f64
 * (photon_det_sincos, photon_det_exp), filled on the host and handed to the kernel by value; the quarter turns are exactly
 * (1, 0) and (0, -1).  photon_piv_phase_tables writes the library's own tables to HOST memory (twiddles f32[win/2][2],
 * window f32[win], filter f32[win]) and launches nothing; it refuses a bad win, window_sigma or diameter and a null pointer.
 *
 * Refused (1, one stderr line, nothing written, no launch): section 5's list with R in [1, win/2 - 1], a mode other than
 * 0 / 1, a window_sigma or diameter that is negative or not finite.  Asynchronous on `stream`, no device scratch; two calls
 * on the same inputs return the same bits.
 * Known limits: the plane is circular -- a displacement beyond win/2 - 1 aliases; pixels that enter the window only after
 * the shift are not seen (section 5 enlarges the region instead), which the window weighting mitigates; images that are
 * not finite are outside the contract.  DESIGN.md section 4.3j. */
int photon_piv_correlate_phase(const float *d_im1, const float *d_im2, int width, int height, int win, int step, int radius,
                               const int *d_offset, int mode, float window_sigma, float diameter, float *d_vectors,
                               int *d_flags, float *d_planes, int *n_rows, int *n_cols, void *stream);
int photon_piv_phase_tables(int win, float window_sigma, float diameter, float *twiddles, float *window, float *filter);

/* ------------------------------------------------------------------------------------
 * Section 14: ensemble correlation (sum of correlation; Meinhart, Wereley & Santiago 2000): one displacement field from
 * n_pairs image pairs of one steady or periodic flow, a static BOS object or a seeding too sparse for single pairs.  The
 * correlation planes and the energies of the pairs are summed per window before the peak is read.  Host model:
 * photon_amd/piv_ensemble.py (correlate_ensemble_model, f64).
 *   pair k    (d_im1 + k pair_stride, d_im2 + k pair_stride), each device f32[height*width] as in section 5;
 *             pair_stride in floats, >= width height.  Two stacks [N][H][W]: stride H W.  A time series f0 .. fN in one
 *             buffer: d_im2 = d_im1 + H W, stride H W (pairs f_k, f_k+1).  Frame-straddled pairs: stride 2 H W.
 *   Grid, windows, d_offset (one integer predictor per window, shared by all pairs), d_flags and the layouts of
 *   d_vectors and d_planes are section 5's.
 * Per window: a_k, b_k, their means, C_k(s) and the energies ea_k, eb_k are section 5's for pair k, each pair
 * mean-subtracted by its own window means.  Pair k contributes unless its window is flat by section 5's rule (all pixels
 * of a_k equal, the in-image pixels of b_k at zero shift all equal or none, or an f32 energy not above 0).  Over the
 * contributing pairs, in pair order:
 *   C(s) = sum_k C_k(s),  Ea = sum_k ea_k,  Eb = sum_k eb_k,  Cn = C / sqrt(Ea Eb)
 * The integer peak with the row-major tie rule, the f64 three-point fit, peak = Cn(s*), the ratio and flag 1 are section
 * 5's on C.  Flag 4 is geometry, the same for all pairs.  No pair contributes: flag 2, every output of the window, its
 * plane included, NaN.
 *   d_count   device int[n], or NULL: the number of contributing pairs per window
 * Order (f32): every sum has a fixed order, two calls on the same inputs return the same bits.  Within a pair the row
 * slices of the plane are summed in section 5's order; the running totals start from the first contributing pair's
 * values, not from 0, so n_pairs = 1 returns section 5's vectors, flags and planes bit for bit.
 * d_vectors == NULL: the size query, as in section 5.  Refused (1, one stderr line, nothing written, no launch): section
 * 5's list, n_pairs < 1, pair_stride < width height.  Asynchronous on `stream`, no device scratch.  DESIGN.md section 4.3m. */
int photon_piv_correlate_ensemble(const float *d_im1, const float *d_im2, long long pair_stride, int n_pairs, int width,
                                  int height, int win, int step, int radius, const int *d_offset, float *d_vectors,
                                  int *d_flags, int *d_count, float *d_planes, int *n_rows, int *n_cols, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 15: image pre-processing of a stack or a time series on the device, the step in front of sections 5, 7, 13 and
 * 14: the background of the frames (what does not move: walls, reflections, the sensor's offset), and per frame the chain
 * subtract, clamp, min-max filter (Westerweel 1993; Adrian & Westerweel 2011, section 9: local contrast normalisation
 * against uneven illumination).  Host models: photon_amd/piv_preprocess.py (background_model, preprocess_model_f32: this
 * section operation by operation; preprocess_model: f64).
 *   frame k   d_frames + k frame_stride, device f32[height*width] as in section 5; frame_stride in floats, >= width height
 *             (section 14's addressing: a stack, every other frame of a straddled series through 2 H W, a series in one buffer)
 *   width, height in [1, 2^22]
 * Below, max(a, b) is "a if a > b, else b", one comparison and no arithmetic; every other operation is one IEEE f32 (where
 * said, f64) operation, nothing fused.
 *
 * photon_piv_background: d_out f32[height*width].
 *   mode 0    the minimum: m = frame_0(p); for k = 1 .. n-1: m = frame_k(p) if frame_k(p) < m, else m.  Exact; the order
 *             decides only the sign of a zero.
 *   mode 1    the mean: s = (double)frame_0(p); s = s + (double)frame_k(p) in ascending k; d_out(p) = (float)(s / (double)n)
 *   photon_piv_background_path returns 1 when the call with these pointers and this stride reads 16 bytes per lane (both
 *   pointers 16-byte aligned, frame_stride a multiple of 4; the last width height mod 4 pixels one by one), 0 when it reads
 *   pixel by pixel.  Both forms return the same bits.  Host arithmetic, nothing launched.
 *   Refused (1, one stderr line, nothing written, no launch): a null pointer, n_frames < 1, frame_stride < width height,
 *   a mode other than 0 / 1, a side outside [1, 2^22], d_out overlapping the span of the frames
 *   [d_frames, d_frames + (n-1) frame_stride + width height).
 *
 * photon_piv_preprocess: frame k of the result at d_out + k out_stride, for all n_frames in one launch.  Per frame:
 *   d         d = max(im - bg, 0) with the one plane d_background f32[height*width] for all frames; d_background NULL:
 *             d = im, no clamp
 *   radius 0  out = d.  d_out == d_frames with out_stride == frame_stride is allowed: in place.
 *   radius r in [1, 8], with N(p) the (2r+1)^2 pixels around p that lie in the image, rows_in x cols_in of them:
 *             mn(p), mx(p) = the smallest and the largest d over N(p)
 *             lo(p) = (sum of mn over N(p)) / (float)(rows_in cols_in),  hi(p) likewise from mx
 *             the sum:  every row of N(p) from +0 in ascending column (s = s + mn), then those row sums from +0 in
 *             ascending row
 *             out(p) = max(d - lo, 0) / max(hi - lo, floor)
 *             floor > 0 is an absolute intensity: where the local contrast hi - lo is below it, the pixel is divided by
 *             floor instead -- a region without particles keeps its noise small instead of being stretched to full scale.
 * Pixels that are not finite are outside the contract: the results within 2r of one are unspecified, nothing faults.
 * Refused (1, one stderr line, nothing written, no launch): a null d_frames or d_out, n_frames < 1, a stride < width
 * height, a side outside [1, 2^22], radius outside [0, 8], radius > 0 with a floor that is not finite or not > 0, radius 0
 * with a NULL background (nothing to do), d_out overlapping the span of the frames (but for the in-place form above) or
 * the background.
 * Both calls are asynchronous on `stream`, use no device scratch and return the same bits for the same inputs.
 * DESIGN.md section 4.3n. */
int photon_piv_background(const float *d_frames, long long frame_stride, int n_frames, int width, int height, int mode,
                          float *d_out, void *stream);
int photon_piv_background_path(const float *d_frames, long long frame_stride, const float *d_out);
int photon_piv_preprocess(const float *d_frames, long long frame_stride, int n_frames, int width, int height,
                          const float *d_background, int radius, float floor, float *d_out, long long out_stride,
                          void *stream);

/* ------------------------------------------------------------------------------------
 * Section 16: a vector field carried from one window grid to another on the same image -- the step between the levels of
 * multigrid window refinement (64 -> 32 -> 16: large windows find the shift, small ones resolve its gradients).  Host
 * models: photon_amd/piv_multigrid.py (regrid_model: this section operation by operation; regrid_model_f64).
 *   d_src     device f32[src_rows*src_cols][src_stride], dx and dy first (src_stride 2: a field of section 7c; 4: d_vectors
 *             of section 5), on the grid (src_win, src_step) of a width x height image
 *   d_dst     device f32[dst_rows*dst_cols][2] on the grid (dst_win, dst_step) of the same image; NULL: the size query --
 *             *dst_rows, *dst_cols (either may be NULL) are written and nothing is launched
 * d_dst(k) = section 7b's D -- bilinear in the window-centre coordinates of the source grid, constant beyond its outermost
 * centres, a source vector that is not finite read as (0, 0) -- at the centre of destination window k.  Per axis, with n
 * source nodes, from exact integers (twice the distance from the first source centre; the half-pixel centres cancel):
 *   num = (dst_win - src_win) + 2 k dst_step,  den = 2 src_step,  inv_den = 1.f / (float)den
 *   num <= 0 or n = 1:  node 0, w = 0;   num >= (n - 1) den:  node n - 1, w = 0;
 *   else  i0 = floor(num / den), i1 = i0 + 1, w = (float)(num - i0 den) inv_den   (i0 from (float)num inv_den, corrected by
 *         the exact remainder: num < 2^24)
 * and, every operation one IEEE f32 operation, nothing fused, for dx and dy alike:
 *   t = a + wx (b - a),  u = c + wx (e - c),  d_dst = t + wy (u - t)      a, b = nodes (i0, j0), (i0, j1); c, e = (i1, j0), (i1, j1)
 * This is the code photon_piv_deform and photon_piv_field_to_pixels run per pixel (there num = 2 p - (win - 1)), entered
 * with a window centre.  The same grid returns the field (a non-finite vector as zeros); a constant field stays constant
 * bit for bit.
 * Refused (1, one stderr line, nothing written, no launch): a (win, step) that section 5 refuses for the image, src_rows x
 * src_cols that is not the source grid, src_stride other than 2 or 4, a side above 2^22, a null d_src, d_dst == d_src.
 * Asynchronous on `stream`, no device scratch; two calls on the same inputs return the same bits.
 *
 * Driver (PhotonLibrary.correlate_multigrid; piv_multigrid.correlate_multigrid_model): level 0 is correlate_deform at
 * schedule[0]; every further level regrids the last (smoothed) field onto its grid as the predictor and runs its
 * iterations of section 7 there.  DESIGN.md section 4.3o. */
int photon_piv_regrid(const float *d_src, int src_stride, int src_rows, int src_cols, int src_win, int src_step, int width,
                      int height, int dst_win, int dst_step, float *d_dst, int *dst_rows, int *dst_cols, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 17: section 5 with excluded pixels -- a model, a wall, a nozzle lip, the region outside the laser sheet or the
 * dot pattern.  Host model: photon_amd/piv_mask.py (correlate_masked_model, f64).  Everything section 5 says about the
 * grid, the offsets, the peak, the subpixel fit, the ratio, bits 1 / 2 / 4, the size query and asynchrony holds here.
 *   d_mask1, d_mask2  device u8[height*width] in image coordinates, nonzero = the pixel is excluded; either may be NULL
 *             (nothing excluded), and they may be one pointer
 *   min_valid in [1, win^2]: the fewest valid pixels a window may keep
 * A pixel of a is valid when mask1 is 0 there; a pixel of b when it lies in the image and mask2 is 0 at its own position
 * (offset and shift applied).  n_a = the valid pixels of a, n_b = the valid pixels of b in the zero-shift window.
 *   mean a over the valid pixels of a, mean b over the valid pixels of the zero-shift window; an invalid pixel of either
 *   contributes 0 after the mean is subtracted (section 5's rule for pixels outside the image, extended); the energies run
 *   over valid pixels; the flat rule (bit 2) reads the extremes of the valid pixels.  The value of an invalid pixel is
 *   never used in arithmetic: NaN or inf under a mask changes no output bit.
 *   d_valid   device int[n][2] = (n_a, n_b), or NULL
 *   d_flags   section 5's bits, and
 *             16 masked out: n_a < min_valid or n_b < min_valid.  Vector and plane NaN as for a flat window; bit 4 is still
 *                reported, bit 2 is not set.
 *             32 partially masked: not masked out, and a pixel with a nonzero mask lies in a's window (mask1) or in the
 *                in-image part of b's search region (mask2).
 * A window without bit 16 or 32 returns section 5's bits exactly (vectors, flags, planes): with NULL masks, with all-zero
 * masks, with masks that are nonzero only where the window does not look.  A window with bit 32 normalises by the overlap:
 *   N(s)  = the number of p with a(p) valid and b(p + s) valid (the correlation of the two 0/1 validity planes)
 *   C'(s) = (float)((double)C(s) (double)n_a / (double)N(s)) where 2 N(s) >= n_a, else 0 (shifts that keep few pairs are
 *           not amplified into peaks; N = 0 included)
 * and peak, ratio, fit and d_planes are read from C', with section 5's 1 / sqrt(energy a energy b).
 * Refused as in section 5, and: min_valid outside [1, win^2], d_valid without d_vectors.  Two calls on the same inputs
 * return the same bits.  DESIGN.md section 4.3p. */
int photon_piv_correlate_masked(const float *d_im1, const float *d_im2, const unsigned char *d_mask1, const unsigned char *d_mask2,
                                int width, int height, int win, int step, int radius, int min_valid, const int *d_offset,
                                float *d_vectors, int *d_flags, int *d_valid, float *d_planes, int *n_rows, int *n_cols, void *stream);

/* ------------------------------------------------------------------------------------
 * Section 18: section 5 with a weight per window pixel -- a Gaussian window in place of the top hat, whose frequency
 * response sinc(win / lambda) is negative for displacement wavelengths below the window size.  Host model:
 * photon_amd/piv_weighting.py (correlate_weighted_model, f64).  Everything section 5 says about the grid, the offsets, the
 * peak, the subpixel fit, the ratio, bits 1 and 4, the outputs and their layouts, the size query and asynchrony holds here.
 *   d_weight  device f32[win*win], row-major in window coordinates: row y, column x of frame 1's window; one table for
 *             all windows.  The kernel reads W = w where w > 0 and 0 otherwise: negative and NaN entries count as 0.
 *             +inf is outside the contract (the sums become inf or NaN and the window comes back flat or NaN).
 * The weight rides on frame 1's window.  With a, b, o and s as in section 5 and every sum over the win^2 pixels p:
 *   mean a = sum W a / sum W;  mean b = sum W b / sum W over the in-image pixels of the zero-shift window (0 where their
 *   weights sum to 0); pixels of im2 outside the image read as mean b (contribute 0)
 *   C(s)  = sum_p W(p) (a(p) - mean a)(b(p + s) - mean b)
 *   Cn    = C / sqrt(ea eb),  ea = sum W (a - mean a)^2,  eb = sum W (b - mean b)^2 at zero shift
 * Flat (bit 2, every output of the window NaN): sum W = 0; all pixels of a with W > 0 equal; the in-image pixels of b at
 * zero shift with W > 0 all equal, or none; an f32 energy not above 0.  As in section 5 this is decided from the pixels,
 * not from the means: (w a) / w need not return a.  A pixel under a weight of 0 is still multiplied by it: the images
 * are finite, as section 5 expects them.
 * With every weight 1.0f the call returns section 5's vectors, flags and planes bit for bit (fmaf(1, v, s) is s + v, 1 d
 * is d, sum W is win^2 exactly, and the staging pass keeps section 5's lane order).  A table scaled by a power of two
 * returns the same planes, peaks and ratios bit for bit.
 * Section 13's window_sigma multiplies both frames by a Gaussian; the product weight on a pair of pixels is then a
 * Gaussian of window_sigma / sqrt(2): the table that weights a pair alike here has sigma = window_sigma / sqrt(2).
 * Refused (1, one stderr line, nothing written, no launch): section 5's list, and a null d_weight.  f32 sums in a fixed
 * order: two calls on the same inputs return the same bits.  DESIGN.md section 4.3q.
 *
 * photon_piv_window_weights fills a host table f32[win*win] for it (needs no GPU): kind 0 uniform (1.0f; param unused),
 * kind 1 Gaussian, exp(-(cy^2 + cx^2) / (2 sigma^2)) with c = index - (win - 1) / 2 and sigma = param pixels, evaluated in
 * f64 and rounded once.  Refused (1, one stderr line, nothing written): win not 16 / 32 / 64, another kind, a sigma that is
 * not finite and > 0, a null pointer. */
int photon_piv_correlate_weighted(const float *d_im1, const float *d_im2, const float *d_weight, int width, int height, int win,
                                  int step, int radius, const int *d_offset, float *d_vectors, int *d_flags, float *d_planes,
                                  int *n_rows, int *n_cols, void *stream);
int photon_piv_window_weights(int win, int kind, float param, float *weights);

/* ------------------------------------------------------------------------------------
 * Section 19: stereo PIV -- the frames of two cameras that look at one light sheet from two sides, resampled onto one grid
 * on the sheet's plane (dewarp), correlated there by any correlator of this header, and the two 2-C fields combined into
 * three components per node (reconstruct); and the disparity between the two dewarped views of one instant triangulated
 * into points of the sheet (triangulate), from which the host corrects the cameras for a sheet that is not at the plane.
 * Host models, the camera fit, the sheet fit and the test generators: photon_amd/piv_stereo.py.
 * Every entry point takes one pointer to a job struct (host memory, read during the call, not kept); the last member is the
 * stream.  None allocates device memory.
 *
 * Camera (photon_piv_camera_t): Soloff's polynomial from world (X, Y, Z) to image (x, y) in pixels, x = column, y = row.
 * With q = ((X, Y, Z) - centre) / scale per component, and the 19 terms T_k(q), cubic in X and Y, quadratic in Z, in this order:
 *   1, X, Y, Z, X^2, XY, Y^2, XZ, YZ, Z^2, X^3, X^2 Y, X Y^2, Y^3, X^2 Z, XYZ, Y^2 Z, X Z^2, Y Z^2
 * (products from the left: X^2 Y = (X X) Y, XYZ = (X Y) Z, X Z^2 = X (Z Z)),  x = sum_k cx[k] T_k, y = sum_k cy[k] T_k.
 * Plane (photon_piv_plane_t): dewarped pixel (row i, column j) is the world point (x0 + j pitch, y0 + i pitch, z), i in
 * [0, height), j in [0, width); pitch > 0 in world units per dewarped pixel.
 *
 * a. photon_piv_dewarp.  Frame f of the source is d_coef + f frame_stride: the cubic B-spline coefficients (section 7a,
 *    unchanged) of a camera frame, f32[height*width]; frame f of the result is d_out + f out_stride, f32[out_height*out_width]
 *    (section 14's stride addressing, in floats, on both sides: the two exposures of a camera, or a series, in one launch).
 *    The camera arrives folded at the plane (piv_stereo.plane_coefficients): with w = (z - centre_z) / scale_z the 10
 *    coefficients per image coordinate of the bivariate cubic in (u, v) = (q_X, q_Y), in the order 1, u, v, u^2, uv, v^2, u^3,
 *    u^2 v, u v^2, v^3:
 *      k0 = (c9 w + c3) w + c0,  k1 = (c17 w + c7) w + c1,  k2 = (c18 w + c8) w + c2,  k3 = c14 w + c4,  k4 = c15 w + c5,
 *      k5 = c16 w + c6,  k6 = c10,  k7 = c11,  k8 = c12,  k9 = c13       (f64; poly[0] from cx, poly[1] from cy)
 *    and grid[4] = (u0, du, v0, dv) = ((x0 - centre_X) / scale_X, pitch / scale_X, (y0 - centre_Y) / scale_Y, pitch / scale_Y):
 *    the kernel divides nothing.  Per output pixel (i, j), one thread, in f64, no fused multiply-add:
 *      u = u0 + (double)j du,  v = v0 + (double)i dv
 *      a0 = ((k9 v + k5) v + k2) v + k0,  a1 = (k8 v + k4) v + k1,  a2 = k7 v + k3,  p = ((k6 u + a2) u + a1) u + a0
 *    for x (poly[0]) and y (poly[1]).  The pixel is inside when 0 <= x <= width - 1 and 0 <= y <= height - 1 (a NaN is
 *    not).  Inside: fx = floor(x), fy = floor(y), tx = (float)(x - fx), ty = (float)(y - fy) -- the absolute coordinate never
 *    enters f32 --, the 4 x 4 taps fx - 1 .. fx + 2, fy - 1 .. fy + 2 under section 7's whole-sample mirror, section 7b's
 *    f32 B-spline weights of tx and ty and section 7b's order of the sums: per row ((w0 c0 + w1 c1) + w2 c2) + w3 c3, the
 *    rows accumulated from 0 in the order of fy - 1 .. fy + 2.  Coordinate, weights and the 8 mirrored indices are computed
 *    once and serve all n_frames frames.  Outside: 0.0f in every frame.  d_mask (device u8[out_height*out_width], or
 *    NULL): 1 outside, 0 inside -- one mask for all frames, it depends on the geometry alone; it is what section 17 takes
 *    as d_mask1 / d_mask2.  Every pixel of the n_frames output frames and of the mask is written, nothing else (the gaps
 *    of a stride above out_width out_height are not touched).  With the identity map (x = j, y = i) the result is
 *    photon_piv_deform's at zero shift bit for bit.  Host model of exactly these f32 / f64 operations:
 *    piv_stereo.dewarp_model_f32 (equal bit for bit); in f64 throughout: piv_stereo.dewarp_model.
 *    Refused (1, one stderr line, nothing written, no launch): a null job, d_coef or d_out; d_out == d_coef; a size below 1
 *    or a side above 2^22 pixels, source or result; n_frames < 1; frame_stride < width height; out_stride < out_width
 *    out_height; a poly or grid value that is not finite.  Asynchronous on `stream`; two calls return the same bits.
 *
 * b. photon_piv_stereo_reconstruct.  d_field1, d_field2: the two cameras' displacement fields on section 5's grid (win,
 *    step) of the dewarped plane->width x plane->height image, device f32[n][field_stride] with dx, dy first (field_stride
 *    2: a field of section 7c; 4: section 5's d_vectors), in dewarped pixels; d_flags1, d_flags2: their int[n] flags, or
 *    NULL (read as 0); d_sigma1, d_sigma2: f32[n][2] = (sigma_x, sigma_y) of section 11 in dewarped pixels, both or neither.
 *    Per node k = i n_cols + j, one thread, in f64 without fused multiply-add, with the window centre
 *      P = (x0 + (j step + (win - 1) / 2.0) pitch,  y0 + (i step + (win - 1) / 2.0) pitch,  z):
 *      1. per camera c the 2 x 3 Jacobian J_c = d(x, y) / d(X, Y, Z) at P: with q as above and the derivatives D_k of the 19
 *         terms with respect to q_X, q_Y, q_Z (zeros included; 2 X Y = (2 X) Y, 3 X^2 = 3 (X X), 2 X Z = (2 X) Z, the rest as
 *         the terms), each entry = (sum over k = 0 .. 18 from 0.0 of c[k] D_k) / scale of its world axis.
 *      2. a_c = pitch (dx_c, dy_c): the apparent in-plane world displacement camera c saw.  Rows 2c, 2c + 1 of A are J_c,
 *         of b are J_c[:, 0] a_c[0] + J_c[:, 1] a_c[1]: four equations in image pixels for Delta = (dX, dY, dZ).
 *      3. N = A^T A (each entry summed over the rows 0 .. 3 from the first product), r = A^T b likewise; Cholesky N = L L^T:
 *         d0 = N00, L10 = N10 / L00, L20 = N20 / L00, d1 = N11 - L10 L10, L21 = (N21 - L20 L10) / L11, d2 = (N22 - L20 L20) -
 *         L21 L21, L_kk = sqrt(d_k).  Pivot ratio = min d_k / max d_k.  Not (ratio > 1e-12) (a pivot <= 0 or NaN included):
 *         degenerate, flag 64, all eight outputs NaN.
 *      4. forward and back substitution for Delta; residual = sqrt(sum over the four rows of ((A Delta)_m - b_m)^2), (A
 *         Delta)_m = (A_m0 dX + A_m1 dY) + A_m2 dZ: the stereo residual in image pixels, the figure of registration quality.
 *      5. with sigmas: N^-1 column by column through the same substitutions, M = N^-1 A^T (3 x 4), per camera G_c = M[:,
 *         2c : 2c + 2] J_c[:, 0 : 2] (3 x 2), var_k = sum over c, then m, from 0.0 of (G_c[k][m] G_c[k][m]) (pitch sigma_cm)^2
 *         -- the diagonal of (A^T A)^-1 A^T Sigma_b A (A^T A)^-1 with Sigma_b = J_xy diag(pitch^2 sigma^2) J_xy^T per camera --,
 *         sigma_k = sqrt(var_k).
 *    d_out f64[n][8] = dX, dY, dZ in world units, the residual, sigma_X, sigma_Y, sigma_Z (NaN without sigmas), the pivot
 *    ratio.  d_flags int[n] = flags1 | flags2, plus 64 (degenerate geometry) and 128 (a dx or dy of either camera is not
 *    finite: the first seven outputs NaN, the ratio reported).  Host model: piv_stereo.reconstruct_model (the same
 *    operations; agreement to 1e-12).
 *    This is a first-order reconstruction: the Jacobian is taken at the plane, at the window centre, not at the
 *    half-displaced particle positions, so a displacement sees the camera's curvature (perspective) only to first order.
 *    The reconstruction itself applies no disparity correction: a sheet that is not at plane.z is found from the disparity
 *    of the two views (c, below) and repaired in the cameras before this call (PhotonLibrary.self_calibrate_stereo).
 *    d_out == NULL: the size query -- *rows_out, *cols_out (where given) receive section 5's grid of the plane, nothing is
 *    launched, n_rows and n_cols are not read.  Refused (1, one stderr line, nothing written, no launch): a null job;
 *    section 5's rules for win, step and the plane's size; with d_out: n_rows x n_cols that is not that grid, a null
 *    d_field1, d_field2 or d_flags, field_stride not 2 or 4, one sigma without the other; a plane or camera value that is
 *    not finite, pitch <= 0, a camera scale of 0.  Asynchronous on `stream`; two calls return the same bits.
 *
 * c. photon_piv_stereo_triangulate: the world points of a disparity field (self-calibration after Wieneke 2005).
 *    d_disparity: device f32[n][field_stride] with dx, dy first (field_stride 2 or 4), in dewarped pixels, on section 5's grid
 *    (win, step) of the plane: the displacement from camera 1's dewarped frame to camera 2's dewarped frame of the same
 *    instant -- what photon_piv_correlate_ensemble returns for (dewarped stack of camera 1, dewarped stack of camera 2);
 *    d_flags_in: its int[n] flags, or NULL (read as 0).  A sheet at plane.z has no disparity; particles off the plane are
 *    seen by the two cameras at two points of the plane, half the disparity to either side of the window centre.
 *    Per node k = i n_cols + j, one thread, in f64 without fused multiply-add:
 *      1. P = the window centre on the plane, b's expression.
 *      2. h = (pitch / 2.0) (dx, dy);  P1 = (P_X - h_x, P_Y - h_y, z),  P2 = (P_X + h_x, P_Y + h_y, z).
 *      3. x1 = M1(P1), x2 = M2(P2), M_c the camera: q as above, the 19 terms T_k in the order and with the products above
 *         (X^3 = (X X) X, X Y^2 = (X Y) Y, Y^3 = (Y Y) Y, X^2 Z = (X X) Z, Y^2 Z = (Y Y) Z), each image coordinate summed
 *         over k = 0 .. 18 from 0.0 of c[k] T_k.
 *      4. W = P; `iterations` times (Gauss-Newton):  r = (x1 - M1(W), x2 - M2(W)), four values;  rows 2c, 2c + 1 of A are
 *         the Jacobian J_c of b.1 at W;  N = A^T A and g = A^T r in b.3's order of sums;  b.3's Cholesky and pivot ratio;
 *         not (ratio > 1e-12), a pivot <= 0 or NaN included: degenerate, the iterations end;  s = N^-1 g by b.4's
 *         substitutions;  W = W + s per component.
 *      5. r once more at the final W.
 *    d_out f64[n][6] = W_X, W_Y, W_Z in world units; the triangulation error sqrt(sum from 0.0 of r_m r_m) in image
 *    pixels -- how far the two lines of sight miss each other; the length sqrt((s_X s_X + s_Y s_Y) + s_Z s_Z) of the last
 *    step in world units, which shows convergence without a second call; the smallest pivot ratio of the iterations (of a
 *    degenerate iteration: that iteration's own).  d_flags int[n] = flags_in, plus 64 (an iteration was degenerate: the
 *    first five outputs NaN) and 128 (dx or dy is not finite: the first five outputs NaN, no step taken, the ratio that of
 *    the start point P).  Every node's six outputs and flag are written, nothing else.  Host model:
 *    piv_stereo.triangulate_model (the same operations; agreement to 1e-12).
 *    d_out == NULL: the size query, as b's.  Refused (1, one stderr line, nothing written, no launch): a null job;
 *    section 5's rules for win, step and the plane's size; with d_out: n_rows x n_cols that is not that grid, a null
 *    d_disparity or d_flags, field_stride not 2 or 4; iterations outside [1, 16]; a plane or camera value that is not
 *    finite, pitch <= 0, a camera scale of 0.  Asynchronous on `stream`; allocates nothing; two calls return the same bits.
 *    What the host does with the points -- the sheet Z = a + b X + c Y by least squares, the frame in which the sheet is
 *    plane.z, the cameras refitted in that frame, the rounds -- is piv_stereo.fit_sheet, sheet_frame, move_camera and
 *    self_calibrate_model; the driver is PhotonLibrary.self_calibrate_stereo.  Not done: the sheet's thickness from the
 *    width of the disparity peak; any correction under a dewarp mask beyond leaving those nodes out.
 *
 * Drivers: PhotonLibrary.dewarp, PhotonLibrary.correlate_stereo and PhotonLibrary.self_calibrate_stereo.  DESIGN.md section
 * 4.3w. */
typedef struct photon_piv_camera_t {
    double centre[3], scale[3], cx[19], cy[19];
} photon_piv_camera_t;
typedef struct photon_piv_plane_t {
    double x0, y0, pitch, z;
    int width, height;
} photon_piv_plane_t;
typedef struct photon_piv_dewarp_t {
    const float *d_coef;
    long long frame_stride;
    int n_frames, width, height;
    double poly[2][10], grid[4];
    int out_width, out_height;
    long long out_stride;
    float *d_out;
    unsigned char *d_mask;
    void *stream;
} photon_piv_dewarp_t;
typedef struct photon_piv_stereo_t {
    const float *d_field1, *d_field2;
    int field_stride;
    const int *d_flags1, *d_flags2;
    const float *d_sigma1, *d_sigma2;
    int n_rows, n_cols, win, step;
    photon_piv_plane_t plane;
    photon_piv_camera_t camera1, camera2;
    double *d_out;
    int *d_flags;
    int *rows_out, *cols_out;
    void *stream;
} photon_piv_stereo_t;
typedef struct photon_piv_triangulate_t {
    const float *d_disparity;
    int field_stride;
    const int *d_flags_in;
    int n_rows, n_cols, win, step, iterations;
    photon_piv_plane_t plane;
    photon_piv_camera_t camera1, camera2;
    double *d_out;
    int *d_flags;
    int *rows_out, *cols_out;
    void *stream;
} photon_piv_triangulate_t;
int photon_piv_dewarp(const photon_piv_dewarp_t *job);
int photon_piv_stereo_reconstruct(const photon_piv_stereo_t *job);
int photon_piv_stereo_triangulate(const photon_piv_triangulate_t *job);

/* ------------------------------------------------------------------------------------
 * Section 20: tomographic PIV -- three components in a volume from three or more cameras: the cameras' frames combined by
 * line of sight into a particle volume (volume_los), and two such volumes correlated with three-dimensional windows and a
 * three-dimensional search region (correlate_volume).  Host models and the test generators: photon_amd/piv_tomo.py.
 * Both entry points take one pointer to a job struct (host memory, read during the call, not kept) whose last member is the
 * stream, as section 19's do; both are asynchronous on that stream, allocate no device memory, write every element they own
 * and nothing else, and return the same bits from two calls.
 *
 * Volume (photon_piv_volume_t): voxel (k, i, j) is the world point (x0 + j pitch, y0 + i pitch, z0 + k pitch), k in [0, nz),
 * i in [0, ny), j in [0, nx); of frame f it is stored at d_out + f out_stride + (k ny + i) nx + j, out_stride >= nx ny nz.
 *
 * a. photon_piv_volume_los.  n_cameras in [2, 8] cameras; of camera c: d_coef[c], the section 7a coefficients of its n_frames
 *    frames, frame_stride[c] floats apart, f32[height[c]*width[c]] each (the sensors may differ), and grid[c][4], section 19a's
 *    grid of that camera on the volume's (x0, y0, pitch).  d_poly: device f64[n_cameras][nz][2][10], camera c folded at slice
 *    k's z = z0 + k pitch by section 19a's formulas (piv_tomo.los_coefficients): the host computes it, the kernel divides
 *    nothing; it is on the device and is not inspected.  Per voxel (k, i, j), one thread: let s_c be the value photon_piv_dewarp
 *    gives at pixel (i, j) with poly = d_poly[c][k], grid[c] and the output size nx x ny -- the same f64 Horner, the same
 *    inside test, the same f32 weights and the same order of sums.  If any camera is outside, the voxel is 0.0f in every
 *    frame and the mask is 1.  Otherwise, with v_c = s_c > 0 ? s_c : 0:  mode 0 (MinLOS): the minimum over c, in camera
 *    order;  mode 1 (multiplicative LOS): the product ((v_0 v_1) v_2) ..., in f32, nothing fused.  The N-th root of the
 *    product is deliberately absent: photon_det_math.h has no bit-reproducible log or pow; the root belongs with the
 *    intensity normalisation of an iterative reconstruction.  Coordinate, weights and mirrored indices are computed once per
 *    camera and voxel and serve the frames four at a time: a pair of exposures costs one coordinate evaluation (a longer
 *    series one per four frames; the bits do not depend on it).  d_mask: device u8[nz ny nx], or NULL: 1 where a camera
 *    does not see the voxel.  The gaps of an out_stride above nx ny nz are not touched.  Host model of exactly these
 *    operations: piv_tomo.los_model_f32 (equal bit for bit); in f64: piv_tomo.los_model.
 *    Refused (1, one stderr line, nothing written, no launch): a null job, d_poly, d_out or d_coef[c]; n_cameras outside [2,
 *    8]; a mode that is not 0 or 1; n_frames < 1; a size below 1 or a side above 2^22, sensor or volume; nx ny nz above
 *    INT_MAX; a frame_stride[c] below width[c] height[c]; out_stride below nx ny nz; d_out's frames overlapping a camera's; a
 *    grid value that is not finite.
 *
 * b. photon_piv_correlate_volume.  d_vol1, d_vol2: device f32[nz][ny][nx], contiguous.  In the plane win, step and radius are
 *    section 5's, under section 5's rules; along z win_z in [1, 64] (<= nz), step_z >= 1, radius_z in [0, min(16, win_z / 2)].
 *    Grid: n_slabs = (nz - win_z) / step_z + 1, n_rows and n_cols as in section 5; node w = (l n_rows + i) n_cols + j has its
 *    centre where section 5 has it in the plane and at l step_z + (win_z - 1) / 2 in z.  d_offset: device int[n][3] = (ox, oy,
 *    oz) per node, or NULL; in a volume of one slice oz is not read and counts as 0.  With R = radius, Rz = radius_z and the
 *    shifts s = (sz, sy, sx) in [-Rz, Rz] x [-R, R]^2, section 5's definition with one more axis:
 *      C(s) = sum_p (a(p) - mean a)(b(p + o + s) - mean b) over the win_z win^2 voxels p of the window;  mean a over the
 *      window;  mean b over the in-volume voxels of the offset window at zero shift (0 where there are none);  voxels of vol2
 *      outside the volume read as mean b (contribute 0);  Cn = C / sqrt(ea eb),  ea = sum (a - mean a)^2,  eb = sum (b - mean
 *      b)^2 at zero shift.
 *    Flat (flag 2, every output of the window NaN): all voxels of a equal; the in-volume voxels of b at zero shift all
 *    equal, or none; an f32 energy not above 0 -- decided from the voxels, as in section 5.  Flag 4: a voxel of vol2 the
 *    window needs (offset, any shift) lies outside the volume.  Flag 1: the integer peak lies on the edge of the search
 *    region in a searched axis; z is searched when radius_z >= 1: with radius_z = 0, dz = oz and z raises no flag.
 *    The peak is the argmax, ties to the first shift in (sz, sy, sx) order; per axis section 5's three-point fit in f64 through
 *    the peak's two neighbours along that axis; the ratio is taken against the largest value at Chebyshev distance >= 2 of
 *    the peak (the largest of the three axes' distances), +inf where that is not positive.
 *    d_vectors f32[n][5] = dx, dy, dz, peak, ratio;  d_flags int[n];  d_planes f32[n][(2Rz+1)(2R+1)^2], in (sz, sy, sx)
 *    order: required together with d_vectors and d_flags -- it is the kernel's workspace for the raw planes, so that the
 *    call needs no second buffer and allocates nothing, and holds Cn on return.  d_vectors == NULL: the size query into
 *    *n_slabs, *n_rows, *n_cols (where given), nothing launched.
 *    One workgroup per window under section 5's plan; the means and the exact flatness counts from a first pass over the
 *    window's planes; then per z-shift (the zero shift first) the win_z plane pairs (pz, pz + oz + sz), each staged as section
 *    5 stages a pair (a plane of vol2 outside [0, nz) is all zeros) and added into the running plane as section 14 adds a
 *    pair; the energies summed in plane order; f32 sums in a fixed order.  A volume of one slice with win_z = 1, step_z =
 *    1, radius_z = 0 returns photon_piv_correlate's dx, dy, peak, ratio, flags and plane bit for bit.
 *    Host model: piv_tomo.correlate_volume_model (f64, planes included).
 *    Refused (1, one stderr line, nothing written, no launch): a null job; section 5's rules for win, radius, step and the
 *    slice's size; a side above 2^22 or nx ny nz above INT_MAX; win_z, step_z or radius_z outside the ranges above; nz <
 *    win_z; a null volume; d_vectors without d_flags or d_planes; more than INT_MAX windows; a (win, radius) whose LDS the
 *    device does not have.
 *
 * Drivers: PhotonLibrary.reconstruct_volume and PhotonLibrary.correlate_tomo.  Iterative reconstruction (MART) from the
 * line-of-sight volume: section 21.  Not here: SMART and MLEM, 3-D validation and multi-pass refinement, volumetric
 * self-calibration.  DESIGN.md section 4.3x. */
typedef struct photon_piv_volume_t {
    double x0, y0, z0, pitch;
    int nx, ny, nz;
} photon_piv_volume_t;
typedef struct photon_piv_volume_los_t {
    int n_cameras, n_frames, mode;
    const float *d_coef[8];
    long long frame_stride[8];
    int width[8], height[8];
    double grid[8][4];
    const double *d_poly;
    photon_piv_volume_t volume;
    long long out_stride;
    float *d_out;
    unsigned char *d_mask;
    void *stream;
} photon_piv_volume_los_t;
typedef struct photon_piv_correlate_volume_t {
    const float *d_vol1, *d_vol2;
    int nx, ny, nz;
    int win, step, radius, win_z, step_z, radius_z;
    const int *d_offset;
    float *d_vectors;
    int *d_flags;
    float *d_planes;
    int *n_slabs, *n_rows, *n_cols;
    void *stream;
} photon_piv_correlate_volume_t;
int photon_piv_volume_los(const photon_piv_volume_los_t *job);
int photon_piv_correlate_volume(const photon_piv_correlate_volume_t *job);

/* ------------------------------------------------------------------------------------
 * Section 21: MART particle volumes for tomographic PIV -- the exact re-projection of a volume onto its cameras
 * (volume_project) and the multiplicative, camera-sequential update that starts from section 20a's line-of-sight volume
 * (volume_mart: MLOS-MART).  Host models: photon_amd/piv_mart.py.  Both entry points take one job struct whose last member
 * is the stream, as section 20's do; both are asynchronous on that stream, allocate no device memory and return the same
 * bits from two calls.  Cameras (n_cameras in [2, 8], width[c], height[c], grid[c], d_poly) and the volume are section 20a's.
 *
 * Footprint.  Voxel (k, i, j) lands on camera c at (x, y) by section 20a's pipeline: d_poly[c][k], grid[c], the same f64 Horner,
 * the same inside test (a NaN is outside: the camera does not see the voxel).  x0 = floor(x), fx = (float)(x - x0); the x
 * taps are x0 and min(x0 + 1, width - 1) with the weights 1.0f - fx and fx; the same in y.  The four tap weights are w = wy wx
 * in f32, nothing fused, in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1): a bilinear footprint.  The projection scatters
 * with these weights and the update gathers with them: a matched pair.
 *
 * a. photon_piv_volume_project.  d_vol: device f32, n_frames volumes [nz][ny][nx], vol_stride floats apart (read only).
 *    d_acc[c]: device int64, n_frames accumulators [height[c] width[c]], acc_stride[c] apart.  With s = scale_log2:
 *      every accumulator starts at 0 (zeroed by the call on its stream);  every voxel with E > 0 that camera c sees adds,
 *      to each of its four taps,  q = llrint(min((double)(w E) 2^s, 2^31)),  the product w E taken in f32; a product that is
 *      not above 0 adds 0 (w = 0, and the NaN of an infinite E under a zero weight).  Voxels with !(E > 0) -- zeros,
 *      negatives, NaN -- add nothing.
 *    This is the definition; the order of the additions is free: integer addition is associative, so atomics in any
 *    order return these integers, and so does piv_mart.project_model (np.add.at on int64).  Bound: two taps of one voxel
 *    share a pixel only where a tap is clamped at the sensor's edge, and the clamped tap's weight is 0; so a voxel adds at
 *    most 2^31 to a pixel, and with nx ny nz <= INT_MAX every sum stays below 2^62 for any input.
 *    d_image[c]: device f32, n_frames images acc_stride[c] floats apart, or NULL:  image = (float)((double)acc 2^-s).
 *    One launch reads every voxel once and scatters it to all cameras; the gaps of a longer acc_stride are not touched.
 *    Refused (1, one stderr line, nothing written, no launch): a null job, d_poly, d_vol or d_acc[c]; n_cameras outside [2,
 *    8]; n_frames < 1; scale_log2 outside [-126, 62]; a size below 1 or a side above 2^22, sensor or volume; nx ny nz above
 *    INT_MAX; vol_stride below nx ny nz; an acc_stride[c] below width[c] height[c]; a grid value that is not finite;
 *    accumulators or images that overlap each other or the volume.
 *
 * b. photon_piv_volume_mart.  d_frame[c]: device f32, the n_frames raw frames of camera c themselves (not section 7a's
 *    coefficients), frame_stride[c] floats apart.  d_vol: device f32, n_frames volumes vol_stride apart, the first guess on
 *    entry, updated in place.  d_mask: device u8[nz ny nx] as section 20a writes it, or NULL: 1 marks a voxel that stays 0.
 *    iterations >= 1; mu_roots in [0, 3]: the relaxation mu = 2^-mu_roots; threshold >= 0, finite.  d_acc: the caller's
 *    workspace, device int64[2][n_frames][max_c height[c] width[c]]: its content on entry does not matter.
 *    For it = 0 .. iterations - 1, for c = 0 .. n_cameras - 1, in this order, per frame:
 *      1. P_c = 21a's accumulators of the current volume for camera c alone;  P_t = (float)((double)acc_t 2^-s) at pixel t.
 *      2. For every voxel with E > 0:  E = 0.0f if camera c does not see the voxel or the mask is 1.  Otherwise, at the
 *         voxel's four taps,  I_bar = ((w0 I0+ + w1 I1+) + w2 I2+) + w3 I3+  with I+ = I > 0 ? I : 0 of the frame, and
 *         P_bar the same expression on P; everything in f32, nothing fused.  If P_bar > 0:  r = I_bar / P_bar, mu_roots
 *         times r = sqrtf(r), E = E r (division and roots correctly rounded).  Then E < threshold gives 0.0f.
 *      3. Voxels with !(E > 0) are not read further and not written: zeros stay zero, before any coordinate is computed.
 *    The ratio is raised to mu alone -- the interpolation weight sits in the footprint, not in the exponent -- so the power
 *    is 0 to 3 square roots and photon_det_math.h needs no log or pow.  One thread per voxel in section 20a's launch shape;
 *    a footprint serves the frames four at a time.  Camera c's update and camera c + 1's projection (camera 0's of the next
 *    iteration behind the last camera) are one launch: a voxel's new value is final when the voxel scatters it, and the
 *    integer sums do not depend on the order; the two halves of d_acc alternate, the half written next is zeroed on the
 *    stream.  One projection launch first; iterations x n_cameras launches in all behind it.  Host models:
 *    piv_mart.mart_model_f32 (equal bit for bit) and piv_mart.mart_model (f64, unquantised).
 *    Refused (1, one stderr line, nothing written, no launch): a null job, d_poly, d_vol, d_acc or d_frame[c]; 21a's rules
 *    for the cameras, the frames' count, scale_log2, the sizes, vol_stride and the grids; a frame_stride[c] below width[c]
 *    height[c]; iterations < 1; mu_roots outside [0, 3]; a threshold that is negative or not finite; d_vol, d_acc and d_mask
 *    overlapping one another, or d_vol or d_acc overlapping a camera's frames.
 *
 * Drivers: PhotonLibrary.reproject, reconstruct_volume(method="mart") and correlate_tomo(reconstruction="mart").  Not here:
 * SMART and MLEM, 3-D validation and multi-pass refinement, volumetric self-calibration (re-projection is the operator it
 * will need), masks and weights in 3-D.  DESIGN.md section 4.3y. */
typedef struct photon_piv_volume_project_t {
    int n_cameras, n_frames, scale_log2;
    int width[8], height[8];
    double grid[8][4];
    const double *d_poly;
    photon_piv_volume_t volume;
    const float *d_vol;
    long long vol_stride;
    long long *d_acc[8];
    long long acc_stride[8];
    float *d_image[8];
    void *stream;
} photon_piv_volume_project_t;
typedef struct photon_piv_volume_mart_t {
    int n_cameras, n_frames, iterations, mu_roots, scale_log2;
    float threshold;
    const float *d_frame[8];
    long long frame_stride[8];
    int width[8], height[8];
    double grid[8][4];
    const double *d_poly;
    photon_piv_volume_t volume;
    long long vol_stride;
    float *d_vol;
    const unsigned char *d_mask;
    long long *d_acc;
    void *stream;
} photon_piv_volume_mart_t;
int photon_piv_volume_project(const photon_piv_volume_project_t *job);
int photon_piv_volume_mart(const photon_piv_volume_mart_t *job);

#ifdef __cplusplus
}
#endif
#endif /* PHOTON_AMD_PARALLEL_RAY_TRACING_H_ */
