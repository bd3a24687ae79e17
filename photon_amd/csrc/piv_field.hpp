// piv_field.hpp - the PIV particle field of photon_sources_piv (run_simulation_02.py:774-996), shared by the generator that
// draws it (photon_scene.hip, sources_piv_kernel) and the one that advects it through a velocity field (photon_flow.hip):
// both draw particle i with piv_draw and store it with piv_store, so an advection by zero time is the frame itself by
// construction.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/photon_det_math.h"
#include "../../include/photon_philox.h"

namespace photon {

// X, Y, Z uniform in the box, radiance = the laser sheet's Gaussian profile in Z, Z shifted to the object plane.  The
// reference draws from numpy's unseeded generator; here particle i takes the four words of Philox(seed, i) -- any particle
// can be regenerated.
struct PivFieldDev {
    double lo[3], hi[3];
    double z_object, coef, two_sigma2;      // coef = irradiance_constant / (sigma sqrt(2 pi))
    int n_diameters;                        // 0: diameter_index = 1 (run_simulation_02.py:992)
};

inline PivFieldDev piv_field_setup(const double box_min[3], const double box_max[3], double z_object, double beam_fwhm,
                                   double irradiance_constant, int n_diameters) {
    PivFieldDev f;
    for (int a = 0; a < 3; a++) { f.lo[a] = box_min[a]; f.hi[a] = box_max[a]; }
    const double sigma = beam_fwhm / (2.0 * sqrt(2.0 * log(2.0)));     // run_simulation_02.py:961
    f.z_object = z_object;
    f.coef = irradiance_constant * (1.0 / (sigma * sqrt(2.0 * PHOTON_PI)));
    f.two_sigma2 = 2.0 * (sigma * sigma);
    f.n_diameters = n_diameters;
    return f;
}

// particle i's start (X, Y, Z) in the world frame and the diameter draw ud, from the four words of Philox(seed, i)
__device__ inline void piv_draw(unsigned long long seed, long long i, const PivFieldDev &f, double &X, double &Y, double &Z,
                                double &ud) {
    const photon_u32x4 r = photon_philox4x32_10(seed, (unsigned long long)i, 0u, PHOTON_STREAM_SCENE);
    const double ux = ((double)r.x + 0.5) * (1.0 / 4294967296.0), uy = ((double)r.y + 0.5) * (1.0 / 4294967296.0);
    const double uz = ((double)r.z + 0.5) * (1.0 / 4294967296.0);
    ud = ((double)r.w + 0.5) * (1.0 / 4294967296.0);
    X = (f.hi[0] - f.lo[0]) * ux + f.lo[0];
    Y = (f.hi[1] - f.lo[1]) * uy + f.lo[1];
    Z = (f.hi[2] - f.lo[2]) * uz + f.lo[2];
}

// source i of the field at world (X, Y, Z): f32 coordinates, z shifted to the object plane, the sheet's profile at Z
__device__ inline void piv_store(long long i, const PivFieldDev &f, double X, double Y, double Z, double ud,
                                 const double *diameter_cdf, float *sx, float *sy, float *sz, double *srad,
                                 int *sdia) {
    sx[i] = (float)X;
    sy[i] = (float)Y;
    sz[i] = (float)(Z + f.z_object);
    srad[i] = f.coef * photon_det_exp(-1.0 * (Z * Z / f.two_sigma2));
    int dia = 1;
    if (f.n_diameters > 0) {
        dia = f.n_diameters - 1;
        for (int d = 0; d < f.n_diameters; d++)
            if (ud < diameter_cdf[d]) { dia = d; break; }
    }
    sdia[i] = dia;
}

}  // namespace photon
