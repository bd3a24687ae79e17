"""PIV frame pairs with known displacements (pure numpy: usable without a GPU).

The library draws a PIV particle field in HBM (``PhotonLibrary.sources_piv``, photon_sources_piv: particle i from
Philox4x32-10(seed, i)) and advects it through a steady velocity field on a grid
(``PhotonLibrary.flow_from_grid`` / ``sources_piv_advected``, photon_sources_piv_advected): frame 2 of a PIV pair is
the particles of frame 1 moved by a known flow.  This module holds

* the host models of both generators -- ``philox4x32_10``, ``piv_field`` and ``advect`` -- in the device's operation
  order (include/parallel_ray_tracing.h): x, y, z, the diameter index and the world positions equal the device's bit
  for bit; the radiance uses numpy's exp where the device uses photon_det_exp, so it may differ by RADIANCE_ULP ulp;
* grid fillers for the velocity field -- ``uniform_flow``, ``solid_body_rotation``, ``lamb_oseen_vortex`` -- each
  returning ``(u, v, w, spacing, origin)``, what ``flow_from_grid`` and ``advect`` take;
* ``image_displacements``: the per-particle image shift of a pair from the sensor moments of its two traces
  (``Scene.trace_moments``, ``PhotonLibrary.render_moments``).
"""
from __future__ import annotations

import math

import numpy as np

from . import deflections

PHOTON_STREAM_SCENE = 3             # include/photon_philox.h
RADIANCE_ULP = 4                    # |photon_det_exp - numpy exp| <= 2 ulp each side of exp, plus the product's rounding

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed: int, counter, draw: int = 0, stream: int = PHOTON_STREAM_SCENE):
    """Philox4x32-10 of include/photon_philox.h, vectorised over `counter` (the 64-bit ray / particle id): returns the four
    32-bit output words as uint64 arrays (x, y, z, w)."""
    ctr = np.asarray(counter, dtype=np.uint64)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2 = np.full_like(ctr, np.uint64(int(draw) & 0xFFFFFFFF))
    c3 = np.full_like(ctr, np.uint64(int(stream) & 0xFFFFFFFF))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # < 2^64: exact in uint64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _unit(word):
    return (word.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _sheet(beam_fwhm: float, irradiance_constant: float):
    sigma = float(beam_fwhm) / (2.0 * math.sqrt(2.0 * math.log(2.0)))           # run_simulation_02.py:961
    return float(irradiance_constant) * (1.0 / (sigma * math.sqrt(2.0 * math.pi))), 2.0 * (sigma * sigma)


def _draw(seed, n, box_min, box_max):
    """(X, Y, Z, ud) of particles 0 .. n-1, as piv_draw (photon_amd/csrc/piv_field.hpp)."""
    r = philox4x32_10(seed, np.arange(int(n), dtype=np.uint64))
    lo = [float(v) for v in box_min]
    hi = [float(v) for v in box_max]
    X, Y, Z = ((hi[a] - lo[a]) * _unit(r[a]) + lo[a] for a in range(3))
    return X, Y, Z, _unit(r[3])


def _store(X, Y, Z, ud, z_object, beam_fwhm, irradiance_constant, diameter_cdf) -> dict:
    """What piv_store writes for particles at world (X, Y, Z), plus those positions ("world", f64 [n][3])."""
    coef, two_sigma2 = _sheet(beam_fwhm, irradiance_constant)
    if diameter_cdf is None or len(diameter_cdf) == 0:
        dia = np.ones(X.shape, np.int32)                                        # run_simulation_02.py:992
    else:
        cdf = np.asarray(diameter_cdf, np.float64)
        dia = np.minimum(np.searchsorted(cdf, ud, side="right"), cdf.size - 1).astype(np.int32)   # first d with ud < cdf[d]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        arg = -1.0 * (Z * Z / two_sigma2)
        # photon_det_exp returns 0 below -708 (include/photon_det_math.h), where numpy's exp still has 3e-308 .. 5e-324: a
        # particle more than 37.6 sigma off the sheet
        radiance = coef * np.where(arg < -708.0, 0.0, np.exp(arg))
    return dict(x=X.astype(np.float32), y=Y.astype(np.float32), z=(Z + float(z_object)).astype(np.float32),
                radiance=radiance, diameter_index=dia, world=np.stack([X, Y, Z], 1))


def piv_field(seed: int, n: int, box_min, box_max, z_object: float, beam_fwhm: float, irradiance_constant: float,
              diameter_cdf=None) -> dict:
    """Host model of photon_sources_piv: {"x", "y", "z" f32, "radiance" f64, "diameter_index" i32, "world" f64 [n][3]}."""
    X, Y, Z, ud = _draw(seed, n, box_min, box_max)
    return _store(X, Y, Z, ud, z_object, beam_fwhm, irradiance_constant, diameter_cdf)


# ---- the velocity field: trilinear in f64, clamped to the grid's edge ----------------------------------------------------
def _axis(p, origin: float, spacing: float, n: int):
    f = (p - origin) / spacing
    c = np.floor(f)
    c = np.where(c >= 0.0, c, 0.0)                      # (a NaN goes to cell 0 ...)
    c = np.where(c <= float(n - 2), c, float(n - 2))
    t = f - c
    t = np.where(t > 0.0, t, 0.0)                       # (... and weight 0)
    t = np.where(t < 1.0, t, 1.0)
    return c.astype(np.int64), t


def _lerp(a, b, t):
    return a + t * (b - a)


class _Grid:
    def __init__(self, flow):
        u, v, w, spacing, origin = flow
        comps = [np.asarray(a, np.float32) for a in (u, v, w)]
        if comps[0].ndim != 3 or any(c.shape != comps[0].shape for c in comps) or min(comps[0].shape) < 2:
            raise ValueError("u, v, w must be three arrays of one shape [nz][ny][nx], each axis >= 2 nodes")
        self.nz, self.ny, self.nx = comps[0].shape
        self.uvw = np.stack([c.reshape(-1) for c in comps], 1).astype(np.float64)      # [nodes][3], f32 values widened
        self.spacing = [float(s) for s in spacing]
        self.origin = [float(o) for o in origin]

    def sample(self, x, y, z):
        """V at the points (x, y, z): [n][3] f64, in the order of include/parallel_ray_tracing.h."""
        with np.errstate(invalid="ignore"):
            i, tx = _axis(x, self.origin[0], self.spacing[0], self.nx)
            j, ty = _axis(y, self.origin[1], self.spacing[1], self.ny)
            k, tz = _axis(z, self.origin[2], self.spacing[2], self.nz)
        sy, sz = self.nx, self.nx * self.ny
        b = k * sz + j * sy + i
        g = self.uvw
        tx, ty, tz = tx[:, None], ty[:, None], tz[:, None]
        c0 = _lerp(_lerp(g[b], g[b + 1], tx), _lerp(g[b + sy], g[b + sy + 1], tx), ty)
        c1 = _lerp(_lerp(g[b + sz], g[b + sz + 1], tx), _lerp(g[b + sz + sy], g[b + sz + sy + 1], tx), ty)
        return _lerp(c0, c1, tz)


def sample_flow(flow, points) -> np.ndarray:
    """The trilinear velocity of `flow` ((u, v, w, spacing, origin)) at points [n][3] -> [n][3] f64."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return _Grid(flow).sample(p[:, 0], p[:, 1], p[:, 2])


def advect(seed: int, n: int, box_min, box_max, z_object: float, beam_fwhm: float, irradiance_constant: float,
           diameter_cdf=None, flow=None, t: float = 0.0, steps: int = 16) -> dict:
    """Host model of photon_sources_piv_advected: piv_field's particles moved through `flow` ((u, v, w, spacing, origin))
    by `steps` classical RK4 steps of h = t / steps, stored like piv_field; "world" = the f64 positions at time t."""
    if int(steps) < 1 or not math.isfinite(float(t)) or (float(t) != 0.0 and flow is None):
        raise ValueError("advect: steps >= 1, a finite t, and a flow when t != 0")
    X, Y, Z, ud = _draw(seed, n, box_min, box_max)
    if flow is not None and float(t) != 0.0:
        g = _Grid(flow)
        h = float(t) / int(steps)
        hh, h6 = 0.5 * h, h / 6.0
        for _ in range(int(steps)):
            k1 = g.sample(X, Y, Z)
            k2 = g.sample(X + hh * k1[:, 0], Y + hh * k1[:, 1], Z + hh * k1[:, 2])
            k3 = g.sample(X + hh * k2[:, 0], Y + hh * k2[:, 1], Z + hh * k2[:, 2])
            k4 = g.sample(X + h * k3[:, 0], Y + h * k3[:, 1], Z + h * k3[:, 2])
            d = k1 + 2.0 * k2 + 2.0 * k3 + k4
            X, Y, Z = X + h6 * d[:, 0], Y + h6 * d[:, 1], Z + h6 * d[:, 2]
    return _store(X, Y, Z, ud, z_object, beam_fwhm, irradiance_constant, diameter_cdf)


# ---- grid fillers: (u, v, w [nz][ny][nx] f32, spacing, origin) on the box [lo, hi] with n nodes per axis -----------------
def grid_nodes(lo, hi, n):
    """Node coordinates of the grid [lo, hi] with n (an int or three) nodes per axis: (x [nx], y [ny], z [nz], spacing,
    origin); node (i, j, k) sits at origin + (i, j, k) * spacing."""
    nn = [int(n)] * 3 if np.ndim(n) == 0 else [int(v) for v in n]
    if min(nn) < 2:
        raise ValueError("a grid needs at least 2 nodes per axis")
    origin = tuple(float(v) for v in lo)
    spacing = tuple((float(hi[a]) - origin[a]) / (nn[a] - 1) for a in range(3))
    axes = [origin[a] + spacing[a] * np.arange(nn[a], dtype=np.float64) for a in range(3)]
    return axes[0], axes[1], axes[2], spacing, origin


def _pack(fu, fv, fw, lo, hi, n):
    x, y, z, spacing, origin = grid_nodes(lo, hi, n)
    Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
    return (np.ascontiguousarray(np.broadcast_to(fu(Xg, Yg, Zg), Xg.shape), np.float32),
            np.ascontiguousarray(np.broadcast_to(fv(Xg, Yg, Zg), Xg.shape), np.float32),
            np.ascontiguousarray(np.broadcast_to(fw(Xg, Yg, Zg), Xg.shape), np.float32), spacing, origin)


def uniform_flow(velocity, lo, hi, n=2):
    """The same velocity (u, v, w) at every node."""
    u, v, w = (float(c) for c in velocity)
    return _pack(lambda X, Y, Z: u, lambda X, Y, Z: v, lambda X, Y, Z: w, lo, hi, n)


def solid_body_rotation(omega: float, lo, hi, n=17, centre=(0.0, 0.0)):
    """Rotation at angular velocity omega (radians per unit of t, counter-clockwise seen from +z) about the axis through
    (centre[0], centre[1]) parallel to z: u = -omega (y - cy), v = omega (x - cx), w = 0.  An affine field, which
    trilinear interpolation reproduces to the f32 rounding of the nodes."""
    om, cx, cy = float(omega), float(centre[0]), float(centre[1])
    return _pack(lambda X, Y, Z: -om * (Y - cy), lambda X, Y, Z: om * (X - cx), lambda X, Y, Z: 0.0, lo, hi, n)


def lamb_oseen_factor(gamma: float, core_radius: float, r2):
    """u_theta / r of the Lamb-Oseen vortex, Gamma / (2 pi r^2) (1 - exp(-r^2 / rc^2)), at squared radii r2 (its limit
    Gamma / (2 pi rc^2) at the axis)."""
    s = np.asarray(r2, np.float64) / (float(core_radius) ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(s > 0, -np.expm1(-s) / np.where(s > 0, s, 1.0), 1.0)
    return float(gamma) / (2.0 * math.pi * float(core_radius) ** 2) * g


def lamb_oseen_peak_speed(gamma: float, core_radius: float) -> float:
    """Largest u_theta of the vortex: 0.638 Gamma / (2 pi rc), at r = 1.1209 rc."""
    xi = 1.1209189
    return float(gamma) / (2.0 * math.pi * float(core_radius)) * (1.0 - math.exp(-xi * xi)) / xi


def lamb_oseen_vortex(gamma: float, core_radius: float, centre, lo, hi, n=65):
    """Lamb-Oseen vortex of circulation gamma (microns^2 per unit of t) and core radius rc about the axis through
    (centre[0], centre[1]) parallel to z: u_theta(r) = Gamma / (2 pi r) (1 - exp(-r^2 / rc^2)), no radial or axial flow."""
    cx, cy = float(centre[0]), float(centre[1])

    def fac(X, Y):
        return lamb_oseen_factor(gamma, core_radius, (X - cx) ** 2 + (Y - cy) ** 2)
    return _pack(lambda X, Y, Z: -fac(X, Y) * (Y - cy), lambda X, Y, Z: fac(X, Y) * (X - cx), lambda X, Y, Z: 0.0 * X, lo, hi, n)


def add_flows(a, b):
    """The sum of two fields on the same grid."""
    if any(not np.allclose(p, q, rtol=0, atol=0) for p, q in ((a[3], b[3]), (a[4], b[4]))) or a[0].shape != b[0].shape:
        raise ValueError("the two fields must share one grid")
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3], a[4])


# ---- image displacements from two moment records -----------------------------------------------------------------------
def image_displacements(rec1, rec2, camera, rays_per_source: int) -> np.ndarray:
    """Per-particle centroid shift, frame 2 minus frame 1, in pixels [particles][2] (x, y along the sensor's pixel axes,
    deflections.to_pixels), from the moment records of the two frames' traces (one record per particle, the same order
    in both).  A particle's centroid is the mean sensor position of the rays of it that arrived; a particle that arrived
    in only one frame (or in neither) gives NaN."""
    m1 = deflections.dot_means(rec1, rays_per_source, 1, "arrived")
    m2 = deflections.dot_means(rec2, rays_per_source, 1, "arrived")
    return deflections.to_pixels(m2["pos"], camera) - deflections.to_pixels(m1["pos"], camera)
