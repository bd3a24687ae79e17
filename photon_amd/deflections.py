"""Dot shifts of a synthetic BOS / PIV pair from per-source sensor moments (pure numpy).

A trace with moments (``PhotonLibrary.render_moments``, ``Scene.trace_moments``; include/parallel_ray_tracing.h,
photon_trace_moments) returns one record of 8 doubles per source, reduced on the GPU from the rays of that source that
reached the sensor.  This module turns records into what the reference's dump workflow computes
(python_codes/light_ray_processing.py:532-639, process_lightray_data): dot-averaged positions in pixels, ray angles, and
the deflections between image 1 (no density gradients) and image 2 (through the volume) -- without writing or reading
a single ray dump.  ``moments_from_dumps`` is the host model of a record: the device's summation order, on the
arrays of pos_ / dir_ dumps (from this library or from a CUDA run of the reference).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

# record layout: n = rays that reached the sensor; sums over those rays of the final sensor-plane position (camera frame,
# microns), of acos of the direction components the dumps hold (radians), and of x^2 + y^2
RECORD_FIELDS = ("n", "sum_x", "sum_y", "sum_z", "sum_acos_dx", "sum_acos_dy", "sum_acos_dz", "sum_r2")
LANES = 64


def _values(pos: np.ndarray, dirs: np.ndarray) -> np.ndarray:
    """[rays][8] f64 summands of a record; +0.0 for a ray that did not arrive (adds nothing to a partial that is never -0.0)."""
    arrived = ~np.isnan(pos).any(axis=1)
    x = pos.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ang = np.arccos(dirs.astype(np.float64))
    v = np.empty((pos.shape[0], 8), np.float64)
    v[:, 0] = 1.0
    v[:, 1:4] = x
    v[:, 4:7] = ang
    v[:, 7] = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]         # both squares exact in f64: one rounding, as on the device
    v[~arrived] = 0.0
    return v


def moments_from_dumps(pos, dir, rays_per_source: int, max_rays: int = 1 << 22) -> np.ndarray:  # noqa: A002
    """Records f64[sources][8] of rays given as pos_ / dir_ dump arrays (f32 [rays][3], source-major: ray j of source s at
    s * rays_per_source + j), in the device's order: lane l of 64 adds the rays j = l (mod 64) in increasing j from +0.0,
    then the 64 partials are folded by halves.  n, the position sums and sum_r2 equal the device's bit for bit; the acos
    sums may differ from it by an ulp of f64 acos per ray."""
    rps = int(rays_per_source)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    dirs = np.asarray(dir, np.float32).reshape(-1, 3)
    if rps < 1 or pos.shape != dirs.shape or pos.shape[0] % rps:
        raise ValueError(f"{pos.shape[0]} rays / {dirs.shape[0]} directions do not make whole sources of {rps} rays")
    n_src = pos.shape[0] // rps
    rounds = -(-rps // LANES)
    out = np.empty((n_src, 8), np.float64)
    step = max(1, max_rays // (rounds * LANES))
    for s0 in range(0, n_src, step):
        s1 = min(n_src, s0 + step)
        v = _values(pos[s0 * rps:s1 * rps], dirs[s0 * rps:s1 * rps]).reshape(s1 - s0, rps, 8)
        pad = np.zeros((s1 - s0, rounds * LANES, 8), np.float64)
        pad[:, :rps] = v
        pad = pad.reshape(s1 - s0, rounds, LANES, 8)
        p = np.zeros((s1 - s0, LANES, 8), np.float64)
        for k in range(rounds):                             # increasing j per lane
            p = p + pad[:, k]
        off = LANES // 2
        while off:                                          # p[l] += p[l + off], l < off
            p[:, :off] = p[:, :off] + p[:, off:2 * off]
            off //= 2
        out[s0:s1] = p[:, 0]
    return out


def dot_means(records, rays_per_source: int, group: int = 1, policy: str = "reference") -> dict:
    """Per-dot means from records.  ``group`` = k merges k consecutive sources into one dot (a BOS pattern of bos_pattern /
    photon_sources_bos: its points_per_dot sources).  Returns {"n": rays arrived, "pos": [dots][3] microns, "dir": [dots][3]
    radians (mean acos of the direction components), "r2": [dots] mean x^2 + y^2}.

    policy "reference": NaN unless every ray of the dot arrived.  For positions that is exactly the reference's
    np.add.reduceat(...) / rays (light_ray_processing.py:243-275): a ray that misses the sensor is NaN in pos_ dumps.
    For angles it differs only for a dot whose rays all left the volume but some missed the sensor: the reference still
    averages their finite dir_ entries, this gives NaN.
    policy "arrived": sums over the rays that arrived divided by their number (NaN for a dot with none)."""
    rec = np.asarray(records, np.float64).reshape(-1, 8)
    k = int(group)
    if k < 1 or rec.shape[0] % k:
        raise ValueError(f"{rec.shape[0]} records do not make whole dots of {k} sources")
    rec = rec.reshape(-1, k, 8)
    tot = rec[:, 0].copy()
    for i in range(1, k):                                   # records are additive
        tot = tot + rec[:, i]
    n = tot[:, 0]
    if policy == "reference":
        full = float(k * int(rays_per_source))
        denom = np.where(n == full, full, np.nan)
    elif policy == "arrived":
        denom = np.where(n > 0, n, np.nan)
    else:
        raise ValueError(f"policy must be 'reference' or 'arrived', not {policy!r}")
    mean = tot / denom[:, None]
    return {"n": n, "pos": mean[:, 1:4], "dir": mean[:, 4:7], "r2": mean[:, 7]}


def _camera(camera) -> dict:
    return camera.camera if hasattr(camera, "camera") else camera


def to_pixels(pos, camera) -> np.ndarray:
    """Sensor-plane positions (microns, [..., >= 2]) -> pixels [..., 2] as light_ray_processing.py:277-300, 513-531 do it:
    (p - p0) / pixel_pitch with p0 = -(pixels / 2 - 1) * pixel_pitch.  Each axis uses its own pixel count; the reference
    uses x_pixel_number for both, which is the same for its square sensors.  ``camera``: a camera dict or a call."""
    cam = _camera(camera)
    pitch = float(cam["pixel_pitch"])
    p = np.asarray(pos, np.float64)
    out = np.empty(p.shape[:-1] + (2,), np.float64)
    for axis, key in ((0, "x_pixel_number"), (1, "y_pixel_number")):
        p0 = -(int(cam[key]) / 2 - 1) * pitch
        out[..., axis] = (p[..., axis] - p0) / pitch
    return out


class DotDeflections(NamedTuple):
    pos1: np.ndarray        # [dots][2] pixels, image 1
    pos2: np.ndarray        # [dots][2] pixels, image 2
    dir1: np.ndarray        # [dots][3] radians, image 1
    dir2: np.ndarray        # [dots][3] radians, image 2
    d_pos: np.ndarray       # pos1 - pos2, pixels (the reference's sign, light_ray_processing.py:228-239)
    d_dir: np.ndarray       # dir2 - dir1, radians
    rms1: np.ndarray        # [dots] rms spot radius of the dot's image about its centroid, pixels, image 1
    rms2: np.ndarray        # the same, image 2


def _rms_px(m: dict, pitch: float) -> np.ndarray:
    var = m["r2"] - (m["pos"][:, 0] ** 2 + m["pos"][:, 1] ** 2)
    return np.sqrt(np.maximum(var, 0.0)) / pitch


def dot_deflections(rec_im1, rec_im2, camera, rays_per_source: int, group: int = 1, policy: str = "reference") -> DotDeflections:
    """The dot shifts of an image pair from the records of its two traces (process_lightray_data without the dumps)."""
    m1 = dot_means(rec_im1, rays_per_source, group, policy)
    m2 = dot_means(rec_im2, rays_per_source, group, policy)
    pos1, pos2 = to_pixels(m1["pos"], camera), to_pixels(m2["pos"], camera)
    pitch = float(_camera(camera)["pixel_pitch"])
    return DotDeflections(pos1, pos2, m1["dir"], m2["dir"], pos1 - pos2, m2["dir"] - m1["dir"], _rms_px(m1, pitch), _rms_px(m2, pitch))


def summary(d: DotDeflections) -> str:
    """The reference's summary lines (light_ray_processing.py:623-624)."""
    return "\n".join("%s: %.2f to %.2f pix." % (axis, np.nanmin(d.d_pos[:, i]), np.nanmax(d.d_pos[:, i])) for i, axis in enumerate("xy"))
