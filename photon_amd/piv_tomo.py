"""Tomographic PIV (pure numpy: usable without a GPU): N cameras on one volume, three displacement components on a 3-D grid.

The device forms are photon_piv_volume_los and photon_piv_correlate_volume (include/parallel_ray_tracing.h, section 20;
``PhotonLibrary.piv_volume_los`` / ``piv_correlate_volume`` on raw device pointers, ``PhotonLibrary.reconstruct_volume`` and
``PhotonLibrary.correlate_tomo`` on arrays).  This module holds what the C side has no part in and the host models:

* the volume -- a dict x0, y0, z0, pitch, nx, ny, nz: voxel (k, i, j) is the world point (x0 + j pitch, y0 + i pitch, z0 + k
  pitch) -- ``volume``, ``centred_volume``, ``slice_plane`` (slice k as a piv_stereo plane) and ``los_coefficients`` (every
  camera folded at every slice: what the kernel takes);
* ``los_model_f32`` (built from piv_stereo.dewarp_model_f32: the device equals it bit for bit) and ``los_model`` (f64);
* ``correlate_volume_model``: section 20b in f64, planes included; on a volume of one slice it is
  piv_correlation.correlate_model exactly (the same numpy operations on the same values);
* ``correlate_tomo_model``: the model of the driver's chain;
* generators for the tests and tools: ``particle_volume_pair`` (particles in a slab around the volume, displaced by a flow,
  imaged through any number of pinhole cameras), ``true_volume`` and ``quality`` (the normalised correlation Q of a
  reconstruction with the true particle field), and the synthetic cases the tests and tools/piv_tomo.py measure (``CASES``,
  ``case_inputs``, ``case_figures``).

Reconstruction here is by line of sight (MinLOS, multiplicative LOS without the N-th root); MART from that first guess is
photon_amd/piv_mart.py (section 21).  What does not exist: SMART and MLEM, 3-D vector validation, multi-pass refinement and
volume deformation, volumetric self-calibration, masks and window weights in 3-D, sum-of-correlation over volume pairs.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc
from . import piv_deformation as pd
from . import piv_stereo as ps

MODES = {"min": 0, "product": 1}
MAX_CAMERAS = 8
MAX_WIN_Z = 64
MAX_RADIUS_Z = 16


# ---- the volume ------------------------------------------------------------------------------------------------------------------
def volume(x0, y0, z0, pitch, nx, ny, nz) -> dict:
    v = dict(x0=float(x0), y0=float(y0), z0=float(z0), pitch=float(pitch), nx=int(nx), ny=int(ny), nz=int(nz))
    if not all(np.isfinite(v[k]) for k in ("x0", "y0", "z0", "pitch")) or v["pitch"] <= 0 or min(v["nx"], v["ny"], v["nz"]) < 1:
        raise ValueError("a volume needs finite x0, y0, z0, a pitch > 0 and a size >= 1")
    return v


def centred_volume(nx: int, ny: int, nz: int, pitch: float) -> dict:
    """The volume whose grid is centred on the world origin."""
    return volume(-(int(nx) - 1) / 2.0 * pitch, -(int(ny) - 1) / 2.0 * pitch, -(int(nz) - 1) / 2.0 * pitch, pitch, nx, ny, nz)


def shape_of(vol):
    return int(vol["nz"]), int(vol["ny"]), int(vol["nx"])


def slice_plane(vol, k: int) -> dict:
    """Slice k of the volume as a piv_stereo plane."""
    return ps.plane(vol["x0"], vol["y0"], vol["pitch"], vol["z0"] + int(k) * vol["pitch"], vol["nx"], vol["ny"])


def los_coefficients(cameras, vol):
    """Every camera folded at every slice by piv_stereo.plane_coefficients: (poly f64 [N, nz, 2, 10], grid f64 [N, 4])."""
    if not 2 <= len(cameras) <= MAX_CAMERAS:
        raise ValueError(f"a line-of-sight volume takes 2 to {MAX_CAMERAS} cameras")
    poly, grid = np.empty((len(cameras), vol["nz"], 2, 10)), np.empty((len(cameras), 4))
    for c, cam in enumerate(cameras):
        for k in range(vol["nz"]):
            poly[c, k], grid[c] = ps.plane_coefficients(cam, slice_plane(vol, k))
    return poly, grid


# ---- line of sight -----------------------------------------------------------------------------------------------------------------
def _mode(mode):
    if mode not in MODES and mode not in MODES.values():
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    return MODES.get(mode, mode)


def _combine(samples, outside, mode, zero):
    """samples: per camera [n, ny, nx]; outside: per camera bool [ny, nx]."""
    any_out = np.logical_or.reduce(outside)
    acc = None
    for s in samples:
        v = np.where(s > 0, s, zero)
        acc = v if acc is None else (np.where(v < acc, v, acc) if mode == 0 else acc * v)
    return np.where(any_out, zero, acc), any_out


def los_model_f32(coefs, poly, grids, shape, mode="min"):
    """Host model of photon_piv_volume_los in the kernel's own operations.  coefs: per camera the section 7a coefficients f32
    [n, height, width] (or [height, width]); poly, grids from los_coefficients; shape (nz, ny, nx).  Per slice and camera
    piv_stereo.dewarp_model_f32, then the samples clamped at 0 and combined in camera order.  Returns (volumes f32 [n, nz, ny,
    nx], mask u8 [nz, ny, nx]); the device returns these bits."""
    mode = _mode(mode)
    nz, ny, nx = (int(v) for v in shape)
    stacks = [ps._stack(c, np.float32)[0] for c in coefs]
    out = np.zeros((stacks[0].shape[0], nz, ny, nx), np.float32)
    mask = np.zeros((nz, ny, nx), np.uint8)
    for k in range(nz):
        each = [ps.dewarp_model_f32(c, poly[i][k], grids[i], (ny, nx)) for i, c in enumerate(stacks)]
        out[:, k], outside = _combine([e[0] for e in each], [e[1] != 0 for e in each], mode, np.float32(0))
        mask[k] = outside
    return out, mask


def los_samples(camera_frames, poly, grids, shape):
    """The cameras' samples at every voxel in f64, before they are clamped and combined: (samples f64 [N, n, nz, ny, nx], 0
    where the camera does not see the voxel; outside bool [N, nz, ny, nx])."""
    nz, ny, nx = (int(v) for v in shape)
    stacks = [ps._stack(f, np.float64)[0] for f in camera_frames]
    samples = np.zeros((len(stacks), stacks[0].shape[0], nz, ny, nx))
    outside = np.zeros((len(stacks), nz, ny, nx), bool)
    for i, s in enumerate(stacks):
        c = np.stack([pd.bspline_coefficients_model(f) for f in s])
        for k in range(nz):
            inside, tx, ty, xi, yi = ps._taps(poly[i][k], grids[i], (ny, nx), c.shape[-2:])
            samples[i, :, k], outside[i, k] = np.where(inside, ps.bspline_sample(c, tx, ty, xi, yi), 0.0), ~inside
    return samples, outside


def los_model(camera_frames, poly, grids, shape, mode="min"):
    """The line-of-sight volume in f64 throughout, from the frames themselves (per camera [n, height, width] or [height,
    width]): (volumes f64 [n, nz, ny, nx], mask u8 [nz, ny, nx])."""
    samples, outside = los_samples(camera_frames, poly, grids, shape)
    out, any_out = _combine(list(samples), list(outside), _mode(mode), 0.0)
    return out, any_out.astype(np.uint8)


# ---- the 3-D correlation -----------------------------------------------------------------------------------------------------------
def z_defaults(vol, win: int, radius: int, win_z=None, step_z=None, radius_z=None):
    """The driver's defaults along z: win_z = win capped at 64 and nz; step_z = max(1, win_z / 2); radius_z = min(radius, 16,
    win_z / 2)."""
    win_z = min(int(win), MAX_WIN_Z, int(vol["nz"])) if win_z is None else int(win_z)
    step_z = max(1, win_z // 2) if step_z is None else int(step_z)
    radius_z = min(int(radius), MAX_RADIUS_Z, win_z // 2) if radius_z is None else int(radius_z)
    return win_z, step_z, radius_z


def check_arguments(shape, win: int, step: int, radius: int, win_z: int, step_z: int, radius_z: int):
    """The arguments photon_piv_correlate_volume refuses, as a ValueError.  shape: (nz, ny, nx)."""
    nz, ny, nx = (int(v) for v in shape)
    pc.check_arguments((ny, nx), win, step, radius)
    if not 1 <= int(win_z) <= MAX_WIN_Z:
        raise ValueError(f"win_z must be within [1, {MAX_WIN_Z}], not {win_z}")
    if int(step_z) < 1:
        raise ValueError(f"step_z must be >= 1, not {step_z}")
    if not 0 <= int(radius_z) <= min(MAX_RADIUS_Z, int(win_z) // 2):
        raise ValueError(f"radius_z must lie in [0, min({MAX_RADIUS_Z}, win_z / 2)], not {radius_z}")
    if nz < int(win_z):
        raise ValueError(f"a volume of {nz} slices is thinner than one window of {win_z}")


def grid_shape(shape, win: int, step: int, win_z: int, step_z: int):
    """(n_slabs, n_rows, n_cols) of the window grid on a volume of `shape` (nz, ny, nx)."""
    nz, ny, nx = (int(v) for v in shape)
    return ((nz - int(win_z)) // int(step_z) + 1,) + pc.grid_shape((ny, nx), win, step)


def window_centres(vol, win: int, step: int, win_z: int, step_z: int) -> np.ndarray:
    """World points [n_slabs, n_rows, n_cols, 3] of the window centres."""
    n_slabs, n_rows, n_cols = grid_shape(shape_of(vol), win, step, win_z, step_z)
    P = np.empty((n_slabs, n_rows, n_cols, 3))
    P[..., 0] = (vol["x0"] + (np.arange(n_cols) * int(step) + (int(win) - 1) / 2.0) * vol["pitch"])[None, None, :]
    P[..., 1] = (vol["y0"] + (np.arange(n_rows) * int(step) + (int(win) - 1) / 2.0) * vol["pitch"])[None, :, None]
    P[..., 2] = (vol["z0"] + (np.arange(n_slabs) * int(step_z) + (int(win_z) - 1) / 2.0) * vol["pitch"])[:, None, None]
    return P


def raw_volume_planes(vol1, vol2, win: int, step: int, radius: int, win_z: int, step_z: int, radius_z: int, offset=None):
    """What section 20b defines before the peak is read, in f64: (C [n, 2Rz+1, 2R+1, 2R+1], ea [n], eb [n], (ox, oy, oz) [n]
    each, outside [n] bool, (n_slabs, n_rows, n_cols)).  Every sum over the window is taken plane by plane with
    piv_correlation.raw_planes' operations and the planes' sums added in plane order: one plane is raw_planes itself."""
    v1, v2 = np.asarray(vol1, np.float64), np.asarray(vol2, np.float64)
    if v1.ndim != 3 or v1.shape != v2.shape:
        raise ValueError("vol1 and vol2 must be two 3-d arrays of one shape")
    win, step, R, win_z, step_z, Rz = (int(v) for v in (win, step, radius, win_z, step_z, radius_z))
    check_arguments(v1.shape, win, step, R, win_z, step_z, Rz)
    D, H, W = v1.shape
    grid = grid_shape(v1.shape, win, step, win_z, step_z)
    n_slabs, n_rows, n_cols = grid
    n = n_slabs * n_rows * n_cols
    k = np.arange(n)
    in_slab = k % (n_rows * n_cols)
    wz0, wy0, wx0 = (k // (n_rows * n_cols)) * step_z, (in_slab // n_cols) * step, (in_slab % n_cols) * step
    if offset is None:
        ox = oy = oz = np.zeros(n, np.int64)
    else:
        o = np.asarray(offset).reshape(n, 3).astype(np.int64)
        ox, oy, oz = o[:, 0], o[:, 1], (o[:, 2] if D > 1 else np.zeros(n, np.int64))
    span, nS, nSz = win + 2 * R, 2 * R + 1, 2 * Rz + 1
    iw, isp = np.arange(win), np.arange(span)
    gy = wy0[:, None] + oy[:, None] - R + isp
    gx = wx0[:, None] + ox[:, None] - R + isp
    iny, inx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
    inside2 = iny[:, :, None] & inx[:, None, :]
    zero = (slice(None), slice(R, R + win), slice(R, R + win))

    def plus(total, term):
        return term if total is None else total + term

    def b_plane(t):                                                 # the region of vol2 at z = wz0 + oz + t, and where it is inside
        gz = wz0 + oz + t
        zin = (gz >= 0) & (gz < D)
        b = v2[np.clip(gz, 0, D - 1)[:, None, None], np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :]]
        return b, inside2 & zin[:, None, None]

    a_raw = [v1[(wz0 + pz)[:, None, None], (wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :]] for pz in range(win_z)]
    sum_a = sum_b = cnt = None
    for pz in range(win_z):
        sum_a = plus(sum_a, a_raw[pz].sum(axis=(1, 2)))
        b, inside = b_plane(pz)
        cnt = plus(cnt, inside[zero].sum(axis=(1, 2)))
        sum_b = plus(sum_b, np.where(inside[zero], b[zero], 0.0).sum(axis=(1, 2)))
    mean_a = sum_a / (win_z * win * win)
    mean_b = np.where(cnt > 0, sum_b / np.maximum(cnt, 1), 0.0)
    a = [p - mean_a[:, None, None] for p in a_raw]
    bs = {}
    for t in range(-Rz, win_z + Rz):
        b, inside = b_plane(t)
        bs[t] = np.where(inside, b - mean_b[:, None, None], 0.0)
    ea = eb = None
    for pz in range(win_z):
        ea = plus(ea, (a[pz] * a[pz]).sum(axis=(1, 2)))
        eb = plus(eb, (bs[pz][zero] * bs[pz][zero]).sum(axis=(1, 2)))
    C = np.empty((n, nSz, nS, nS), np.float64)
    for sz in range(nSz):
        for sy in range(nS):
            for sx in range(nS):
                c = None
                for pz in range(win_z):
                    c = plus(c, np.einsum("nij,nij->n", a[pz], bs[pz + sz - Rz][:, sy:sy + win, sx:sx + win]))
                C[:, sz, sy, sx] = c
    outside = ~inside2.all(axis=(1, 2)) | (wz0 + oz - Rz < 0) | (wz0 + oz + win_z - 1 + Rz >= D)
    return C, ea, eb, (ox, oy, oz), outside, grid


def peak_outputs_volume(C, R: int, Rz: int, offsets, norm, flat, outside, grid, planes: bool = False):
    """piv_correlation.peak_outputs with one more axis: the first maximum in (sz, sy, sx) order, the three-point fit per
    searched axis, the ratio against the largest value at Chebyshev distance >= 2, the flags.  Returns (vectors [n_slabs,
    n_rows, n_cols, 5], flags int32 [n_slabs, n_rows, n_cols]) and, with planes=True, the normalised planes."""
    ox, oy, oz = offsets
    n, nS, nSz = len(C), 2 * R + 1, 2 * Rz + 1
    k = np.arange(n)
    Cf = C.reshape(n, nSz * nS * nS)
    best = np.argmax(Cf, axis=1)
    pz, py, px = best // (nS * nS), (best % (nS * nS)) // nS, best % nS
    peak_c = Cf[k, best]
    sz_g, sy_g, sx_g = np.meshgrid(np.arange(nSz), np.arange(nS), np.arange(nS), indexing="ij")
    far = np.maximum(np.abs(sz_g[None] - pz[:, None, None, None]),
                     np.maximum(np.abs(sy_g[None] - py[:, None, None, None]), np.abs(sx_g[None] - px[:, None, None, None]))) >= 2
    m2 = np.where(far, C, -np.inf).reshape(n, -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(m2 > 0, peak_c / np.where(m2 > 0, m2, 1.0), np.inf)
    edge_x, edge_y = (px == 0) | (px == nS - 1), (py == 0) | (py == nS - 1)
    edge_z = ((pz == 0) | (pz == nSz - 1)) & (Rz >= 1)
    pxi, pyi = np.clip(px, 1, nS - 2), np.clip(py, 1, nS - 2)
    dx = np.where(edge_x, 0.0, pc._subpixel(C[k, pz, py, pxi - 1], C[k, pz, py, pxi], C[k, pz, py, pxi + 1]))
    dy = np.where(edge_y, 0.0, pc._subpixel(C[k, pz, pyi - 1, px], C[k, pz, pyi, px], C[k, pz, pyi + 1, px]))
    dz = np.zeros(n)
    if Rz >= 1:
        pzi = np.clip(pz, 1, nSz - 2)
        dz = np.where(edge_z, 0.0, pc._subpixel(C[k, pzi - 1, py, px], C[k, pzi, py, px], C[k, pzi + 1, py, px]))
    with np.errstate(invalid="ignore"):
        vectors = np.stack([ox + (px - R) + dx, oy + (py - R) + dy, oz + (pz - Rz) + dz, peak_c * norm, ratio], axis=1)
    flags = np.where(edge_x | edge_y | edge_z, pc.FLAG_EDGE_PEAK, 0) | np.where(outside, pc.FLAG_OUTSIDE, 0)
    flags = np.where(flat, pc.FLAG_FLAT | np.where(outside, pc.FLAG_OUTSIDE, 0), flags).astype(np.int32)
    vectors[flat] = np.nan
    out = (vectors.reshape(grid + (5,)), flags.reshape(grid))
    if planes:
        with np.errstate(invalid="ignore"):
            Cn = C * norm[:, None, None, None]
        Cn[flat] = np.nan
        out = out + (Cn.reshape(grid + (nSz, nS, nS)),)
    return out


def correlate_volume_model(vol1, vol2, win: int, step: int, radius: int, win_z: int, step_z: int, radius_z: int, offset=None,
                           planes: bool = False):
    """Host model of photon_piv_correlate_volume in f64.  vol1, vol2 [nz, ny, nx]; offset: integer (ox, oy, oz) per node,
    [n_slabs, n_rows, n_cols, 3] or [n][3], or None.  Returns (vectors [n_slabs, n_rows, n_cols, 5] = dx, dy, dz, peak, ratio;
    flags int32 [n_slabs, n_rows, n_cols]) and, with planes=True, the normalised planes [n_slabs, n_rows, n_cols, 2Rz+1, 2R+1,
    2R+1].  Flat where an f64 energy is 0 (piv_correlation.correlate_model's note on the device's f32 energies holds)."""
    C, ea, eb, offsets, outside, grid = raw_volume_planes(vol1, vol2, win, step, radius, win_z, step_z, radius_z, offset)
    flat = (ea == 0.0) | (eb == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(ea * eb)
    return peak_outputs_volume(C, int(radius), int(radius_z), offsets, norm, flat, outside, grid, planes)


def windows_touching(mask, win: int, step: int, win_z: int, step_z: int) -> np.ndarray:
    """bool [n_slabs, n_rows, n_cols]: the windows that hold a nonzero voxel of mask [nz, ny, nx]."""
    mask = np.asarray(mask) != 0
    n_slabs, n_rows, n_cols = grid_shape(mask.shape, win, step, win_z, step_z)
    return np.array([[[mask[l * step_z:l * step_z + win_z, i * step:i * step + win, j * step:j * step + win].any() for j in range(n_cols)]
                      for i in range(n_rows)] for l in range(n_slabs)])


def correlate_tomo_model(camera_frames, cameras, vol, win: int = 32, step: int = 16, radius: int = 4, win_z=None, step_z=None,
                         radius_z=None, mode="min", offsets=None):
    """Host model of PhotonLibrary.correlate_tomo in f64: los_model on the two exposures of every camera, then
    correlate_volume_model.  Returns (displacements f64 [n_slabs, n_rows, n_cols, 3] in world units, vectors [.., 5], flags,
    partial bool [n_slabs, n_rows, n_cols])."""
    win_z, step_z, radius_z = z_defaults(vol, win, radius, win_z, step_z, radius_z)
    check_arguments(shape_of(vol), win, step, radius, win_z, step_z, radius_z)
    volumes, mask = los_model(camera_frames, *los_coefficients(cameras, vol), shape_of(vol), mode)
    if volumes.shape[0] != 2:
        raise ValueError("correlate_tomo takes the two exposures of each camera, [2, height, width]")
    vectors, flags = correlate_volume_model(volumes[0], volumes[1], win, step, radius, win_z, step_z, radius_z, offsets)
    return vol["pitch"] * vectors[..., :3], vectors, flags, windows_touching(mask, win, step, win_z, step_z)


# ---- generators ------------------------------------------------------------------------------------------------------------------
def particle_volume_pair(cameras, flow, vol, seed: int, shape=(96, 96), ppp: float = 0.03, diameter: float = 2.5, margin: float = 4.0):
    """Two exposures per camera of particles that move with `flow`: particles scattered uniformly in a slab `margin` voxels
    larger than the volume on every side, `ppp` per voxel column of the slab (particles per pixel of a camera that images a
    voxel onto a pixel), particle k at P_k - flow(P_k) / 2 in the first exposure and P_k + flow(P_k) / 2 in the second,
    imaged as a Gaussian of e^-2 diameter `diameter` px through each of `cameras` (piv_stereo.Pinhole objects or fitted
    cameras; any number).  flow(P [n, 3]) -> [n, 3] world units.  Returns (one f32 stack [2, height, width] per camera;
    (P [n, 3], brightness [n], half [n, 3]): the particles, for true_volume)."""
    rng = np.random.default_rng(seed)
    p = vol["pitch"]
    lo = np.array([vol["x0"], vol["y0"], vol["z0"]]) - margin * p
    hi = np.array([vol["x0"] + (vol["nx"] - 1) * p, vol["y0"] + (vol["ny"] - 1) * p, vol["z0"] + (vol["nz"] - 1) * p]) + margin * p
    n = int(round(ppp * (hi[0] - lo[0]) * (hi[1] - lo[1]) / p ** 2))
    P = rng.uniform(lo, hi, (n, 3))
    brightness = rng.uniform(0.5, 1.0, n)
    half = 0.5 * np.asarray(flow(P), np.float64)
    out = []
    for cam in cameras:
        out.append(np.stack([ps._render(ps._project(cam, Q), brightness, shape, diameter) for Q in (P - half, P + half)]).astype(np.float32))
    return tuple(out), (P, brightness, half)


def true_volume(vol, positions, brightness, diameter: float = 2.5, reach: int = 3) -> np.ndarray:
    """The particle field itself on the volume's grid, f64 [nz, ny, nx]: Gaussian blobs of e^-2 diameter `diameter` voxels at
    the world points `positions` [n, 3], sampled at the voxel centres."""
    nz, ny, nx = shape_of(vol)
    q = (np.asarray(positions, np.float64) - np.array([vol["x0"], vol["y0"], vol["z0"]])) / vol["pitch"]       # (x, y, z) in voxels
    out = np.zeros((nz, ny, nx))
    c = np.rint(q).astype(np.int64)
    for dz in range(-reach, reach + 1):
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                ix, iy, iz = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
                ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny) & (iz >= 0) & (iz < nz)
                r2 = (ix[ok] - q[ok, 0]) ** 2 + (iy[ok] - q[ok, 1]) ** 2 + (iz[ok] - q[ok, 2]) ** 2
                np.add.at(out, (iz[ok], iy[ok], ix[ok]), np.asarray(brightness)[ok] * np.exp(-8.0 * r2 / diameter ** 2))
    return out


def quality(E, truth) -> float:
    """The normalised correlation Q of a reconstruction E with the true field: sum E T / sqrt(sum E^2 sum T^2)."""
    E, T = np.asarray(E, np.float64), np.asarray(truth, np.float64)
    return float((E * T).sum() / np.sqrt((E * E).sum() * (T * T).sum()))


# ---- the synthetic cases of the tests and of tools/piv_tomo.py --------------------------------------------------------------------
CASE_VOLUME = centred_volume(64, 64, 24, 0.1)          # 6.4 x 6.4 x 2.4 mm at 0.1 mm per voxel
CASE_SENSOR = (96, 96)
CASE_GRID = dict(win=16, step=8, radius=3, win_z=16, step_z=4, radius_z=3)
CASE_PPP = 0.08
CASE_SEEDS = tuple(range(8))


def uniform_flow(P):
    return np.broadcast_to(np.array([0.16, -0.09, 0.12]), np.shape(P))          # 1.6, -0.9, 1.2 voxels


def shear_flow(P):
    P = np.asarray(P, np.float64)
    return np.stack([0.10 + 0.02 * P[..., 1], np.full(P.shape[:-1], -0.07), 0.08 + 0.015 * P[..., 0]], axis=-1)


_FOUR = ((30.0, 15.0), (-30.0, 15.0), (30.0, -15.0), (-30.0, -15.0))               # (theta, phi) in degrees: azimuth and elevation
CASES = {
    "uniform": dict(angles=_FOUR, flow=uniform_flow),
    "shear": dict(angles=_FOUR, flow=shear_flow),
    "four_cross": dict(angles=((-35.0, 0.0), (35.0, 0.0), (0.0, -25.0), (0.0, 25.0)), flow=uniform_flow),
    "three": dict(angles=((-30.0, -10.0), (0.0, 15.0), (30.0, -10.0)), flow=uniform_flow),
}


def calibrated_views(angles, vol=None, shape=CASE_SENSOR, distance: float = 300.0, px_per_mm: float = 10.0):
    """((pinhole, fitted camera, rms, max residual) per (theta, phi) of `angles`): pinholes at `distance` with `px_per_mm` at
    the origin, fitted on a 9 x 9 x 5 target that spans the volume."""
    vol = CASE_VOLUME if vol is None else vol
    mid = slice_plane(vol, 0)
    mid["z"] = vol["z0"] + (vol["nz"] - 1) / 2.0 * vol["pitch"]
    depth = (vol["nz"] - 1) / 2.0 * vol["pitch"] * 1.2
    target = ps.calibration_target(mid, 9, np.linspace(-depth, depth, 5))
    out = []
    for theta, phi in angles:
        view = ps.pinhole(np.deg2rad(theta), np.deg2rad(phi), distance, px_per_mm, shape)
        out.append((view, *ps.fit_camera(target, view.project(target))))
    return tuple(out)


def case_inputs(name: str, seed: int = 0):
    """(frames per camera f32 [2, 96, 96], the fitted cameras, CASE_VOLUME, the particles) of CASES[name] at `seed`, rendered
    through the pinholes themselves."""
    case = CASES[name]
    views = calibrated_views(case["angles"])
    frames, particles = particle_volume_pair([v[0] for v in views], case["flow"], CASE_VOLUME, 1000 + seed, shape=CASE_SENSOR, ppp=CASE_PPP)
    return frames, tuple(v[1] for v in views), CASE_VOLUME, particles


def interior(grid):
    """The index of the nodes that touch no face of the window grid (all of an axis that has fewer than 3 nodes)."""
    return tuple(slice(1, -1) if n >= 3 else slice(None) for n in grid)


def case_figures(name: str, displacements, flags=None):
    """Of a result on CASES[name] (world displacements [n_slabs, n_rows, n_cols, 3] on CASE_GRID), over the interior nodes, in
    voxels: (rms error of dX, dY, dZ; the number of interior nodes)."""
    g = CASE_GRID
    truth = CASES[name]["flow"](window_centres(CASE_VOLUME, g["win"], g["step"], g["win_z"], g["step_z"]))
    err = ((np.asarray(displacements) - truth) / CASE_VOLUME["pitch"])[interior(truth.shape[:3])]
    return np.sqrt(np.mean(err ** 2, axis=(0, 1, 2))), int(err[..., 0].size)
