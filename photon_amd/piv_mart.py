"""MART particle volumes for tomographic PIV (pure numpy: usable without a GPU): the exact re-projection of a volume onto
the cameras and the multiplicative update that starts from a line-of-sight volume (MLOS-MART).

The device forms are photon_piv_volume_project and photon_piv_volume_mart (include/parallel_ray_tracing.h, section 21;
``PhotonLibrary.piv_volume_project`` / ``piv_volume_mart`` on raw device pointers, ``PhotonLibrary.reproject`` and
``reconstruct_volume(method="mart")`` / ``correlate_tomo(reconstruction="mart")`` on arrays).  This module holds the host
models:

* ``footprint``: where voxel (k, i, j) lands on a camera -- piv_tomo's coordinate pipeline, then four bilinear taps and their
  weights; ``volume_footprint``: the same for every slice;
* ``project_model``: the re-projection in 64-bit integer fixed point, exact: integer addition is associative, so any order
  of the voxels returns the same integers, and so does the device with its atomics; ``images_of``: the accumulators as f32;
* ``mart_model_f32``: section 21b in the kernel's own operations (the device returns these bits); ``mart_model``: the same
  algorithm in f64 without the quantisation;
* ``scale_log2_for``, ``default_threshold``, ``mu_roots_of``, ``check_arguments``: what the drivers decide on the host;
* ``reconstruct_model`` and ``mart_tomo_model``: the models of the drivers' chains in f64;
* the synthetic cases ``CASES`` (piv_tomo.CASES and one whose particles all lie inside the volume), ``case_inputs``,
  ``case_figures`` and ``interior_quality``.

The voxel-driven, camera-sequential form: the ratio of the frame to the re-projection is gathered at the voxel's footprint
with the weights the projection scattered with (a matched pair) and raised to the relaxation mu alone; with mu in {1, 1/2,
1/4, 1/8} the power is 0 to 3 correctly rounded square roots.  What does not exist: SMART and MLEM, volumetric
self-calibration, masks and weights in 3-D.
"""
from __future__ import annotations

import numpy as np

from . import piv_stereo as ps
from . import piv_tomo as pt

MAX_CAMERAS = pt.MAX_CAMERAS
MAX_MU_ROOTS = 3
SCALE_LOG2_RANGE = (-126, 62)
CAP = float(2 ** 31)                        # the largest contribution of one voxel to one tap
RELAXATIONS = {1.0: 0, 0.5: 1, 0.25: 2, 0.125: 3}
DEFAULT_THRESHOLD = 1e-4                    # of the frames' maximum


# ---- the footprint -----------------------------------------------------------------------------------------------------------------
def footprint(poly_k, grid, out_shape, sensor_shape, dtype=np.float32):
    """Where the voxels of one slice land on a camera.  poly_k f64 [2, 10] and grid f64 [4]: the camera folded at the slice
    (piv_tomo.los_coefficients); out_shape (ny, nx); sensor_shape (height, width).  The inside test (a NaN is outside), x0 =
    floor(x) and x - x0 are piv_stereo.sensor_points'; fx = dtype(x - x0), the x taps x0 and min(x0 + 1, width - 1) with the
    weights 1 - fx and fx; the same in y; the four weights wy wx in `dtype`, in the order (y0, x0), (y0, x1), (y1, x0), (y1,
    x1).  Returns (inside bool [ny, nx], pixel index int64 [4, ny, nx] = y width + x, weights dtype [4, ny, nx]); outside
    voxels hold index 0 and what the coordinate (0, 0) gives."""
    h, w = (int(v) for v in sensor_shape)
    inside, ix0, iy0, tx, ty = ps.sensor_points(poly_k, grid, out_shape, (h, w))
    one = dtype(1)
    fx, fy = tx.astype(dtype), ty.astype(dtype)
    wx, wy = (one - fx, fx), (one - fy, fy)
    ix, iy = (ix0, np.minimum(ix0 + 1, w - 1)), (iy0, np.minimum(iy0 + 1, h - 1))
    index = np.stack([iy[a] * w + ix[b] for a in (0, 1) for b in (0, 1)])
    weights = np.stack([wy[a] * wx[b] for a in (0, 1) for b in (0, 1)])
    return inside, index, weights


def volume_footprint(poly_c, grid, shape, sensor_shape, dtype=np.float32):
    """footprint at every slice: poly_c f64 [nz, 2, 10]; shape (nz, ny, nx).  Returns (inside [nz, ny, nx], index [4, nz, ny,
    nx], weights [4, nz, ny, nx])."""
    nz, ny, nx = (int(v) for v in shape)
    each = [footprint(poly_c[k], grid, (ny, nx), sensor_shape, dtype) for k in range(nz)]
    return np.stack([e[0] for e in each]), np.stack([e[1] for e in each], axis=1), np.stack([e[2] for e in each], axis=1)


# ---- the host's decisions ------------------------------------------------------------------------------------------------------
def mu_roots_of(relaxation) -> int:
    """The number of square roots that raise the ratio to `relaxation`: 1, 0.5, 0.25, 0.125 -> 0, 1, 2, 3."""
    try:
        return RELAXATIONS[float(relaxation)]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"relaxation must be one of {sorted(RELAXATIONS, reverse=True)}, not {relaxation!r}") from None


def check_arguments(iterations, mu_roots, threshold, scale_log2):
    """The scalar arguments photon_piv_volume_mart refuses, as a ValueError."""
    if int(iterations) < 1:
        raise ValueError(f"iterations must be >= 1, not {iterations}")
    if not 0 <= int(mu_roots) <= MAX_MU_ROOTS:
        raise ValueError(f"mu_roots must be within [0, {MAX_MU_ROOTS}], not {mu_roots}")
    if not (np.isfinite(threshold) and float(threshold) >= 0):
        raise ValueError(f"threshold must be finite and >= 0, not {threshold}")
    check_scale(scale_log2)


def check_scale(scale_log2):
    if not SCALE_LOG2_RANGE[0] <= int(scale_log2) <= SCALE_LOG2_RANGE[1]:
        raise ValueError(f"scale_log2 must be within [{SCALE_LOG2_RANGE[0]}, {SCALE_LOG2_RANGE[1]}], not {scale_log2}")


def _maximum(frames) -> float:
    m = 0.0
    for f in frames:
        a = np.asarray(f, np.float64)
        if a.size:
            m = max(m, float(np.nanmax(np.where(np.isfinite(a), a, 0.0))))
    return m


def scale_log2_for(frames) -> int:
    """The drivers' scale: the largest s with 4 max(frames) 2^s <= 2^31, within the range the call accepts (0 for frames
    without a positive finite value).  frames: one array or a list of arrays."""
    m = _maximum(frames if isinstance(frames, (list, tuple)) else [frames])
    if not m > 0:
        return 0
    mant, e = np.frexp(m)                               # m = mant 2^e, mant in [0.5, 1)
    s = 29 - int(e) + (1 if mant == 0.5 else 0)
    return int(min(max(s, SCALE_LOG2_RANGE[0]), SCALE_LOG2_RANGE[1]))


def default_threshold(frames) -> float:
    """The drivers' threshold: DEFAULT_THRESHOLD of the largest finite value of the frames, as an f32."""
    return float(np.float32(DEFAULT_THRESHOLD * _maximum(frames if isinstance(frames, (list, tuple)) else [frames])))


# ---- the re-projection ---------------------------------------------------------------------------------------------------------
def quantise(p, scale_log2: int) -> np.ndarray:
    """One contribution in fixed point: llrint(min(f64(p) 2^s, 2^31)) as int64; what is not above 0 (a NaN included: an
    infinite voxel under a zero weight) is 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(p).astype(np.float64) * np.ldexp(1.0, int(scale_log2))
        return np.where(t >= CAP, CAP, np.where(t > 0, np.rint(t), 0.0)).astype(np.int64)


def images_of(acc, scale_log2: int) -> np.ndarray:
    """The accumulators as images: f32(f64(acc) 2^-s)."""
    with np.errstate(over="ignore"):
        return (np.asarray(acc, np.int64).astype(np.float64) * np.ldexp(1.0, -int(scale_log2))).astype(np.float32)


def _volumes(volumes, dtype):
    v = np.asarray(volumes, dtype)
    if v.ndim not in (3, 4):
        raise ValueError("volumes must be [nz, ny, nx] or [n, nz, ny, nx]")
    return v.reshape((-1,) + v.shape[-3:]), v.ndim == 3


def _project_exact(E, fp, n_pixels, scale_log2, order=None):
    """int64 [n_pixels]: one volume f32 [nz, ny, nx] on one camera."""
    inside, index, weights = fp
    live = np.flatnonzero((E > 0) & inside)
    if order is not None:
        live = live[order(len(live))]
    acc = np.zeros(n_pixels, np.int64)
    e = E.reshape(-1)[live]
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(4):
            np.add.at(acc, index[t].reshape(-1)[live], quantise(weights[t].reshape(-1)[live] * e, scale_log2))
    return acc


def project_model(volumes, poly, grids, sensor_shapes, scale_log2: int, order=None):
    """Host model of photon_piv_volume_project, exact.  volumes f32 [n, nz, ny, nx] (or [nz, ny, nx]); poly, grids from
    piv_tomo.los_coefficients; sensor_shapes: (height, width) per camera.  Every voxel with E > 0 that camera c sees adds
    quantise(w E) -- the product in f32 -- to each of its four taps.  order: a callable n -> a permutation of range(n), the
    order in which the n contributing voxels are added: the integers do not depend on it.  Returns per camera int64 [n,
    height, width] ([height, width] for one volume)."""
    check_scale(scale_log2)
    v, single = _volumes(volumes, np.float32)
    out = []
    for c, (h, w) in enumerate(sensor_shapes):
        fp = volume_footprint(poly[c], grids[c], v.shape[1:], (h, w))
        acc = np.stack([_project_exact(E, fp, int(h) * int(w), scale_log2, order).reshape(int(h), int(w)) for E in v])
        out.append(acc[0] if single else acc)
    return out


# ---- MART ------------------------------------------------------------------------------------------------------------------------
def _gather(img, index, weights, sel):
    t = [weights[k][sel] * img[index[k][sel]] for k in range(4)]
    return ((t[0] + t[1]) + t[2]) + t[3]


def _mart(frames, volumes, poly, grids, iterations, mu_roots, threshold, scale_log2, mask, exact, each=None):
    dtype = np.float32 if exact else np.float64
    check_arguments(iterations, mu_roots, threshold, scale_log2 if exact else 0)
    v, single = _volumes(volumes, dtype)
    v = v.copy()
    n, shape = v.shape[0], v.shape[1:]
    stacks = [ps._stack(f, dtype)[0] for f in frames]
    if not 2 <= len(stacks) <= MAX_CAMERAS or len(poly) != len(stacks) or any(s.shape[0] != n for s in stacks):
        raise ValueError(f"MART takes 2 to {MAX_CAMERAS} cameras and one frame per camera and volume")
    masked = np.zeros(shape, bool) if mask is None else np.asarray(mask).reshape(shape) != 0
    fps = [volume_footprint(poly[c], grids[c], shape, s.shape[1:], dtype) for c, s in enumerate(stacks)]
    thr, zero = dtype(threshold), dtype(0)
    for it in range(int(iterations)):
        for c, s in enumerate(stacks):
            inside, index, weights = fps[c]
            n_pixels = s.shape[1] * s.shape[2]
            for f in range(n):
                E = v[f]
                live = E > 0
                if exact:
                    P = images_of(_project_exact(E, fps[c], n_pixels, scale_log2), scale_log2)
                else:
                    sel = live & inside
                    P = np.zeros(n_pixels)
                    for t in range(4):
                        P += np.bincount(index[t][sel], weights[t][sel] * E[sel], n_pixels)
                img = s[f].reshape(-1)
                img = np.where(img > 0, img, zero)
                E[live & (~inside | masked)] = zero
                sel = live & inside & ~masked
                with np.errstate(all="ignore"):
                    i_bar, p_bar = _gather(img, index, weights, sel), _gather(P, index, weights, sel)
                    ok = p_bar > 0
                    r = i_bar / np.where(ok, p_bar, dtype(1))
                    for _ in range(int(mu_roots)):
                        r = np.sqrt(r)
                    new = np.where(ok, E[sel] * r, E[sel])
                    E[sel] = np.where(new < thr, zero, new)
        if each is not None:
            each(it, v)
    return v[0] if single else v


def mart_model_f32(frames, volumes, poly, grids, iterations: int, mu_roots: int, threshold: float, scale_log2: int, mask=None):
    """Host model of photon_piv_volume_mart in the kernel's own operations.  frames: per camera the raw frames f32 [n, height,
    width] (or [height, width]); volumes f32 [n, nz, ny, nx] (or [nz, ny, nx]), the first guess (not written); poly, grids
    from piv_tomo.los_coefficients; mask [nz, ny, nx], nonzero = the voxel stays 0, or None.  Per iteration and camera, in
    camera order: the exact re-projection of the current volume on that camera (project_model, images_of), then for every
    voxel with E > 0: 0 where the camera does not see it or the mask is set; otherwise the frame clamped at 0 and the
    re-projection gathered at the four taps in f32, ((w0 a0 + w1 a1) + w2 a2) + w3 a3; where the gathered re-projection is
    above 0 the ratio, `mu_roots` square roots and the product with E; then what is below `threshold` becomes 0.  Voxels
    that are not above 0 (zeros, negatives, NaN) are left as they are.  The device returns these bits."""
    return _mart(frames, volumes, poly, grids, iterations, mu_roots, np.float32(threshold), scale_log2, mask, True)


def mart_model(frames, volumes, poly, grids, iterations: int, mu_roots: int, threshold: float, mask=None, each=None):
    """The same algorithm in f64 throughout and without the quantisation.  each(iteration, volumes): called after every
    iteration with the current volumes (read them, do not keep them)."""
    return _mart(frames, volumes, poly, grids, iterations, mu_roots, threshold, 0, mask, False, each)


# ---- the drivers' chains in f64 --------------------------------------------------------------------------------------------------
def reconstruct_model(camera_frames, cameras, vol, iterations: int = 5, relaxation: float = 0.5, threshold=None, each=None):
    """Host model of PhotonLibrary.reconstruct_volume(method="mart") in f64: piv_tomo.los_model in mode "min", then mart_model
    on the frames themselves.  Returns (volumes f64 [n, nz, ny, nx], the line-of-sight volumes, mask u8 [nz, ny, nx])."""
    roots = mu_roots_of(relaxation)
    poly, grids = pt.los_coefficients(cameras, vol)
    first, mask = pt.los_model(camera_frames, poly, grids, pt.shape_of(vol), "min")
    thr = default_threshold(list(camera_frames)) if threshold is None else float(threshold)
    return mart_model(camera_frames, first, poly, grids, iterations, roots, thr, mask, each), first, mask


def mart_tomo_model(camera_frames, cameras, vol, win: int = 32, step: int = 16, radius: int = 4, win_z=None, step_z=None, radius_z=None,
                    iterations: int = 5, relaxation: float = 0.5, threshold=None, offsets=None, volumes=None):
    """Host model of PhotonLibrary.correlate_tomo(reconstruction="mart") in f64: reconstruct_model on the two exposures of every
    camera, then piv_tomo.correlate_volume_model.  volumes: reconstruct_model's result, where the caller has it already.
    Returns what piv_tomo.correlate_tomo_model returns."""
    win_z, step_z, radius_z = pt.z_defaults(vol, win, radius, win_z, step_z, radius_z)
    pt.check_arguments(pt.shape_of(vol), win, step, radius, win_z, step_z, radius_z)
    E, _, mask = reconstruct_model(camera_frames, cameras, vol, iterations, relaxation, threshold) if volumes is None else volumes
    if E.shape[0] != 2:
        raise ValueError("correlate_tomo takes the two exposures of each camera, [2, height, width]")
    vectors, flags = pt.correlate_volume_model(E[0], E[1], win, step, radius, win_z, step_z, radius_z, offsets)
    return vol["pitch"] * vectors[..., :3], vectors, flags, pt.windows_touching(mask, win, step, win_z, step_z)


# ---- the synthetic cases of the tests and of tools/piv_tomo.py --mart -------------------------------------------------------------
CASES = {**{name: dict(case, margin=4.0) for name, case in pt.CASES.items()},
         "uniform_inside": dict(pt.CASES["uniform"], margin=0.0)}         # every particle inside the volume
INTERIOR_MARGIN = (4, 8, 8)                                               # (z, y, x) voxels


def case_inputs(name: str, seed: int = 0):
    """piv_tomo.case_inputs for CASES[name]: (frames per camera f32 [2, 96, 96], the fitted cameras, CASE_VOLUME, the
    particles)."""
    case = CASES[name]
    views = pt.calibrated_views(case["angles"])
    frames, particles = pt.particle_volume_pair([v[0] for v in views], case["flow"], pt.CASE_VOLUME, 1000 + seed, shape=pt.CASE_SENSOR,
                                                ppp=pt.CASE_PPP, margin=case["margin"])
    return frames, tuple(v[1] for v in views), pt.CASE_VOLUME, particles


def case_figures(name: str, displacements):
    """piv_tomo.case_figures for CASES[name]."""
    g = pt.CASE_GRID
    truth = CASES[name]["flow"](pt.window_centres(pt.CASE_VOLUME, g["win"], g["step"], g["win_z"], g["step_z"]))
    err = ((np.asarray(displacements) - truth) / pt.CASE_VOLUME["pitch"])[pt.interior(truth.shape[:3])]
    return np.sqrt(np.mean(err ** 2, axis=(0, 1, 2))), int(err[..., 0].size)


def interior_quality(E, truth) -> float:
    """piv_tomo.quality on the volume less INTERIOR_MARGIN voxels on every side: 4 in z, 8 in y and x."""
    mz, my, mx = INTERIOR_MARGIN
    inner = (slice(mz, -mz), slice(my, -my), slice(mx, -mx))
    return pt.quality(np.asarray(E)[inner], np.asarray(truth)[inner])
