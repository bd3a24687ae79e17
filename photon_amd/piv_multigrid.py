"""Multigrid window refinement of image-deformation correlation (pure numpy: usable without a GPU).

Large windows find a shift that small ones cannot see (the search radius is at most win / 2), small windows resolve the
gradients that large ones average away: 64 -> 32 -> 16 in one evaluation.  The device step is photon_piv_regrid
(include/parallel_ray_tracing.h, section 16; ``PhotonLibrary.piv_regrid`` on raw device pointers), the driver is
``PhotonLibrary.correlate_multigrid``.  This module holds their host models:

* ``regrid_model``: section 16 operation by operation in f32 (the device returns its bits);
* ``regrid_model_f64``: the definition written independently, bilinear interpolation in window-centre coordinates;
* ``check_schedule``: the argument rules of the driver, as ``ValueError``s;
* ``correlate_multigrid_model``: the driver on the parts of ``piv_deformation.correlate_deform_model``.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc
from . import piv_deformation as pd

MAX_SIDE = 1 << 22          # num = (dst_win - src_win) + 2 k dst_step stays below 2^24
DEFAULT_SCHEDULE = ((64, 32), (32, 16), (16, 8))
DEFAULT_ITERATIONS = (1, 1, 2)


def _check_grids(field, shape, src, dst):
    """(f [src_rows, src_cols, 2] as given (not cleaned), (h, w), (src_win, src_step), (dst_win, dst_step)) of a regrid
    call, or the ValueError of what photon_piv_regrid refuses."""
    h, w = (int(v) for v in shape)
    (sw, ss), (dw, ds) = (tuple(int(v) for v in g) for g in (src, dst))
    for win, step in ((sw, ss), (dw, ds)):
        pc.check_win(win)
        pc.check_grid((h, w), win, step)
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"the image is larger than 2^22 pixels a side: {w} x {h}")
    f = np.asarray(field)
    if f.ndim != 3 or f.shape[2] < 2 or tuple(f.shape[:2]) != pc.grid_shape((h, w), sw, ss):
        raise ValueError(f"a field of shape {f.shape} is not [n_rows, n_cols, >= 2] on the grid of a {h} x {w} image, win {sw}, step {ss}")
    return f[..., :2], (h, w), (sw, ss), (dw, ds)


def _weights_f32(n_dst: int, dst_win: int, dst_step: int, src_win: int, src_step: int, n: int):
    """Section 16's node indices and weight per destination node of one axis: (i0, i1 int64 [n_dst], w f32 [n_dst])."""
    num = (dst_win - src_win) + 2 * np.arange(n_dst, dtype=np.int64) * dst_step
    den = 2 * src_step
    inv_den = np.float32(1.0) / np.float32(den)
    q = (num.astype(np.float32) * inv_den).astype(np.int64)         # num < 2^24: exact as f32; the cast truncates as C does
    r = num - q * den
    q, r = np.where(r < 0, q - 1, q), np.where(r < 0, r + den, r)
    q, r = np.where(r >= den, q + 1, q), np.where(r >= den, r - den, r)
    w = r.astype(np.float32) * inv_den
    low, high = (num <= 0) | (n == 1), num >= (n - 1) * den
    i0 = np.where(low, 0, np.where(high, n - 1, q))
    i1 = np.where(low, 0, np.where(high, n - 1, q + 1))
    return i0, i1, np.where(low | high, np.float32(0.0), w).astype(np.float32)


def regrid_model(field, shape, src, dst) -> np.ndarray:
    """Host model of photon_piv_regrid, every operation the device's f32 operation (the library is built without fused
    multiply-adds): the field [src_rows, src_cols, >= 2] (dx, dy first) of the grid src = (win, step) on an image of `shape`
    (height, width), at the window centres of the grid dst = (win, step).  Returns f32 [dst_rows, dst_cols, 2]."""
    f, (h, w), (sw, ss), (dw, ds) = _check_grids(field, shape, src, dst)
    f = np.array(f, np.float32)
    f[~np.isfinite(f).all(axis=-1)] = 0.0
    n_rows, n_cols = f.shape[:2]
    d_rows, d_cols = pc.grid_shape((h, w), dw, ds)
    i0, i1, wy = _weights_f32(d_rows, dw, ds, sw, ss, n_rows)
    j0, j1, wx = _weights_f32(d_cols, dw, ds, sw, ss, n_cols)
    wx, wy = wx[None, :, None], wy[:, None, None]
    with np.errstate(over="ignore", invalid="ignore"):
        t = f[i0][:, j0] + wx * (f[i0][:, j1] - f[i0][:, j0])
        u = f[i1][:, j0] + wx * (f[i1][:, j1] - f[i1][:, j0])
        out = t + wy * (u - t)
    assert out.dtype == np.float32
    return out


def regrid_model_f64(field, shape, src, dst) -> np.ndarray:
    """The definition of section 16 in f64, written from the coordinates: bilinear interpolation of the source field between
    its window centres (win - 1) / 2 + i step, at the destination's window centres, constant beyond the outermost source
    centres; a vector that is not finite reads as (0, 0).  Returns f64 [dst_rows, dst_cols, 2]."""
    f, (h, w), (sw, ss), (dw, ds) = _check_grids(field, shape, src, dst)
    f = pd._clean_field(f)
    n_rows, n_cols = f.shape[:2]
    d_rows, d_cols = pc.grid_shape((h, w), dw, ds)

    def axis(n_dst, n):
        centre = (dw - 1) / 2.0 + np.arange(n_dst, dtype=np.float64) * ds
        g = np.clip((centre - (sw - 1) / 2.0) / ss, 0.0, n - 1.0)
        k0 = np.minimum(np.floor(g).astype(np.int64), max(n - 2, 0))
        return k0, np.minimum(k0 + 1, n - 1), g - k0

    i0, i1, wy = axis(d_rows, n_rows)
    j0, j1, wx = axis(d_cols, n_cols)
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = (1.0 - wx) * f[i0][:, j0] + wx * f[i0][:, j1]
    bottom = (1.0 - wx) * f[i1][:, j0] + wx * f[i1][:, j1]
    return (1.0 - wy) * top + wy * bottom


def check_schedule(shape, schedule, iterations, radius, residual_radius, method, window_sigma=None, diameter: float = 2.5):
    """The arguments correlate_multigrid refuses, as a ValueError: an empty schedule, lengths of schedule and iterations
    that differ, iterations[0] < 0 or iterations[l] < 1 after, a (win, step) the correlator of its level refuses for the
    image (an image smaller than the largest window among them), `radius` outside the range of level 0's correlator,
    `residual_radius` outside the range of any level that iterates.  Returns (schedule, iterations) as tuples of ints."""
    try:
        schedule = tuple((int(win), int(step)) for win, step in schedule)
        iterations = tuple(int(n) for n in iterations)
    except (TypeError, ValueError):
        raise ValueError("schedule must be a sequence of (win, step) pairs and iterations a sequence of ints") from None
    if not schedule:
        raise ValueError("the schedule is empty")
    if len(iterations) != len(schedule):
        raise ValueError(f"{len(schedule)} levels but {len(iterations)} iteration counts")
    for level, n in enumerate(iterations):
        if n < (0 if level == 0 else 1):
            raise ValueError(f"iterations[{level}] must be >= {0 if level == 0 else 1}, not {n}")
    shape = tuple(int(v) for v in shape)
    for level, ((win, step), n) in enumerate(zip(schedule, iterations)):
        _, first_radius, check = pd.model_correlator(method, win, radius if level == 0 else None, window_sigma, diameter)
        try:
            if level == 0:
                check(shape, win, step, first_radius)
            if n > 0:
                check(shape, win, step, residual_radius)
        except ValueError as e:
            raise ValueError(f"level {level} (win {win}, step {step}): {e}") from None
    return schedule, iterations


def correlate_multigrid_model(im1, im2, schedule=DEFAULT_SCHEDULE, iterations=DEFAULT_ITERATIONS, radius=None, residual_radius: int = 4,
                              smooth: bool = True, eps: float = 0.1, threshold: float = 2.0, method: str = "direct", window_sigma=None,
                              diameter: float = 2.5, history: bool = False, mask=None, min_valid_fraction: float = 0.5,
                              fill_masked: bool = False, weighting=None):
    """Host model of PhotonLibrary.correlate_multigrid.  Level 0 is correlate_deform_model at schedule[0] with `radius` and
    iterations[0] iterations; level l > 0 takes regrid_model of the previous level's smoothed field (smooth=False: of the
    field itself) as its predictor and runs iterations[l] >= 1 deformation iterations on its own grid with
    `residual_radius`.  Each level has its own correlator (method="phase": window_sigma None = win / 4 of that level).
    Returns (vectors [n_rows, n_cols, 4] = dx, dy of the last unsmoothed field, peak and ratio of the last correlation;
    status [n_rows, n_cols]) on the last level's grid; with history=True also the list of the unsmoothed fields after pass
    0 and after every iteration of every level, each on its level's grid.  mask, min_valid_fraction, fill_masked: as
    correlate_deform_model takes them; every level takes min_valid from its own win.  weighting: as the driver takes it;
    the string forms make one table per level's win, an array has to be [win, win] for every level's win."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    schedule, iterations = check_schedule(im1.shape, schedule, iterations, radius, residual_radius, method, window_sigma, diameter)
    if weighting is not None:
        from . import piv_weighting
        piv_weighting.check_method(method, weighting, mask)
        for win, _ in schedule:
            piv_weighting.resolve(weighting, win)
    if mask is not None:
        from . import piv_mask
        piv_mask.check_method(method, mask)
        m1, m2 = piv_mask.mask_pair(mask, im1.shape)
        im1, im2 = piv_mask.replace_masked(im1, m1), piv_mask.replace_masked(im2, m2)
    fields, coef = [], None
    for level, ((win, step), n) in enumerate(zip(schedule, iterations)):
        correlate, first_radius, _ = pd.model_correlator(method, win, radius if level == 0 else None, window_sigma, diameter, mask,
                                                         min_valid_fraction, weighting)
        if level == 0:
            vec, flg = correlate(im1, im2, win, step, first_radius)
            field, smoothed, status, _, _ = pd.validate_model(None, vec, flg, eps, threshold)
            fields.append(field)
        else:
            field = smoothed = regrid_model(smoothed if smooth else field, im1.shape, schedule[level - 1], (win, step))
        if n > 0 and coef is None:
            coef = pd.bspline_coefficients_model(im1), pd.bspline_coefficients_model(im2)
        for _ in range(n):
            pred = smoothed if smooth else field
            vec, flg = correlate(pd.deform_model(coef[0], pred, win, step, -0.5), pd.deform_model(coef[1], pred, win, step, 0.5), win, step,
                                 int(residual_radius))
            field, smoothed, status, _, _ = pd.validate_model(pred, vec, flg, eps, threshold)
            fields.append(field)
    vectors = np.concatenate([field.astype(np.float64), vec[..., 2:4]], axis=-1)
    if mask is not None:
        vectors = piv_mask.fill_masked(vectors, status, fill_masked)
    return (vectors, status, fields) if history else (vectors, status)
