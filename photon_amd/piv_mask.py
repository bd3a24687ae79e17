"""Window correlation with excluded pixels: a model in the test section, a wall, the region outside the laser sheet or the
dot pattern (pure numpy: usable without a GPU).

The device form is photon_piv_correlate_masked (include/parallel_ray_tracing.h, section 17;
``PhotonLibrary.piv_correlate_masked`` on raw device pointers, ``mask=`` on ``PhotonLibrary.correlate``,
``correlate_deform``, ``correlate_multigrid`` and ``correlation_predictor``).  This module holds

* ``correlate_masked_model``: its f64 host model, section 17 on ``piv_correlation.peak_outputs``; with no masked pixel it
  is ``piv_correlation.correlate_model`` bit for bit;
* ``window_valid``: the free pixels of every window and their centroid -- where a partially masked window's vector sits;
* ``mask_pair``, ``min_valid_for``, ``replace_masked``, ``fill_masked``: what the drivers and their models share -- the
  ``mask=`` argument as two bool planes, min_valid from a fraction of the window, a frame with its masked pixels at the mean
  of the others (what the deformation drivers hand to the B-spline prefilter), and the returned field's rule for
  masked-out nodes.

The mask lives in unwarped image coordinates on every iteration and level of the deformation drivers: it does not follow
the warp (known limits).
"""
from __future__ import annotations

import math

import numpy as np

from . import piv_correlation as pc

FLAG_MASKED_OUT = 16        # fewer than min_valid valid pixels in a, or in b at zero shift: every output of the window is NaN
FLAG_PARTIAL = 32           # not masked out, and a masked pixel lies in a's window or in the in-image part of b's search region


def mask_pair(mask, shape):
    """The drivers' mask= as two bool planes of `shape` (height, width): one array [height, width] (any dtype, nonzero =
    excluded) serves both frames, a tuple or list of two serves frame 1 and frame 2."""
    pair = tuple(mask) if isinstance(mask, (tuple, list)) and len(mask) == 2 else (mask, mask)
    out = tuple(np.asarray(m) != 0 for m in pair)
    for m in out:
        if m.shape != tuple(int(v) for v in shape):
            raise ValueError(f"a mask of shape {m.shape} does not cover a {shape[0]} x {shape[1]} image")
    return out


def min_valid_for(win: int, fraction: float) -> int:
    """min_valid = ceil(fraction win^2), fraction in (0, 1]."""
    f = float(fraction)
    if not 0.0 < f <= 1.0:
        raise ValueError(f"min_valid_fraction must lie in (0, 1], not {fraction}")
    return max(1, min(int(win) ** 2, math.ceil(f * int(win) ** 2)))


def check_method(method: str, mask):
    """Masks exist in the direct correlator alone."""
    if mask is not None and method == "phase":
        raise ValueError('mask= needs method="direct": the phase correlator has no masks')


def check_arguments(shape, win: int, step: int, radius: int, min_valid: int):
    """The arguments photon_piv_correlate_masked refuses, as a ValueError."""
    pc.check_arguments(shape, win, step, radius)
    if not 1 <= int(min_valid) <= int(win) ** 2:
        raise ValueError(f"min_valid must lie in [1, win^2], not {min_valid}")


def correlate_masked_model(im1, im2, mask1, mask2, win: int, step: int, radius: int, min_valid: int = 1, offset=None,
                           planes: bool = False, valid: bool = False):
    """Host model of photon_piv_correlate_masked in f64.  im1, im2 [height, width]; mask1, mask2 [height, width] (nonzero =
    excluded) or None; offset as correlate_model takes it.  Returns (vectors [n_rows, n_cols, 4], flags [n_rows, n_cols]
    int32), then the normalised planes with planes=True, then (n_a, n_b) int32 [n_rows, n_cols, 2] with valid=True.
    Flatness is decided as in correlate_model: an f64 energy over the valid pixels that is 0."""
    im1 = np.asarray(im1, np.float64)
    im2 = np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d arrays of one shape")
    win, step, R, min_valid = int(win), int(step), int(radius), int(min_valid)
    check_arguments(im1.shape, win, step, R, min_valid)
    H, W = im1.shape
    m1, m2 = (np.zeros((H, W), bool) if m is None else mask_pair(m, (H, W))[0] for m in (mask1, mask2))
    n_rows, n_cols = pc.grid_shape(im1.shape, win, step)
    n = n_rows * n_cols
    k = np.arange(n)
    wy0, wx0 = (k // n_cols) * step, (k % n_cols) * step
    if offset is None:
        ox = oy = np.zeros(n, np.int64)
    else:
        o = np.asarray(offset).reshape(n, 2).astype(np.int64)
        ox, oy = o[:, 0], o[:, 1]
    span, nS = win + 2 * R, 2 * R + 1
    iw, isp = np.arange(win), np.arange(span)

    # every select below keeps the value under a mask out of the arithmetic: NaN or inf there changes nothing
    ia = ((wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :])
    va = ~m1[ia]
    n_a = va.sum(axis=(1, 2))
    a = np.where(va, im1[ia], 0.0)
    mean_a = a.sum(axis=(1, 2)) / np.maximum(n_a, 1)
    a = np.where(va, a - mean_a[:, None, None], 0.0)
    gy = wy0[:, None] + oy[:, None] - R + isp                     # [n][span]
    gx = wx0[:, None] + ox[:, None] - R + isp
    iny, inx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
    inside = iny[:, :, None] & inx[:, None, :]
    ib = (np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :])
    hidden_b = inside & m2[ib]
    vb = inside & ~hidden_b
    b = np.where(vb, im2[ib], 0.0)
    zero = (slice(None), slice(R, R + win), slice(R, R + win))
    n_b = vb[zero].sum(axis=(1, 2))
    mean_b = np.where(n_b > 0, b[zero].sum(axis=(1, 2)) / np.maximum(n_b, 1), 0.0)
    b = np.where(vb, b - mean_b[:, None, None], 0.0)
    ea = (a * a).sum(axis=(1, 2))
    eb = (b[zero] * b[zero]).sum(axis=(1, 2))

    masked_out = (n_a < min_valid) | (n_b < min_valid)
    partial = ~masked_out & (~va.all(axis=(1, 2)) | hidden_b.any(axis=(1, 2)))
    C = np.empty((n, nS, nS), np.float64)
    for sy in range(nS):
        for sx in range(nS):
            C[:, sy, sx] = np.einsum("nij,nij->n", a, b[:, sy:sy + win, sx:sx + win])
    if partial.any():                                           # the overlap normalisation, on the windows a mask touches
        fa, fb = va[partial].astype(np.float64), vb[partial].astype(np.float64)
        N = np.empty((len(fa), nS, nS), np.float64)
        for sy in range(nS):
            for sx in range(nS):
                N[:, sy, sx] = np.einsum("nij,nij->n", fa, fb[:, sy:sy + win, sx:sx + win])
        na = n_a[partial].astype(np.float64)[:, None, None]
        C[partial] = np.where(2.0 * N >= na, C[partial] * na / np.where(N > 0, N, 1.0), 0.0)

    outside = ~inside.all(axis=(1, 2))
    flat = (ea == 0.0) | (eb == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(ea * eb)
    out = pc.peak_outputs(C, R, ox, oy, norm, flat | masked_out, outside, (n_rows, n_cols), planes)
    flags = out[1].reshape(n)
    flags[masked_out] = FLAG_MASKED_OUT | np.where(outside[masked_out], pc.FLAG_OUTSIDE, 0)
    flags[partial] |= FLAG_PARTIAL
    if valid:
        out = out + (np.stack([n_a, n_b], axis=1).astype(np.int32).reshape(n_rows, n_cols, 2),)
    return out


def window_valid(mask, win: int, step: int):
    """The free pixels of every window of the (win, step) grid on the mask [height, width] (nonzero = excluded): (count
    [n_rows, n_cols] int64, row [n_rows, n_cols] f64, column [n_rows, n_cols] f64), the centroid of the free pixels in index
    coordinates, NaN where a window has none.  A partially masked window measures the displacement of its free pixels: its
    vector sits at this centroid, not at the window's centre."""
    free = np.asarray(mask) == 0
    pc.check_grid(free.shape, win, step)
    w = np.lib.stride_tricks.sliding_window_view(free, (int(win), int(win)))[::int(step), ::int(step)].astype(np.float64)
    count = w.sum(axis=(2, 3))
    n_rows, n_cols = count.shape
    off = np.arange(int(win), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        row = (w.sum(axis=3) * off).sum(axis=2) / count + (np.arange(n_rows) * int(step))[:, None]
        col = (w.sum(axis=2) * off).sum(axis=2) / count + (np.arange(n_cols) * int(step))[None, :]
    return count.astype(np.int64), row, col


def replace_masked(im, mask) -> np.ndarray:
    """The frame with its masked pixels at the mean of the unmasked ones: what the deformation drivers hand to the B-spline
    prefilter and the warps, so that a bright body does not ring into the free pixels and NaNs under the mask stay there."""
    im = np.asarray(im, np.float64)
    m = np.asarray(mask) != 0
    free = np.where(m, 0.0, im)
    return np.where(m, free.sum() / max(int((~m).sum()), 1), im)


def fill_masked(vectors, status, fill: bool = False) -> np.ndarray:
    """The drivers' rule for the nodes with FLAG_MASKED_OUT in `status`, on vectors [n_rows, n_cols, 4].  fill=False: dx, dy,
    peak and ratio are NaN there.  fill=True: dx and dy keep what they hold (the deformation loop leaves the neighbours'
    median) and, where they are not finite (a single correlation pass), take the median of the finite 3 x 3 neighbours, 0
    where there is none; peak and ratio stay as they are."""
    v = np.array(vectors, np.float64)
    out_nodes = (np.asarray(status) & FLAG_MASKED_OUT) != 0
    if not fill:
        v[out_nodes] = np.nan
        return v
    d = v[..., :2]
    bad = out_nodes & ~np.isfinite(d).all(axis=-1)
    if bad.any():
        good = np.where(np.isfinite(d).all(axis=-1)[..., None], d, np.nan)
        with np.testing.suppress_warnings() as sup:
            sup.filter(RuntimeWarning)
            repl = np.nan_to_num(np.nanmedian(pc._neighbours(good), axis=0), nan=0.0)
        d[bad] = repl[bad]
    return v
