"""Windowed FFT correlation of an image pair: circular cross-correlation and robust phase correlation (pure numpy: usable
without a GPU).

The device form is photon_piv_correlate_phase (include/parallel_ray_tracing.h, section 13; ``PhotonLibrary.piv_correlate_phase``
on raw device pointers, ``method="phase"`` of ``PhotonLibrary.correlate`` / ``correlate_deform`` / ``correlation_predictor``).
This module holds

* ``tables``: the twiddle, window and spectral-filter tables, f32 values rounded from f64 -- what photon_piv_phase_tables
  returns;
* ``correlate_phase_model_f32``: section 13 operation by operation in f32, the definition the device matches value for value;
* ``correlate_phase_model``: the mathematical definition in f64 on ``np.fft``;
* ``check_arguments``: the arguments photon_piv_correlate_phase refuses.

Grid, window numbering, offsets, vectors and flags are those of ``piv_correlation`` (section 5); the plane of a window is the
central (2R+1)^2 crop of its circular win x win plane.  Mode 0 is the circular cross-correlation of the mean-subtracted,
weighted windows; mode 1 the phase correlation with the spectral filter of Eckstein & Vlachos (2009) for particles of e^-2
diameter ``diameter``.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc

MODE_CIRCULAR, MODE_PHASE = 0, 1


def check_arguments(shape, win: int, step: int, radius: int, mode: int = MODE_PHASE, window_sigma: float = 0.0, diameter: float = 0.0):
    """The arguments photon_piv_correlate_phase refuses, as a ValueError."""
    pc.check_win(win)
    if not 1 <= int(radius) <= int(win) // 2 - 1:
        raise ValueError(f"radius must lie in [1, win / 2 - 1], not {radius}")
    pc.check_grid(shape, win, step)
    if int(mode) not in (MODE_CIRCULAR, MODE_PHASE):
        raise ValueError(f"mode must be 0 (circular correlation) or 1 (phase correlation), not {mode}")
    for name, v in (("window_sigma", window_sigma), ("diameter", diameter)):
        if not (np.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} must be finite and >= 0, not {v}")


def default_radius(win: int, radius=None) -> int:
    """The drivers' radius for method="phase": None and win / 2 (section 5's default) become win / 2 - 1, the largest
    shift a circular plane tells from its negative."""
    return int(win) // 2 - 1 if radius is None or int(radius) == int(win) // 2 else int(radius)


def tables(win: int, window_sigma: float, diameter: float):
    """(twiddles f32 [win/2, 2], window f32 [win], filter f32 [win]), each value f64 rounded once to f32:
    twiddles[k] = (cos, -sin)(2 pi k / win), the quarter turns exactly (1, 0) and (0, -1);
    window[p] = exp(-(p - (win-1)/2)^2 / (2 sigma^2)), all 1 for sigma 0;
    filter[k] = exp(-(d^2 / 16) (2 pi f / win)^2), f = k below win/2 and k - win from there on, all 1 for d 0.
    window_sigma and diameter are taken at their f32 values, as the C entry point receives them."""
    win = int(win)
    s, d = float(np.float32(window_sigma)), float(np.float32(diameter))
    k = np.arange(win // 2, dtype=np.float64)
    ang = 2.0 * np.pi * k / win
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    tw[0] = (1.0, 0.0)
    tw[win // 4] = (0.0, -1.0)
    c = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    window = np.exp(-(c * c) / (2.0 * s * s)) if s > 0.0 else np.ones(win)
    f = np.arange(win, dtype=np.float64)
    f = np.where(f < win // 2, f, f - win)
    u = 2.0 * np.pi * f / win
    filt = np.exp(-(d * d / 16.0) * (u * u))
    return tw.astype(np.float32), window.astype(np.float32), filt.astype(np.float32)


def filter_sum(filt) -> float:
    """sum W over the bins that contribute, as section 13 takes it: (sum_k filter[k])^2 - 1, the sum in f64 in the order of
    k; the 1 is W(0, 0), the bin of the mean."""
    s = 0.0
    for v in np.asarray(filt):
        s += float(v)
    return s * s - 1.0


def bit_reverse(n: int) -> np.ndarray:
    """The bit-reversal permutation of range(n), n a power of two."""
    bits = int(n).bit_length() - 1
    i = np.arange(n)
    out = np.zeros(n, np.int64)
    for b in range(bits):
        out |= ((i >> b) & 1) << (bits - 1 - b)
    return out


def _windows(im1, im2, win, step, offset):
    """Window pixels of both frames [n, win, win] (im2 at the offset, clipped into the image), the in-image mask of im2's,
    and the offsets."""
    H, W = im1.shape
    n_rows, n_cols = pc.grid_shape(im1.shape, win, step)
    n = n_rows * n_cols
    k = np.arange(n)
    wy0, wx0 = (k // n_cols) * step, (k % n_cols) * step
    if offset is None:
        ox = oy = np.zeros(n, np.int64)
    else:
        o = np.asarray(offset).reshape(n, 2).astype(np.int64)
        ox, oy = o[:, 0], o[:, 1]
    iw = np.arange(win)
    a = im1[(wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :]]
    gy, gx = wy0[:, None] + oy[:, None] + iw, wx0[:, None] + ox[:, None] + iw
    inside = ((gy >= 0) & (gy < H))[:, :, None] & ((gx >= 0) & (gx < W))[:, None, :]
    b = im2[np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :]]
    return a, b, inside, ox, oy, (n_rows, n_cols)


def _flat_by_pixels(a, b, inside):
    """Section 5's rule from the smallest and the largest pixel: all of a equal, or all (or none) of b's in-image pixels."""
    cnt = inside.sum(axis=(1, 2))
    b_lo = np.where(inside, b, np.inf).min(axis=(1, 2))
    b_hi = np.where(inside, b, -np.inf).max(axis=(1, 2))
    return (a.min(axis=(1, 2)) == a.max(axis=(1, 2))) | (cnt == 0) | (b_lo == b_hi)


def _crop(P, R):
    """The central (2R+1)^2 crop of circular planes [n, win, win]: shift s at index s mod win."""
    idx = np.arange(-R, R + 1) % P.shape[-1]
    return P[:, idx][:, :, idx]


# ---- the f64 definition ------------------------------------------------------------------------------------------------
def correlate_phase_model(im1, im2, win: int, step: int, radius: int, offset=None, mode: int = MODE_PHASE, window_sigma: float = 0.0,
                          diameter: float = 0.0, planes: bool = False):
    """The mathematical definition of section 13 in f64 on np.fft.  Arguments and results as piv_correlation.correlate_model
    takes and returns them; mode, window_sigma and diameter as photon_piv_correlate_phase."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d arrays of one shape")
    win, step, R, mode = int(win), int(step), int(radius), int(mode)
    check_arguments(im1.shape, win, step, R, mode, window_sigma, diameter)
    a, b, inside, ox, oy, grid = _windows(im1, im2, win, step, offset)
    flat = _flat_by_pixels(a, b, inside)
    cnt = inside.sum(axis=(1, 2))
    mean_b = np.where(inside, b, 0.0).sum(axis=(1, 2)) / np.maximum(cnt, 1)
    c = np.arange(win) - (win - 1) / 2.0
    g = np.exp(-(c * c) / (2.0 * float(window_sigma) ** 2)) if float(window_sigma) > 0.0 else np.ones(win)
    g2 = g[:, None] * g[None, :]
    a = (a - a.mean(axis=(1, 2))[:, None, None]) * g2
    b = np.where(inside, b - mean_b[:, None, None], 0.0) * g2
    S = np.conj(np.fft.fft2(a)) * np.fft.fft2(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == MODE_CIRCULAR:
            C = np.fft.ifft2(S).real
            norm = 1.0 / np.sqrt((a * a).sum(axis=(1, 2)) * (b * b).sum(axis=(1, 2)))
        else:
            f = np.fft.fftfreq(win) * win
            w = np.exp(-(float(diameter) ** 2 / 16.0) * (2.0 * np.pi * f / win) ** 2)
            Wt = w[:, None] * w[None, :]
            Wt[0, 0] = 0.0                                         # the mean's bin holds rounding only: it has no phase
            mag = np.abs(S)
            C = np.fft.ifft2(np.where(mag > 0.0, Wt * S / np.where(mag > 0.0, mag, 1.0), 0.0)).real * float(win * win)
            norm = np.full(len(a), 1.0 / Wt.sum())
    flat = flat | ~np.isfinite(norm)
    outside = ~inside.all(axis=(1, 2))
    return pc.peak_outputs(_crop(C, R), R, ox, oy, norm, flat, outside, grid, planes)


# ---- the f32 definition, operation by operation ------------------------------------------------------------------------
def _rows_then_tree(v):
    """Section 13's sum of [n, win, win] f32 values: every row from its first column on, then the win row sums by halving
    (row i + row i + h for h = win/2 ... 1)."""
    acc = np.zeros(v.shape[:2], np.float32)
    for x in range(v.shape[2]):
        acc = acc + v[:, :, x]
    h = v.shape[1] // 2
    while h >= 1:
        acc = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return acc[:, 0]


def _butterflies(re, im, twr, twi, inverse: bool):
    """Radix-2 transform along the last axis in f32, every multiply and add rounded on its own.  Forward: decimation in
    frequency, natural order in, bit-reversed order out, (u, v) -> (u + v, (u - v) w).  Inverse: decimation in time,
    bit-reversed in, natural out, conjugate twiddles, (u, v) -> (u + v w, u - v w); no 1 / n."""
    shape, n = re.shape, re.shape[-1]
    halves = []
    h = n // 2
    while h >= 1:
        halves.append(h)
        h //= 2
    for h in (reversed(halves) if inverse else halves):
        j = np.arange(h) * (n // (2 * h))
        wr, wi = twr[j], (-twi[j] if inverse else twi[j])
        r, i = re.reshape(shape[:-1] + (n // (2 * h), 2, h)), im.reshape(shape[:-1] + (n // (2 * h), 2, h))
        ur, ui, vr, vi = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        if inverse:
            tr, ti = vr * wr - vi * wi, vr * wi + vi * wr
            re, im = np.stack([ur + tr, ur - tr], axis=-2), np.stack([ui + ti, ui - ti], axis=-2)
        else:
            dr, di = ur - vr, ui - vi
            re, im = np.stack([ur + vr, dr * wr - di * wi], axis=-2), np.stack([ui + vi, dr * wi + di * wr], axis=-2)
        re, im = re.reshape(shape), im.reshape(shape)
    return re, im


def _along_columns(re, im, twr, twi, inverse):
    re, im = _butterflies(np.swapaxes(re, -1, -2), np.swapaxes(im, -1, -2), twr, twi, inverse)
    return np.swapaxes(re, -1, -2), np.swapaxes(im, -1, -2)


def correlate_phase_model_f32(im1, im2, win: int, step: int, radius: int, offset=None, mode: int = MODE_PHASE,
                              window_sigma: float = 0.0, diameter: float = 0.0, planes: bool = False, tabs=None, details: bool = False):
    """Section 13 in the device's f32 operations and order: the planes, peaks and ratios photon_piv_correlate_phase returns,
    value for value, and its dx, dy up to the f64 logarithm of the fit.  Returns (vectors f32 [n_rows, n_cols, 4], flags)
    and with planes=True the planes f32 [n_rows, n_cols, 2R+1, 2R+1]; tabs: the tables to use instead of ``tables``'s;
    details=True appends a dict with the number of bins of each window other than (0, 0) whose |S| is 0 ("zero_bins")."""
    im1, im2 = np.asarray(im1, np.float32), np.asarray(im2, np.float32)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d arrays of one shape")
    win, step, R, mode = int(win), int(step), int(radius), int(mode)
    check_arguments(im1.shape, win, step, R, mode, window_sigma, diameter)
    tw, g, w = tables(win, window_sigma, diameter) if tabs is None else tabs
    twr, twi = np.ascontiguousarray(tw[:, 0]), np.ascontiguousarray(tw[:, 1])
    a, b, inside, ox, oy, grid = _windows(im1, im2, win, step, offset)
    flat = _flat_by_pixels(a, b, inside)
    zero = np.float32(0.0)
    b = np.where(inside, b, zero)

    # means: a over win^2; b over its in-image pixels (the others add 0 to the sum and read as the mean)
    cnt = inside.sum(axis=(1, 2)).astype(np.float32)
    mean_a = _rows_then_tree(a) / np.float32(win * win)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_b = np.where(cnt > 0, _rows_then_tree(b) / np.where(cnt > 0, cnt, np.float32(1.0)), zero)
    a = ((a - mean_a[:, None, None]) * g[None, :, None]) * g[None, None, :]
    b = (np.where(inside, b - mean_b[:, None, None], zero) * g[None, :, None]) * g[None, None, :]
    ea, eb = _rows_then_tree(a * a), _rows_then_tree(b * b)
    flat = flat | ~(ea > 0) | ~(eb > 0)

    # Z = DFT(a + i b), rows then columns; both axes come out in bit-reversed order
    zr, zi = _butterflies(a, b, twr, twi, False)
    zr, zi = _along_columns(zr, zi, twr, twi, False)
    rev = bit_reverse(win)
    zr, zi = zr[:, rev][:, :, rev], zi[:, rev][:, :, rev]                 # natural order (the device works in place)
    neg = (-np.arange(win)) % win
    mr, mi = zr[:, neg][:, :, neg], zi[:, neg][:, :, neg]                 # Z(-k)
    ar, ai, br, bi = zr + mr, zi - mi, zi + mi, mr - zr                   # 2 A, 2 B
    sr, si = ar * br + ai * bi, ar * bi - ai * br                         # 4 conj(A) B
    zero_bins = np.zeros(len(a), np.int64)
    if mode == MODE_PHASE:
        mag = np.sqrt(sr * sr + si * si)
        ok = mag > 0
        zero_bins = (~ok).sum(axis=(1, 2)) - (~ok[:, 0, 0])
        ok[:, 0, 0] = False                                                # the mean's bin never contributes
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = (w[:, None] * w[None, :])[None] / np.where(ok, mag, np.float32(1.0))
            sr, si = np.where(ok, sr * q, zero), np.where(ok, si * q, zero)
    sr, si = sr[:, rev][:, :, rev], si[:, rev][:, :, rev]                 # back to the storage order
    pr, pi = _along_columns(sr, si, twr, twi, True)
    pr, pi = _butterflies(pr, pi, twr, twi, True)

    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == MODE_CIRCULAR:
            norm = 1.0 / (4.0 * win * win * np.sqrt(ea.astype(np.float64) * eb.astype(np.float64)))
        else:
            norm = np.full(len(a), np.float64(1.0) / np.float64(filter_sum(w)))
    outside = ~inside.all(axis=(1, 2))
    out = pc.peak_outputs(_crop(pr.astype(np.float64), R), R, ox, oy, norm, flat, outside, grid, planes)
    with np.errstate(over="ignore"):
        out = (out[0].astype(np.float32), out[1]) + tuple(p.astype(np.float32) for p in out[2:])
    if details:
        out = out + ({"zero_bins": zero_bins.reshape(grid)},)
    return out


def log_curvature(planes):
    """|ln C- - 2 ln C0 + ln C+| through the integer peak of every plane [..., nS, nS] along (x, y): the denominator of the
    Gaussian fit, which decides how far a last-bit difference of the f64 logarithm moves dx, dy.  +inf where the fit is
    parabolic or the peak lies on the edge."""
    p = np.asarray(planes, np.float64)
    nS = p.shape[-1]
    flatp = p.reshape(-1, nS, nS)
    n = len(flatp)
    out = np.full((n, 2), np.inf)
    for k in range(n):
        c = flatp[k]
        if not np.isfinite(c).all():
            continue
        py, px = np.unravel_index(np.argmax(c), c.shape)
        for axis, tri in enumerate(((c[py, px - 1:px + 2] if 0 < px < nS - 1 else None), (c[py - 1:py + 2, px] if 0 < py < nS - 1 else None))):
            if tri is not None and (tri > 0).all():
                l = np.log(tri)
                out[k, axis] = abs(l[0] - 2.0 * l[1] + l[2])
    return out.reshape(p.shape[:-2] + (2,))
