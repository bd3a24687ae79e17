"""Iterative image-deformation correlation (pure numpy: usable without a GPU).

The device forms are photon_piv_bspline_coefficients, photon_piv_deform and photon_piv_validate
(include/parallel_ray_tracing.h, section 7; ``PhotonLibrary.bspline_coefficients`` / ``piv_deform`` / ``piv_validate`` on raw
device pointers, ``PhotonLibrary.correlate_deform`` on arrays).  This module holds their f64 host models, one function per
entry point, and the model of the driver:

* ``bspline_coefficients_model``: the cubic B-spline coefficient image with whole-sample mirror boundaries;
* ``dense_field``, ``deform_model`` and ``deform_dense_model``: the grid's vectors interpolated to every pixel, and the image
  warped by them or by any per-pixel field;
* ``validate_model``: total, normalised median test, replacement, status and the smoothed predictor, in the operation
  order of section 7c (the device returns its f32 outputs bit for bit);
* ``correlate_deform_model``: the driver on ``piv_correlation.correlate_model``.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc

FLAG_REPLACED = 8           # validate: the vector was an outlier of the median test and took its neighbours' median
POLE = np.sqrt(3.0) - 2.0
MAX_SHIFT = float(2 ** 24)


def mirror_index(i, n: int) -> np.ndarray:
    """Whole-sample mirror of any integer index into [0, n): ... 2 1 | 0 1 2 ... n-2 n-1 | n-2 n-3 ..."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    m = np.mod(i, period)
    return np.where(m < n, m, period - m)


def _filter_axis(a: np.ndarray, axis: int, radius: int) -> np.ndarray:
    n = a.shape[axis]
    out = np.sqrt(3.0) * a
    for j in range(1, radius + 1):
        out = out + np.sqrt(3.0) * POLE ** j * (np.take(a, mirror_index(np.arange(n) - j, n), axis=axis) +
                                                np.take(a, mirror_index(np.arange(n) + j, n), axis=axis))
    return out


def bspline_coefficients_model(im, radius: int = 48) -> np.ndarray:
    """Cubic B-spline coefficients of an image [height, width] in f64, such that the spline interpolates the image at the
    pixel centres: c = h * (h * im) along the columns and the rows of the mirrored image, h[j] = sqrt(3) z^|j|, z = sqrt(3) - 2,
    summed to |j| <= radius (z^48 = 4e-28)."""
    a = np.asarray(im, np.float64)
    if a.ndim != 2:
        raise ValueError("the image must be a 2-d array")
    return _filter_axis(_filter_axis(a, 1, int(radius)), 0, int(radius))


def _clean_field(field) -> np.ndarray:
    f = np.array(np.asarray(field, np.float64)[..., :2])
    f[~np.isfinite(f).all(axis=-1)] = 0.0
    return f


def _grid_weights(n_pix: int, win: int, step: int, n: int):
    f = np.clip((np.arange(n_pix, dtype=np.float64) - (win - 1) / 2.0) / step, 0.0, n - 1.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), max(n - 2, 0))
    return i0, np.minimum(i0 + 1, n - 1), f - i0


def dense_field(field, shape, win: int, step: int) -> np.ndarray:
    """The grid's vectors [n_rows, n_cols, >= 2] (dx, dy first) at every pixel of an image of `shape`: bilinear in the
    window-centre coordinates of section 5, constant beyond the outermost centres; a vector that is not finite reads as
    (0, 0).  Returns [height, width, 2] f64."""
    h, w = (int(v) for v in shape)
    f = _clean_field(field)
    n_rows, n_cols = f.shape[:2]
    if (n_rows, n_cols) != pc.grid_shape((h, w), win, step):
        raise ValueError(f"a {n_rows} x {n_cols} field is not the grid of a {h} x {w} image, win {win}, step {step}")
    i0, i1, wy = _grid_weights(h, int(win), int(step), n_rows)
    j0, j1, wx = _grid_weights(w, int(win), int(step), n_cols)
    wx, wy = wx[None, :, None], wy[:, None, None]
    t = f[i0][:, j0] + wx * (f[i0][:, j1] - f[i0][:, j0])
    u = f[i1][:, j0] + wx * (f[i1][:, j1] - f[i1][:, j0])
    return t + wy * (u - t)


def _bspline_weights(t):
    u = 1.0 - t
    return np.stack([u * u * u, 4.0 - 3.0 * t * t * (2.0 - t), 4.0 - 3.0 * u * u * (2.0 - u), t * t * t]) / 6.0


def deform_dense_model(coef, dense, scale: float) -> np.ndarray:
    """Host model of photon_piv_deform_dense in f64: out(r, q) = S(r + scale Dy, q + scale Dx), S the cubic B-spline of the
    coefficient image `coef`, D = dense[r, q] = (Dx, Dy) given per pixel, [height, width, 2]."""
    c = np.asarray(coef, np.float64)
    h, w = c.shape
    d = np.asarray(dense, np.float64)
    if d.shape != (h, w, 2):
        raise ValueError(f"the dense field must be [{h}, {w}, 2], not {d.shape}")
    s = np.clip(float(scale) * d, -MAX_SHIFT, MAX_SHIFT)
    fl = np.floor(s)
    wx, wy = _bspline_weights(s[..., 0] - fl[..., 0]), _bspline_weights(s[..., 1] - fl[..., 1])
    bx = np.arange(w)[None, :] + fl[..., 0].astype(np.int64) - 1
    by = np.arange(h)[:, None] + fl[..., 1].astype(np.int64) - 1
    out = np.zeros((h, w))
    for u in range(4):
        yi = mirror_index(by + u, h)
        row = np.zeros((h, w))
        for t in range(4):
            row += wx[t] * c[yi, mirror_index(bx + t, w)]
        out += wy[u] * row
    return out


def deform_model(coef, field, win: int, step: int, scale: float) -> np.ndarray:
    """Host model of photon_piv_deform in f64: deform_dense_model with D = dense_field(field)."""
    return deform_dense_model(coef, dense_field(field, np.shape(coef), win, step), scale)


def _median_sorted(v, m):
    """Median of the first m (>= 1) of the values sorted along axis 0: (v[(m-1)/2] + v[m/2]) / 2; NaN where m is 0."""
    lo = np.take_along_axis(v, np.maximum((m - 1) // 2, 0)[None], axis=0)[0]
    hi = np.take_along_axis(v, (m // 2)[None], axis=0)[0]
    with np.errstate(invalid="ignore"):
        return np.where(m > 0, (lo + hi) / 2.0, np.nan)


def _neighbour_median(nb):
    """Per-component median over the neighbours that are not NaN: nb [8, r, c, 2] -> (median [r, c, 2], sorted, count)."""
    m = (~np.isnan(nb)).sum(axis=0)
    srt = np.sort(np.where(np.isnan(nb), np.inf, nb), axis=0)
    return _median_sorted(srt, m), srt, m


def validate_model(pred, vectors, flags, eps: float = 0.1, threshold: float = 2.0):
    """Host model of photon_piv_validate (section 7c).  pred [n_rows, n_cols, 2] or None; vectors [n_rows, n_cols, >= 2];
    flags [n_rows, n_cols].  Returns (field f32 [n_rows, n_cols, 2], smooth f32 [n_rows, n_cols, 2], status int32
    [n_rows, n_cols], outliers bool [n_rows, n_cols], score f64 [n_rows, n_cols]: r_x^2 + r_y^2, NaN where there is
    none)."""
    v = np.asarray(vectors, np.float32).astype(np.float64)[..., :2]
    flags = np.asarray(flags, np.int32)
    eps, threshold = float(eps), float(threshold)
    if not (np.isfinite(eps) and eps >= 0.0) or not (np.isfinite(threshold) and threshold > 0.0):
        raise ValueError("eps must be finite and >= 0, threshold finite and > 0")
    p = 0.0 if pred is None else np.asarray(pred, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (p + v) + 0.0
    t[((flags & pc.FLAG_FLAT) != 0) | ~np.isfinite(t).all(axis=-1)] = np.nan

    nb = pc._neighbours(t)
    med, srt, m = _neighbour_median(nb)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dev = np.sort(np.where(np.isinf(srt), np.inf, np.abs(srt - med[None])), axis=0)
        rm = _median_sorted(dev, m)
        r = np.abs(t - med) / (rm + eps)
        score = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
        outliers = np.isnan(t[..., 0]) | ((m[..., 0] > 0) & (score > threshold * threshold))

    good = np.where(outliers[..., None], np.nan, t)
    repl = np.nan_to_num(_neighbour_median(pc._neighbours(good))[0], nan=0.0)
    out = np.where(outliers[..., None], repl, t)
    status = (flags | np.where(outliers, FLAG_REPLACED, 0)).astype(np.int32)

    e = np.pad(out, ((0, 0), (1, 1), (0, 0)), mode="edge")
    hrow = ((e[:, :-2] + 2.0 * e[:, 1:-1]) + e[:, 2:]) / 4.0
    e = np.pad(hrow, ((1, 1), (0, 0), (0, 0)), mode="edge")
    smooth = ((e[:-2] + 2.0 * e[1:-1]) + e[2:]) / 4.0
    return out.astype(np.float32), smooth.astype(np.float32), status, outliers, score


def model_correlator(method: str, win: int, radius, window_sigma, diameter, mask=None, min_valid_fraction: float = 0.5,
                     weighting=None):
    """What method= selects in the models of the drivers, as library._Correlator does on the device: (correlate(im1, im2,
    win, step, radius) -> (vectors, flags), the radius, check(shape, win, step, radius)).  "direct": piv_correlation's model,
    radius None = win // 2.  "phase": piv_phase.correlate_phase_model in mode 1 (window_sigma None = win / 4; radius None or
    win // 2 = win // 2 - 1).  mask (a plane, or a pair of them for the two frames): piv_mask.correlate_masked_model with
    min_valid = ceil(min_valid_fraction win^2), "direct" alone.  weighting (the drivers' weighting=):
    piv_weighting.correlate_weighted_model with the table piv_weighting.resolve makes of it for `win`, "direct" without a
    mask alone."""
    if weighting is not None:
        from . import piv_weighting
        piv_weighting.check_method(method, weighting, mask)
        table = piv_weighting.resolve(weighting, win)

        def correlate_weighted(a, b, win, step, radius):
            return piv_weighting.correlate_weighted_model(a, b, table, win, step, radius)
        return correlate_weighted, (int(win) // 2 if radius is None else int(radius)), pc.check_arguments
    if mask is not None:
        from . import piv_mask
        piv_mask.check_method(method, mask)
        if method == "direct":
            min_valid = piv_mask.min_valid_for(win, min_valid_fraction)

            def correlate_masked(a, b, win, step, radius):
                m1, m2 = piv_mask.mask_pair(mask, np.shape(a))
                return piv_mask.correlate_masked_model(a, b, m1, m2, win, step, radius, min_valid)
            return correlate_masked, (int(win) // 2 if radius is None else int(radius)), pc.check_arguments
    if method == "direct":
        return pc.correlate_model, (int(win) // 2 if radius is None else int(radius)), pc.check_arguments
    if method != "phase":
        raise ValueError(f'method must be "direct" or "phase", not {method!r}')
    from . import piv_phase as pp
    how = dict(mode=pp.MODE_PHASE, window_sigma=int(win) / 4.0 if window_sigma is None else float(window_sigma), diameter=float(diameter))

    def correlate(a, b, win, step, radius):
        return pp.correlate_phase_model(a, b, win, step, radius, **how)

    def check(shape, win, step, radius):
        pp.check_arguments(shape, win, step, radius, **how)
    return correlate, pp.default_radius(win, radius), check


def correlate_deform_model(im1, im2, win: int = 32, step: int = 16, radius=None, iterations: int = 3, residual_radius: int = 4,
                           smooth: bool = True, eps: float = 0.1, threshold: float = 2.0, history: bool = False, method: str = "direct",
                           window_sigma=None, diameter: float = 2.5, mask=None, min_valid_fraction: float = 0.5,
                           fill_masked: bool = False, weighting=None):
    """Host model of PhotonLibrary.correlate_deform: returns (vectors [n_rows, n_cols, 4] = dx, dy of the last unsmoothed
    field, peak and ratio of the last correlation; status [n_rows, n_cols]); with history=True also the list of the
    unsmoothed fields after pass 0 and after every iteration.  method="phase": every pass correlates with
    piv_phase.correlate_phase_model in mode 1 (window_sigma None = win / 4; radius None or win // 2 = win // 2 - 1).
    mask, min_valid_fraction, fill_masked: as the driver takes them -- every pass correlates with
    piv_mask.correlate_masked_model under the mask in unwarped image coordinates, each frame's masked pixels are at that
    frame's unmasked mean before the coefficients, and piv_mask.fill_masked decides what masked-out nodes return.
    weighting: as the driver takes it -- every pass correlates with piv_weighting.correlate_weighted_model."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    if int(iterations) < 0:
        raise ValueError(f"iterations must be >= 0, not {iterations}")
    correlate, radius, check = model_correlator(method, win, radius, window_sigma, diameter, mask, min_valid_fraction, weighting)
    check(im1.shape, win, step, radius)
    if int(iterations) > 0:
        check(im1.shape, win, step, residual_radius)
    if mask is not None:
        from . import piv_mask
        m1, m2 = piv_mask.mask_pair(mask, im1.shape)
        im1, im2 = piv_mask.replace_masked(im1, m1), piv_mask.replace_masked(im2, m2)
    vec, flg = correlate(im1, im2, win, step, radius)
    field, smoothed, status, _, _ = validate_model(None, vec, flg, eps, threshold)
    fields = [field]
    if int(iterations) > 0:
        c1, c2 = bspline_coefficients_model(im1), bspline_coefficients_model(im2)
    for _ in range(int(iterations)):
        pred = smoothed if smooth else field
        vec, flg = correlate(deform_model(c1, pred, win, step, -0.5), deform_model(c2, pred, win, step, 0.5), win, step, int(residual_radius))
        field, smoothed, status, _, _ = validate_model(pred, vec, flg, eps, threshold)
        fields.append(field)
    vectors = np.concatenate([field.astype(np.float64), vec[..., 2:4]], axis=-1)
    if mask is not None:
        vectors = piv_mask.fill_masked(vectors, status, fill_masked)
    return (vectors, status, fields) if history else (vectors, status)
