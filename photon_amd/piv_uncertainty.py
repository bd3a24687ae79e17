"""Displacement uncertainty per vector from correlation statistics (Wieneke 2015; pure numpy: usable without a GPU).

The device form is photon_piv_uncertainty (include/parallel_ray_tracing.h, section 11; ``PhotonLibrary.piv_uncertainty`` on
raw device pointers, ``PhotonLibrary.displacement_uncertainty`` on arrays).  This module holds its f64 host model:

* ``uncertainty_model``: the definition of section 11, sum by sum, on a matched image pair;
* ``sigma_from_stats``: the last step alone -- (sigma, flags) from the four sums (C0, C1, S(0), V) of each axis;
* ``displacement_uncertainty_model``: the driver -- both frames warped half-way by the field (piv_deformation), then
  ``uncertainty_model``.

The method reads the converged pair only.  With both frames warped by the measured field, what is left between them is
noise; the asymmetry of the correlation peak, C(+e) - C(-e) = sum_p d(p), has an expectation of zero, and its variance V
follows from the d(p) themselves, with their spatial covariance out to `reach` pixels.  Pushing C(+-e) apart by +-sqrt(V) / 2
through section 5's three-point fit gives the standard deviation of that fit's peak position.  What it cannot see: bias,
peak locking, the truncation error of a field that varies inside a window.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc
from . import piv_deformation as pd

FLAG_FLAT = pc.FLAG_FLAT        # 2: all pixels of a window of either frame are equal: sigma and stats NaN
FLAG_NO_PEAK = 16               # den <= 0 in an axis: no maximum at zero shift, sigma of that axis NaN
FLAG_NEGATIVE_VARIANCE = 32     # V < 0 (or NaN) in an axis: S(0) stands in for it
MAX_REACH = 4


def check_arguments(shape, win: int, step: int, reach: int):
    """The arguments photon_piv_uncertainty refuses, as a ValueError (null pointers aside)."""
    pc.check_win(win)
    if not 0 <= int(reach) <= MAX_REACH:
        raise ValueError(f"reach must lie in [0, {MAX_REACH}], not {reach}")
    pc.check_grid(shape, win, step)


def half_neighbourhood(reach: int):
    """H_K: the (Dr, Dq) with 0 <= Dr <= K, |Dq| <= K and Dr > 0 or Dq > 0 -- one of every pair +-D."""
    K = int(reach)
    return [(dr, dq) for dr in range(K + 1) for dq in range(-K, K + 1) if dr > 0 or dq > 0]


def _axis_sums(A, B, reach: int):
    """(C0, C1, S00, V, T) of the axis along the last dimension of the windows A, B [..., win, win]."""
    u, v = A[..., :, :-1] * B[..., :, 1:], A[..., :, 1:] * B[..., :, :-1]
    d = u - v
    C1 = 0.5 * (u + v).sum(axis=(-2, -1))
    C0 = 0.5 * (A[..., :, :-1] * B[..., :, :-1] + A[..., :, 1:] * B[..., :, 1:]).sum(axis=(-2, -1))
    T = ((np.abs(u) + np.abs(v)) ** 2).sum(axis=(-2, -1))
    S00 = (d * d).sum(axis=(-2, -1))
    V = S00.copy()
    nr, nq = d.shape[-2:]
    for dr, dq in half_neighbourhood(reach):
        if dr >= nr or abs(dq) >= nq:
            continue
        q0, q1 = max(0, -dq), nq - max(0, dq)
        V = V + 2.0 * (d[..., :nr - dr, q0:q1] * d[..., dr:, q0 + dq:q1 + dq]).sum(axis=(-2, -1))
    return C0, C1, S00, V, T


def sigma_from_stats(stats):
    """The last step of section 11: stats [..., 2, 4] = (C0, C1, S(0), V) per axis -> (sigma f64 [..., 2], flags int32
    [...]).  A window whose stats are NaN is flat: flag 2, sigma NaN."""
    st = np.asarray(stats, np.float64)
    C0, C1, S00, V = (st[..., k] for k in range(4))
    flat = np.isnan(C0).any(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        negative = ~(V >= 0.0)
        s = np.sqrt(np.where(negative, S00, V))
        lo, hi = C1 - s / 2.0, C1 + s / 2.0
        gauss = (lo > 0.0) & (C0 > 0.0)
        l0, llo, lhi = (np.log(np.where(gauss, x, 1.0)) for x in (C0, lo, hi))
        num = np.where(gauss, lhi - llo, hi - lo)
        den = np.where(gauss, (4.0 * l0 - 2.0 * llo) - 2.0 * lhi, 4.0 * (C0 - C1))
        peak = den > 0.0
        sigma = np.where(peak, num / np.where(peak, den, 1.0), np.nan)
    flags = np.where((negative & ~flat[..., None]).any(axis=-1), FLAG_NEGATIVE_VARIANCE, 0) \
        | np.where((~peak & ~flat[..., None]).any(axis=-1), FLAG_NO_PEAK, 0)
    flags = np.where(flat, FLAG_FLAT, flags).astype(np.int32)
    sigma[flat] = np.nan
    return sigma, flags


def uncertainty_model(im1, im2, win: int, step: int, reach: int):
    """Host model of photon_piv_uncertainty in f64 on a matched pair [height, width].  Returns (sigma [n_rows, n_cols, 2]
    = (sigma_x, sigma_y) px, flags int32 [n_rows, n_cols], stats [n_rows, n_cols, 2, 4] = (C0, C1, S(0), V) per axis with V
    as summed, T [n_rows, n_cols, 2]: the rounding scale sum_P (|A(p) B(p+e)| + |A(p+e) B(p)|)^2 of S and V)."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d images of one shape")
    check_arguments(im1.shape, win, step, reach)
    win, step = int(win), int(step)
    a, b = (np.lib.stride_tricks.sliding_window_view(im, (win, win))[::step, ::step] for im in (im1, im2))
    flat = (a.min(axis=(-2, -1)) == a.max(axis=(-2, -1))) | (b.min(axis=(-2, -1)) == b.max(axis=(-2, -1)))
    A = a - a.mean(axis=(-2, -1), keepdims=True)
    B = b - b.mean(axis=(-2, -1), keepdims=True)
    x = _axis_sums(A, B, reach)
    y = _axis_sums(np.swapaxes(A, -2, -1), np.swapaxes(B, -2, -1), reach)      # rows and columns swap roles
    stats = np.stack([np.stack(x[:4], axis=-1), np.stack(y[:4], axis=-1)], axis=-2)
    T = np.stack([x[4], y[4]], axis=-1)
    stats[flat] = np.nan
    sigma, flags = sigma_from_stats(stats)
    return sigma, flags, stats, T


def displacement_uncertainty_model(im1, im2, field, win: int = 32, step: int = 16, reach: int = 2):
    """Host model of PhotonLibrary.displacement_uncertainty: the B-spline coefficients of both frames, frame 1 warped by
    -field / 2 and frame 2 by +field / 2 (piv_deformation.deform_model; a vector that is not finite reads as (0, 0)), then
    uncertainty_model on the warped pair.  field [n_rows, n_cols, >= 2] on section 5's grid.  Returns what
    uncertainty_model returns."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    check_arguments(im1.shape, win, step, reach)
    w1 = pd.deform_model(pd.bspline_coefficients_model(im1), field, win, step, -0.5)
    w2 = pd.deform_model(pd.bspline_coefficients_model(im2), field, win, step, 0.5)
    return uncertainty_model(w1, w2, win, step, reach)
