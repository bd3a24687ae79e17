"""Window weighting in the direct correlator: a Gaussian (or any non-negative) window in place of the top hat (pure numpy:
usable without a GPU).

A top-hat window of `win` pixels answers a displacement of wavelength lambda with sinc(win / lambda): below the window
size the measured field has the wrong sign, and a deformation loop amplifies it (Astarita 2007; Schrijer & Scarano 2008).
A window that falls off towards its edge has a response that stays positive.

The device form is photon_piv_correlate_weighted (include/parallel_ray_tracing.h, section 18;
``PhotonLibrary.piv_correlate_weighted`` on raw device pointers, ``weighting=`` on ``PhotonLibrary.correlate``,
``correlate_deform``, ``correlate_multigrid`` and ``correlation_predictor``).  This module holds

* ``window_weights``: the tables photon_piv_window_weights fills, bit for bit;
* ``check_weights`` and ``resolve``: what the drivers' ``weighting=`` accepts, as one f32 table [win, win] or None;
* ``correlate_weighted_model``: the f64 host model, section 18 on ``piv_correlation.peak_outputs``; with uniform weights it
  is ``piv_correlation.correlate_model`` exactly.

The phase correlator has a window of its own (``window_sigma``, section 13): it multiplies both frames, so the table that
weights a pair of pixels alike has sigma = window_sigma / sqrt(2).
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc

KINDS = {"uniform": 0, "gaussian": 1}       # photon_piv_window_weights' `kind`


def default_sigma(win: int) -> float:
    return int(win) / 4.0


def window_weights(win: int, kind: str = "gaussian", sigma=None) -> np.ndarray:
    """The f32 table [win, win] photon_piv_window_weights fills.  "uniform": ones.  "gaussian": exp(-(cy^2 + cx^2) /
    (2 sigma^2)) with c = index - (win - 1) / 2 and sigma pixels (None = win / 4; rounded to f32 first, as the C helper takes
    it), evaluated in f64 and rounded once."""
    pc.check_win(win)
    win = int(win)
    if kind not in KINDS:
        raise ValueError(f'kind must be "uniform" or "gaussian", not {kind!r}')
    if kind == "uniform":
        return np.ones((win, win), np.float32)
    s = float(np.float32(default_sigma(win) if sigma is None else sigma))
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"sigma must be finite and > 0, not {sigma}")
    c = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    cy, cx = c[:, None], c[None, :]
    return np.exp(-(cy * cy + cx * cx) / (2.0 * s * s)).astype(np.float32)


def check_weights(weight, win: int) -> np.ndarray:
    """A caller's table as f32 [win, win], or the ValueError of what ``weighting=`` refuses: another shape, a value that is
    not finite or is negative, no value above 0.  (The kernel itself reads negative and NaN entries as 0.)"""
    pc.check_win(win)
    w = np.asarray(weight)
    if w.shape != (int(win), int(win)):
        raise ValueError(f"a weight table of shape {w.shape} is not [{int(win)}, {int(win)}]")
    w = np.ascontiguousarray(w, np.float32)
    if not np.isfinite(w).all():
        raise ValueError("a weight is not finite")
    if (w < 0).any():
        raise ValueError("a weight is negative")
    if not (w > 0).any():
        raise ValueError("no weight is above 0")
    return w


def resolve(weighting, win: int):
    """The drivers' ``weighting=`` for windows of `win` pixels, as an f32 table [win, win] or None: None (section 5, no
    table), "gaussian" (sigma = win / 4), ("gaussian", sigma), "uniform", or an array [win, win] that check_weights
    passes."""
    if weighting is None:
        return None
    if isinstance(weighting, str):
        return window_weights(win, weighting)
    if isinstance(weighting, (tuple, list)) and len(weighting) == 2 and isinstance(weighting[0], str):
        return window_weights(win, weighting[0], weighting[1])
    return check_weights(weighting, win)


def check_method(method: str, weighting, mask=None):
    """Weights exist in the plain direct correlator alone: the phase correlator has window_sigma, and masks with weights
    are out of scope."""
    if weighting is None:
        return
    if method == "phase":
        raise ValueError('weighting= needs method="direct": the phase correlator weights its windows with window_sigma')
    if mask is not None:
        raise ValueError("weighting= and mask= cannot be combined: the masked correlator is unweighted")


def correlate_weighted_model(im1, im2, weight, win: int, step: int, radius: int, offset=None, planes: bool = False):
    """Host model of photon_piv_correlate_weighted in f64.  im1, im2 [height, width]; weight [win, win], entries that are
    not above 0 (negative, NaN) read as 0; offset as correlate_model takes it.  Returns what correlate_model returns.
    A window is flat by its pixels -- no weight above 0, all pixels of a under a weight equal, the in-image pixels of b at
    zero shift under a weight all equal or none -- or where an f64 energy is 0; the device also calls flat a window whose
    f32 energies are not above 0."""
    im1 = np.asarray(im1, np.float64)
    im2 = np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d arrays of one shape")
    win, step, R = int(win), int(step), int(radius)
    pc.check_arguments(im1.shape, win, step, R)
    wt = np.asarray(weight, np.float64)
    if wt.shape != (win, win):
        raise ValueError(f"a weight table of shape {wt.shape} is not [{win}, {win}]")
    with np.errstate(invalid="ignore"):
        Wt = np.where(wt > 0, wt, 0.0)
    live = Wt > 0
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
    span, nS = win + 2 * R, 2 * R + 1
    iw, isp = np.arange(win), np.arange(span)
    sw = Wt.sum()

    a_px = im1[(wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :]]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = a_px - ((Wt * a_px).sum(axis=(1, 2)) / sw)[:, None, None]
    gy = wy0[:, None] + oy[:, None] - R + isp                     # [n][span]
    gx = wx0[:, None] + ox[:, None] - R + isp
    iny, inx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
    inside = iny[:, :, None] & inx[:, None, :]
    b = im2[np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :]]
    zero = (slice(None), slice(R, R + win), slice(R, R + win))
    swb = np.where(inside[zero], Wt, 0.0).sum(axis=(1, 2))
    mean_b = np.where(swb > 0, np.where(inside[zero], Wt * b[zero], 0.0).sum(axis=(1, 2)) / np.where(swb > 0, swb, 1.0), 0.0)
    b_px = b[zero]
    b = np.where(inside, b - mean_b[:, None, None], 0.0)
    wa = Wt * a
    ea = (wa * a).sum(axis=(1, 2))
    eb = (Wt * b[zero] * b[zero]).sum(axis=(1, 2))

    C = np.empty((n, nS, nS), np.float64)
    for sy in range(nS):
        for sx in range(nS):
            C[:, sy, sx] = np.einsum("nij,nij->n", wa, b[:, sy:sy + win, sx:sx + win])

    # flatness from the pixels: the extremes over the weighted pixels of a, and of b at zero shift inside the image
    seen_b = inside[zero] & live
    flat_a = ~live.any() | (np.where(live, a_px, -np.inf).max(axis=(1, 2)) == np.where(live, a_px, np.inf).min(axis=(1, 2)))
    flat_b = ~seen_b.any(axis=(1, 2)) | (np.where(seen_b, b_px, -np.inf).max(axis=(1, 2)) == np.where(seen_b, b_px, np.inf).min(axis=(1, 2)))
    flat = flat_a | flat_b | (ea == 0.0) | (eb == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(ea * eb)
    return pc.peak_outputs(C, R, ox, oy, norm, flat, ~inside.all(axis=(1, 2)), (n_rows, n_cols), planes)
