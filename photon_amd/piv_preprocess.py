"""Host models of section 15 of include/parallel_ray_tracing.h (numpy): the background of a stack of frames and the chain
subtract -> clamp -> min-max filter that photon_piv_background and photon_piv_preprocess run on the device.

* ``background_model``: the per-pixel minimum or mean of the frames, in the header's order; the device returns its bits.
* ``preprocess_model_f32``: the header's operations one IEEE f32 operation at a time; the device returns its bits.
* ``preprocess_model``: the same definition and order in f64, what the f32 chain is measured against.
"""
from __future__ import annotations

import numpy as np

MODE_MIN, MODE_MEAN = 0, 1
MAX_RADIUS = 8
MAX_SIDE = 1 << 22


def check_arguments(shape, n_frames: int = 1, mode: int = MODE_MIN, radius: int = 0, floor=None, background: bool = True,
                    frame_stride=None, out_stride=None):
    """The arguments photon_piv_background (shape, n_frames, mode, frame_stride) and photon_piv_preprocess (all but mode)
    refuse, as a ValueError -- null pointers and overlapping buffers aside.  shape: (height, width); background: whether
    there is one; a stride None is width x height."""
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"width and height must be >= 1, not {w} x {h}")
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"the image is larger than 2^22 pixels a side: {w} x {h}")
    if int(n_frames) < 1:
        raise ValueError(f"n_frames must be >= 1, not {n_frames}")
    for name, s in (("frame_stride", frame_stride), ("out_stride", out_stride)):
        if s is not None and int(s) < w * h:
            raise ValueError(f"{name} {s} is smaller than one image of {w} x {h}")
    if int(mode) not in (MODE_MIN, MODE_MEAN):
        raise ValueError(f"mode must be 0 (minimum) or 1 (mean), not {mode}")
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"radius must lie in [0, {MAX_RADIUS}], not {radius}")
    if int(radius) > 0 and not (floor is not None and np.isfinite(np.float32(floor)) and np.float32(floor) > 0):
        raise ValueError(f"floor must be finite and > 0 with radius > 0, not {floor}")
    if int(radius) == 0 and not background:
        raise ValueError("radius 0 without a background: nothing to do")


def _stack(frames, dtype=np.float32):
    f = np.asarray(frames, dtype)
    if f.ndim == 2:
        f = f[None]
    if f.ndim != 3:
        raise ValueError("frames must be [N, height, width] (or one [height, width] image)")
    return f


def background_model(frames, mode: int = MODE_MIN) -> np.ndarray:
    """photon_piv_background's result, f32 [height, width], from f32 frames [N, height, width]: mode 0 the minimum, taken
    frame by frame (m = frame_k where frame_k < m), mode 1 the f64 sum in ascending k over N, rounded once."""
    f = _stack(frames)
    check_arguments(f.shape[1:], f.shape[0], mode)
    if int(mode) == MODE_MIN:
        m = f[0].copy()
        for k in range(1, f.shape[0]):
            m = np.where(f[k] < m, f[k], m)
        return m
    s = f[0].astype(np.float64)
    for k in range(1, f.shape[0]):
        s = s + f[k].astype(np.float64)
    return (s / np.float64(f.shape[0])).astype(np.float32)


def _shifted(a, d, axis):
    """(a moved so that out[p] = a[p + d] along `axis`, the mask of the p whose p + d lies in the image)."""
    n = a.shape[axis]
    idx = np.arange(n) + d
    ok = (idx >= 0) & (idx < n)
    moved = np.take(a, np.clip(idx, 0, n - 1), axis=axis)
    shape = [1] * a.ndim
    shape[axis] = n
    return moved, ok.reshape(shape)


def _extreme(a, r, op):
    """op (np.minimum / np.maximum) of a over the clipped (2r+1)^2 neighbourhood: exact, so rows and columns separate."""
    for axis in (a.ndim - 1, a.ndim - 2):
        out = a.copy()
        for d in range(-r, r + 1):
            moved, ok = _shifted(a, d, axis)
            out = np.where(ok, op(out, moved), out)
        a = out
    return a


def _box_sum(a, r):
    """The header's sum over the clipped neighbourhood in a's own precision: every row from +0 in ascending column, then
    the row sums from +0 in ascending row -- one addition at a time, a term outside the image skipped."""
    for axis in (a.ndim - 1, a.ndim - 2):
        s = np.zeros_like(a)
        for d in range(-r, r + 1):
            moved, ok = _shifted(a, d, axis)
            s = np.where(ok, s + moved, s)
        a = s
    return a


def _count(shape, r, dtype):
    h, w = shape
    rows = np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1
    cols = np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1
    return (rows[:, None] * cols[None, :]).astype(dtype)


def _chain(frames, background, radius, floor, dtype, parts):
    f = _stack(frames, dtype)
    bg = None if background is None else np.asarray(background, dtype)
    check_arguments(f.shape[1:], f.shape[0], radius=radius, floor=floor, background=bg is not None)
    if bg is not None and bg.shape != f.shape[1:]:
        raise ValueError("the background must be one [height, width] plane")
    zero = dtype(0)
    if bg is None:
        d = f
    else:
        x = f - bg
        d = np.where(x > zero, x, zero)
    r = int(radius)
    if r == 0:
        return d.copy()
    mn, mx = _extreme(d, r, np.minimum), _extreme(d, r, np.maximum)
    cnt = _count(f.shape[1:], r, dtype)
    lo, hi = _box_sum(mn, r) / cnt, _box_sum(mx, r) / cnt
    num, rng = d - lo, hi - lo
    fl = dtype(floor)
    out = np.where(num > zero, num, zero) / np.where(rng > fl, rng, fl)
    return (out, lo, hi) if parts else out


def preprocess_model_f32(frames, background=None, radius: int = 0, floor=None, parts: bool = False):
    """photon_piv_preprocess's result, f32 [N, height, width], every operation one f32 operation in the header's order (numpy
    keeps f32 operands in f32).  frames: f32 [N, height, width] or one image; background: one plane or None.
    parts=True: (out, lo, hi)."""
    return _chain(frames, background, radius, floor, np.float32, parts)


def preprocess_model(frames, background=None, radius: int = 0, floor=None, parts: bool = False):
    """The same definition in f64."""
    return _chain(frames, background, radius, floor, np.float64, parts)
