"""Host models (numpy, no GPU) of the dot tracking of include/parallel_ray_tracing.h, section 8: detect the dots of an
image, locate each to a fraction of a pixel, pair the dots of two frames, average the pairs onto section 5's window grid.

The definitions are the header's, in the same words; detect, match and window means are what the device must return
exactly (integers, f32 steps and f64 sums in the header's order), the fit is the f64 reference the device is held to
within 1e-3 px.  Coordinates are index coordinates: x = column, y = row.
"""
from __future__ import annotations

import numpy as np

from . import deflections
from . import piv_correlation as pc

STATUS_BOX_OUTSIDE = 1      # the box leaves the image
STATUS_PULLED = 2           # the final position lies more than 1 px from the peak pixel's centre in either axis
STATUS_NO_WEIGHT = 4        # a round's sum of weights was not > 0
STATUS_NO_PIXEL = 8         # the peak index is no pixel of the image
FLAG_NO_DATA = pc.FLAG_FLAT  # section 5's "no data" bit: fewer than min_count dots in the window

MAX_BOX_RADIUS, MAX_ITERATIONS = 7, 16


def image_max_model(im) -> np.float32:
    """The largest finite pixel, 0 when there is none above 0 (photon_dots_image_max)."""
    a = np.asarray(im, np.float32)
    a = a[np.isfinite(a)]
    return np.float32(max(a.max(), 0.0)) if a.size else np.float32(0.0)


def detect_model(im, threshold: float, scale=None, max_dots=None):
    """Section 8a: (peaks int32 [min(total, max_dots)] in increasing pixel index, total)."""
    a = np.asarray(im, np.float32)
    if a.ndim != 2 or a.shape[0] < 3 or a.shape[1] < 3:
        raise ValueError("the image must be 2-d and at least 3 x 3")
    if not np.isfinite(threshold):
        raise ValueError("threshold must be finite")
    if max_dots is not None and int(max_dots) < 1:
        raise ValueError("max_dots must be >= 1")
    h, w = a.shape
    thr = np.float32(threshold) * (np.float32(1.0) if scale is None else np.float32(scale))
    v = a[1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v > thr)
        for dr, dq in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):        # the four that precede: v > n, a NaN passes
            ok &= ~(v <= a[1 + dr:h - 1 + dr, 1 + dq:w - 1 + dq])
        for dr, dq in ((0, 1), (1, -1), (1, 0), (1, 1)):            # the four that follow: v >= n, a NaN passes
            ok &= ~(v < a[1 + dr:h - 1 + dr, 1 + dq:w - 1 + dq])
    r, q = np.nonzero(ok)
    peaks = ((r + 1) * w + (q + 1)).astype(np.int32)                # np.nonzero is row-major: increasing index
    total = int(peaks.size)
    return (peaks if max_dots is None else peaks[:int(max_dots)]), total


def _check_fit(box_radius, sigma_w, iterations, background):
    if not 1 <= int(box_radius) <= MAX_BOX_RADIUS:
        raise ValueError(f"box_radius must lie in [1, {MAX_BOX_RADIUS}], not {box_radius}")
    if not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in [0, {MAX_ITERATIONS}], not {iterations}")
    if not (np.isfinite(sigma_w) and sigma_w > 0):
        raise ValueError(f"sigma_w must be finite and > 0, not {sigma_w}")
    if not np.isfinite(background):
        raise ValueError(f"background must be finite, not {background}")


def fit_model(im, peaks, box_radius: int = 3, sigma_w: float = 1.0, iterations: int = 4, background: float = 0.0):
    """Section 8b in f64: (dots [n, 4] = x, y, I at the peak pixel, diameter; status int32 [n])."""
    _check_fit(box_radius, sigma_w, iterations, background)
    a = np.asarray(im, np.float32).astype(np.float64)
    h, w = a.shape
    R, nb = int(box_radius), 2 * int(box_radius) + 1
    p = np.asarray(peaks, np.int64).ravel()
    n = p.size
    dots, status = np.full((n, 4), np.nan), np.zeros(n, np.int32)
    pixel = (p >= 0) & (p < h * w)
    status[~pixel] = STATUS_NO_PIXEL
    if not pixel.any():
        return dots, status
    r, q = p[pixel] // w, p[pixel] % w
    off = np.arange(-R, R + 1)
    rows, cols = r[:, None] + off, q[:, None] + off                # [m, nb]
    inside = ((rows >= 0) & (rows < h))[:, :, None] & ((cols >= 0) & (cols < w))[:, None, :]
    box = a[np.clip(rows, 0, h - 1)[:, :, None], np.clip(cols, 0, w - 1)[:, None, :]]
    box = np.where(inside & np.isfinite(box), box, background)
    I = np.maximum(box - float(background), 0.0)                     # [m, row, column]
    st = np.where((q - R < 0) | (q + R > w - 1) | (r - R < 0) | (r + R > h - 1), STATUS_BOX_OUTSIDE, 0).astype(np.int32)
    dx = pc._subpixel(I[:, R, R - 1], I[:, R, R], I[:, R, R + 1])
    dy = pc._subpixel(I[:, R - 1, R], I[:, R, R], I[:, R + 1, R])
    o = off.astype(np.float64)[None, :]
    two_s2 = 2.0 * float(sigma_w) ** 2

    def weights(dx, dy):
        ex = np.exp(-(o - dx[:, None]) ** 2 / two_s2)
        ey = np.exp(-(o - dy[:, None]) ** 2 / two_s2)
        return I * ey[:, :, None] * ex[:, None, :]

    for _ in range(int(iterations)):
        wgt = weights(dx, dy)
        sw = wgt.sum(axis=(1, 2))
        good = sw > 0.0
        safe = np.where(good, sw, 1.0)
        dx = np.where(good, (wgt * o[:, None, :]).sum(axis=(1, 2)) / safe, dx)
        dy = np.where(good, (wgt * o[:, :, None]).sum(axis=(1, 2)) / safe, dy)
        st[~good] |= STATUS_NO_WEIGHT
    diameter = np.full(dx.shape, np.nan)
    if int(iterations) > 0:
        wgt = weights(dx, dy)
        sw = wgt.sum(axis=(1, 2))
        d2 = (o[:, None, :] - dx[:, None, None]) ** 2 + (o[:, :, None] - dy[:, None, None]) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (wgt * d2).sum(axis=(1, 2)) / (2.0 * sw)
            sg2 = float(sigma_w) ** 2
            s2 = v * sg2 / (sg2 - v) - 1.0 / 12.0
            ok = (sw > 0.0) & np.isfinite(s2) & (s2 > 0.0)
            diameter = np.where(ok, 4.0 * np.sqrt(np.where(ok, s2, 1.0)), np.nan)
    st[(np.abs(dx) > 1.0) | (np.abs(dy) > 1.0)] |= STATUS_PULLED
    dots[pixel] = np.stack([q + dx, r + dy, I[:, R, R], diameter], axis=1)
    status[pixel] = st
    return dots, status


def _grid_weight_at(p, win: int, step: int, n: int):
    """Section 8c's f32 steps: node indices and weight of the bilinear rule at the continuous coordinate p."""
    f32 = np.float32
    c = f32(win - 1) * f32(0.5)
    f = (p.astype(f32) - c) / f32(step)
    f = np.minimum(np.maximum(f, f32(0.0)), f32(n - 1))
    i0 = np.minimum(np.floor(f).astype(np.int64), max(n - 2, 0))
    return i0, np.minimum(i0 + 1, n - 1), (f - i0.astype(f32)).astype(f32)


def predict_model(field, win: int, step: int, x, y) -> np.ndarray:
    """The predictor grid [n_rows, n_cols, >= 2] at the continuous positions (x, y), f32 [n, 2] (section 8c)."""
    F = np.array(np.asarray(field, np.float32)[..., :2])
    F[~np.isfinite(F).all(axis=-1)] = 0.0
    n_rows, n_cols = F.shape[:2]
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    i0, i1, wy = _grid_weight_at(y, int(win), int(step), n_rows)
    j0, j1, wx = _grid_weight_at(x, int(win), int(step), n_cols)
    wx, wy = wx[:, None], wy[:, None]

    def lerp(a, b, w):
        return (a + (w * (b - a)).astype(np.float32)).astype(np.float32)

    return lerp(lerp(F[i0, j0], F[i0, j1], wx), lerp(F[i1, j0], F[i1, j1], wx), wy)


def match_model(dots1, status1, dots2, status2, radius: float, predictor=None, reject_mask: int = 0):
    """Section 8c by brute force, O(n1 n2): (pair int32 [n1], shift f32 [n1, 4], npaired).  predictor: None, or
    (field [n_rows, n_cols, >= 2], win, step)."""
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError(f"radius must be finite and > 0, not {radius}")
    f32 = np.float32
    p1, p2 = (np.asarray(d, f32).reshape(-1, 4)[:, :2] for d in (dots1, dots2))
    n1, n2 = p1.shape[0], p2.shape[0]

    def part(p, status):
        ok = np.isfinite(p).all(axis=1)
        if status is not None:
            ok &= (np.asarray(status).ravel() & int(reject_mask)) == 0
        return ok

    with np.errstate(invalid="ignore", over="ignore"):
        ok1, ok2 = part(p1, status1), part(p2, status2)
        t = p1.copy()
        if predictor is not None and n1:
            field, win, step = predictor
            safe = np.where(ok1[:, None], p1, f32(0.0))
            t = (p1 + predict_model(field, win, step, safe[:, 0], safe[:, 1])).astype(f32)
        ok1 &= np.isfinite(t).all(axis=1)
        pair, shift = np.full(n1, -1, np.int32), np.full((n1, 4), np.nan, f32)
        if n1 and n2:
            r2 = f32(radius) * f32(radius)
            jstar, jbest = np.full(n1, -1, np.int64), np.full(n1, np.inf, f32)
            istar, ibest = np.full(n2, -1, np.int64), np.full(n2, np.inf, f32)
            for s in range(0, n1, 512):                            # blocks of targets, in increasing index
                rows = np.arange(s, min(s + 512, n1))
                ex = (p2[None, :, 0] - t[rows, None, 0]).astype(f32)
                ey = (p2[None, :, 1] - t[rows, None, 1]).astype(f32)
                d2 = ((ex * ex).astype(f32) + (ey * ey).astype(f32)).astype(f32)
                d2 = np.where(ok1[rows, None] & ok2[None, :] & (d2 <= r2), d2, f32(np.inf))
                j = np.argmin(d2, axis=1)                           # the first minimum: ties to the smallest index
                jbest[rows] = d2[np.arange(rows.size), j]
                jstar[rows] = np.where(np.isfinite(jbest[rows]), j, -1)
                i = np.argmin(d2, axis=0)
                best = d2[i, np.arange(n2)]
                better = best < ibest                               # strictly: an earlier block's equal distance stays
                istar[better], ibest[better] = rows[i[better]], best[better]
            paired = (jstar >= 0) & (istar[np.maximum(jstar, 0)] == np.arange(n1))
            pair[paired] = jstar[paired]
            d = (p2[jstar[paired]] - p1[paired]).astype(f32)
            shift[paired, :2] = (p1[paired] + (d * f32(0.5)).astype(f32)).astype(f32)
            shift[paired, 2:] = d
    return pair, shift, int((pair >= 0).sum())


def window_means_model(dots1, pair, shift, shape, win: int, step: int, min_count: int = 3, anchor: int = 0, rounded: bool = True):
    """Section 8d: (vectors f32 [n_rows, n_cols, 4] = mean dx, mean dy, count, rms; flags int32 [n_rows, n_cols]).  f64 sums
    in increasing dot index; rounded=False returns the f64 values before the one rounding to f32."""
    if int(win) < 1 or int(step) < 1 or int(min_count) < 1 or int(anchor) not in (0, 1):
        raise ValueError("win, step and min_count must be >= 1 and anchor 0 or 1")
    h, w = (int(v) for v in shape)
    if h < win or w < win:
        raise ValueError(f"a {h} x {w} image is smaller than one {win} x {win} window")
    n_rows, n_cols = pc.grid_shape((h, w), win, step)
    p1 = np.asarray(dots1, np.float32).reshape(-1, 4)
    sh = np.asarray(shift, np.float32).reshape(-1, 4)
    pr = np.asarray(pair).ravel()
    a = (sh[:, :2] if int(anchor) else p1[:, :2]).astype(np.float64)
    d = sh[:, 2:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        col, row = np.floor(a[:, 0] + 0.5), np.floor(a[:, 1] + 0.5)
    use = (pr >= 0) & np.isfinite(d).all(axis=1) & np.isfinite(col) & np.isfinite(row)

    def owners(c: int, n: int):
        """the windows i along one axis with i step <= c < i step + win"""
        lo = max(0, -((win - 1 - c) // step))                      # ceil((c - win + 1) / step)
        return range(lo, min(n - 1, c // step) + 1)

    win, step = int(win), int(step)
    members = [[[] for _ in range(n_cols)] for _ in range(n_rows)]
    for k in np.nonzero(use)[0]:                                     # increasing dot index
        if not (0 <= row[k] < h + win and 0 <= col[k] < w + win):
            continue
        for i in owners(int(row[k]), n_rows):
            for j in owners(int(col[k]), n_cols):
                members[i][j].append(k)
    vectors = np.full((n_rows, n_cols, 4), np.nan, np.float32 if rounded else np.float64)
    flags = np.zeros((n_rows, n_cols), np.int32)
    for i in range(n_rows):
        for j in range(n_cols):
            ks = members[i][j]
            cnt = len(ks)
            vectors[i, j, 2] = cnt
            if cnt < int(min_count):
                flags[i, j] = FLAG_NO_DATA
                continue
            sx = sy = 0.0
            for k in ks:
                sx = sx + d[k, 0]
                sy = sy + d[k, 1]
            mx, my = sx / cnt, sy / cnt
            q = 0.0
            for k in ks:
                ex, ey = d[k, 0] - mx, d[k, 1] - my
                q = q + (ex * ex + ey * ey)
            vectors[i, j, 0], vectors[i, j, 1], vectors[i, j, 3] = mx, my, np.sqrt(q / cnt)
    return vectors, flags


def default_max_dots(shape) -> int:
    """The capacity track_dots takes when none is given: one dot per 32 pixels, at least 1024."""
    return max(1024, int(shape[0]) * int(shape[1]) // 32)


def track_dots_model(im1, im2, threshold: float, box_radius: int = 3, sigma_w: float = 1.0, iterations: int = 4,
                     background: float = 0.0, radius: float = 3.0, predictor=None, max_dots=None, grid=None,
                     relative: bool = False) -> dict:
    """The chain of PhotonLibrary.track_dots on the host, the same keys: dots1 / dots2 [n, 4], status1 / status2, count1 /
    count2 (the totals detect found), pair, shift, npaired, and with grid = (win, step, min_count, anchor) vectors and
    flags.  predictor: None or (field, win, step).  relative: the threshold is a fraction of each image's own maximum (image_max_model)."""
    a, b = (np.asarray(x, np.float32) for x in (im1, im2))
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("im1 and im2 must be two 2-d images of one shape")
    cap = default_max_dots(a.shape) if max_dots is None else int(max_dots)
    out = {}
    for name, im in (("1", a), ("2", b)):
        peaks, total = detect_model(im, threshold, image_max_model(im) if relative else None, cap)
        dots, status = fit_model(im, peaks, box_radius, sigma_w, iterations, background)
        out["dots" + name], out["status" + name], out["count" + name] = dots.astype(np.float32), status, total
    out["pair"], out["shift"], out["npaired"] = match_model(out["dots1"], out["status1"], out["dots2"], out["status2"], radius, predictor)
    if grid is not None:
        win, step, min_count, anchor = grid
        out["vectors"], out["flags"] = window_means_model(out["dots1"], out["pair"], out["shift"], a.shape, win, step, min_count, anchor)
    return out


def true_dots(records1, records2, camera, rays_per_source: int, group: int = 1, policy: str = "reference") -> dict:
    """The per-dot truth of a rendered pair in image index coordinates, from the records of its two traces
    (deflections.dot_deflections) and piv_correlation.image_positions: {"pos1", "pos2": [dots, 2] (x = column, y = row),
    "shift": pos2 - pos1, the shift from frame 1 to frame 2 as section 8c reports it}.  NaN for a dot the policy drops."""
    d = deflections.dot_deflections(records1, records2, camera, rays_per_source, group, policy)
    pos1, pos2 = pc.image_positions(d.pos1, camera), pc.image_positions(d.pos2, camera)
    return {"pos1": pos1, "pos2": pos2, "shift": pos2 - pos1}


def identify(tracked_xy, true_xy, radius: float = 1.0):
    """For every true dot the nearest tracked position within `radius` px: index [n_true] (-1: none).  Brute force, in
    blocks."""
    t = np.asarray(tracked_xy, np.float64).reshape(-1, 2)
    g = np.asarray(true_xy, np.float64).reshape(-1, 2)
    out = np.full(g.shape[0], -1, np.int64)
    if not t.shape[0]:
        return out
    tt = np.where(np.isfinite(t), t, 1e30)
    for s in range(0, g.shape[0], 1024):
        blk = g[s:s + 1024]
        with np.errstate(invalid="ignore"):
            d2 = ((blk[:, None, :] - tt[None, :, :]) ** 2).sum(axis=-1)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        k = np.argmin(d2, axis=1)
        ok = d2[np.arange(blk.shape[0]), k] <= radius * radius
        out[s:s + 1024][ok] = k[ok]
    return out


def score(result: dict, true_pos1, true_shift, inside=None) -> dict:
    """A tracked pair against the per-dot truth: a true dot (of `inside`, a bool mask, default all finite ones) is
    identified when a PAIRED frame-1 position lies within 1 px of it.  Returns tracked (share of the true dots
    identified), wrong (share of the identified whose shift is off by more than 0.5 px), median and p95 of the per-dot
    error |shift - truth| over the identified, and n."""
    p = np.asarray(true_pos1, np.float64).reshape(-1, 2)
    s = np.asarray(true_shift, np.float64).reshape(-1, 2)
    use = np.isfinite(p).all(axis=1) & np.isfinite(s).all(axis=1)
    if inside is not None:
        use &= np.asarray(inside, bool)
    paired = np.nonzero(np.asarray(result["pair"]) >= 0)[0]
    k = identify(np.asarray(result["dots1"])[paired, :2], p[use])
    found = k >= 0
    err = np.linalg.norm(np.asarray(result["shift"], np.float64)[paired[k[found]], 2:] - s[use][found], axis=1)
    n = int(use.sum())
    return {"n": n, "tracked": float(found.sum() / max(n, 1)), "wrong": float((err > 0.5).mean()) if err.size else 0.0,
            "median": float(np.median(err)) if err.size else np.nan, "p95": float(np.percentile(err, 95)) if err.size else np.nan}
