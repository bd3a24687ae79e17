"""Windowed direct cross-correlation of an image pair (pure numpy: usable without a GPU).

The device form is photon_piv_correlate (include/parallel_ray_tracing.h, section 5; ``PhotonLibrary.piv_correlate`` on raw
device pointers, ``PhotonLibrary.correlate`` on arrays).  This module holds

* ``correlate_model``: its f64 host model -- the definition of section 5, vectorised over windows, one loop over shifts
  (``raw_planes``: the unnormalised planes and the energies it reads the peak from);
* ``normalized_median_test`` and ``predictor``: the outlier test of Westerweel & Scarano (2005) on the 3 x 3 neighbourhood
  and the integer window offsets a second pass takes from the first;
* ``sensor_displacements``: the measured ``(dx, dy)`` -- along the image's columns and rows -- in the ``(x, y)`` pixel axes
  of ``deflections.to_pixels`` and ``piv_pairs.image_displacements``.

Axis mapping.  The 4-pixel splat (a camera without diffraction) writes column ``d_x`` and row ``d_y`` with
``d = (hit - p1) / pixel_pitch``: both grow with the sensor coordinates, so (x, y) = (dx, dy).  The erf splat (a camera
with diffraction) writes column ``x_pixel_number - 1 - d_x``, the reference's x-flipped pixel coordinate, and row ``d_y``:
there (x, y) = (-dx, dy).  Both are pinned by tests/test_piv_correlation_gpu.py.

Vectors and flags come in the window grid's shape: ``vectors[i, j] = (dx, dy, peak, ratio)`` of window (i, j),
``flags[i, j]`` its bits (FLAG_EDGE_PEAK, FLAG_FLAT, FLAG_OUTSIDE).
"""
from __future__ import annotations

import numpy as np

from . import deflections

WINDOW_SIZES = (16, 32, 64)
FLAG_EDGE_PEAK = 1          # the integer peak lies on the edge of the search square (no subpixel fit in that axis)
FLAG_FLAT = 2               # an energy is 0 (all pixels of a, or of b at zero shift, equal): every output of the window is NaN
FLAG_OUTSIDE = 4            # a pixel of im2 the window needs lies outside the image (it reads as the window's mean)


def check_win(win: int):
    if int(win) not in WINDOW_SIZES:
        raise ValueError(f"win must be one of {WINDOW_SIZES}, not {win}")


def check_grid(shape, win: int, step: int):
    """The (win, step) grids every window entry point refuses (sections 5, 11 and 13), as a ValueError.  An entry point with
    a rule that depends on win alone (radius, reach) checks win, then that rule, then the grid, as the device does."""
    h, w = shape
    check_win(win)
    if int(step) < 1:
        raise ValueError(f"step must be >= 1, not {step}")
    if h < win or w < win:
        raise ValueError(f"a {h} x {w} image is smaller than one {win} x {win} window")


def check_arguments(shape, win: int, step: int, radius: int):
    """The arguments photon_piv_correlate refuses, as a ValueError."""
    check_win(win)
    if not 1 <= int(radius) <= int(win) // 2:
        raise ValueError(f"radius must lie in [1, win / 2], not {radius}")
    check_grid(shape, win, step)


def grid_shape(shape, win: int, step: int):
    """(n_rows, n_cols) of the window grid on an image of `shape` (height, width)."""
    h, w = shape
    return (int(h) - int(win)) // int(step) + 1, (int(w) - int(win)) // int(step) + 1


def window_centres(shape, win: int, step: int):
    """Row and column index coordinates of the window centres, each [n_rows, n_cols] f64."""
    n_rows, n_cols = grid_shape(shape, win, step)
    c = (int(win) - 1) / 2.0
    r = np.arange(n_rows, dtype=np.float64) * step + c
    q = np.arange(n_cols, dtype=np.float64) * step + c
    return np.meshgrid(r, q, indexing="ij")


def _subpixel(cm, c0, cp):
    """3-point fit in f64: Gaussian where all three are positive, parabolic otherwise, 0 where the denominator is 0."""
    gauss = (cm > 0) & (c0 > 0) & (cp > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lm, l0, lp = (np.log(np.where(gauss, v, 1.0)) for v in (cm, c0, cp))
        num = np.where(gauss, lm - lp, cm - cp)
        den = np.where(gauss, 2.0 * (lm - 2.0 * l0 + lp), 2.0 * (cm - 2.0 * c0 + cp))
        return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), 0.0)


def peak_outputs(C, R: int, ox, oy, norm, flat, outside, grid, planes: bool = False):
    """What sections 5 and 13 report from the correlation planes C [n, 2R+1, 2R+1] of n = n_rows n_cols windows: the integer
    peak with the row-major tie rule, the three-point fit, the ratio, the flags; norm [n] scales C to the normalised plane.
    Returns (vectors [n_rows, n_cols, 4], flags [n_rows, n_cols] int32) and, with planes=True, the normalised planes."""
    n_rows, n_cols = grid
    n, nS = len(C), 2 * R + 1
    k = np.arange(n)
    Cf = C.reshape(n, nS * nS)
    best = np.argmax(Cf, axis=1)                                   # the first maximum: the tie rule
    py, px = best // nS, best % nS
    peak_c = Cf[k, best]
    sy_g, sx_g = np.meshgrid(np.arange(nS), np.arange(nS), indexing="ij")
    far = np.maximum(np.abs(sy_g[None] - py[:, None, None]), np.abs(sx_g[None] - px[:, None, None])) >= 2
    m2 = np.where(far, C, -np.inf).reshape(n, -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(m2 > 0, peak_c / np.where(m2 > 0, m2, 1.0), np.inf)

    edge_x, edge_y = (px == 0) | (px == nS - 1), (py == 0) | (py == nS - 1)
    pxi, pyi = np.clip(px, 1, nS - 2), np.clip(py, 1, nS - 2)
    dx = np.where(edge_x, 0.0, _subpixel(C[k, py, pxi - 1], C[k, py, pxi], C[k, py, pxi + 1]))
    dy = np.where(edge_y, 0.0, _subpixel(C[k, pyi - 1, px], C[k, pyi, px], C[k, pyi + 1, px]))
    with np.errstate(invalid="ignore"):                            # (a flat window: 0 * inf, NaN below anyway)
        vectors = np.stack([ox + (px - R) + dx, oy + (py - R) + dy, peak_c * norm, ratio], axis=1)
    flags = np.where(edge_x | edge_y, FLAG_EDGE_PEAK, 0) | np.where(outside, FLAG_OUTSIDE, 0)
    flags = np.where(flat, FLAG_FLAT | np.where(outside, FLAG_OUTSIDE, 0), flags).astype(np.int32)
    vectors[flat] = np.nan
    out = (vectors.reshape(n_rows, n_cols, 4), flags.reshape(n_rows, n_cols))
    if planes:
        with np.errstate(invalid="ignore"):
            Cn = C * norm[:, None, None]
        Cn[flat] = np.nan
        out = out + (Cn.reshape(n_rows, n_cols, nS, nS),)
    return out


def raw_planes(im1, im2, win: int, step: int, radius: int, offset=None):
    """What section 5 defines for one pair before the peak is read, in f64: (C [n, 2R+1, 2R+1] the unnormalised planes,
    ea [n], eb [n] the energies, ox [n], oy [n] the integer offsets, outside [n] bool, (n_rows, n_cols)).  correlate_model
    reads the peak off these; piv_ensemble.correlate_ensemble_model sums them over pairs first."""
    im1 = np.asarray(im1, np.float64)
    im2 = np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d arrays of one shape")
    win, step, R = int(win), int(step), int(radius)
    check_arguments(im1.shape, win, step, R)
    H, W = im1.shape
    n_rows, n_cols = grid_shape(im1.shape, win, step)
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

    a = im1[(wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :]]
    a = a - a.mean(axis=(1, 2))[:, None, None]
    gy = wy0[:, None] + oy[:, None] - R + isp                     # [n][span]
    gx = wx0[:, None] + ox[:, None] - R + isp
    iny, inx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
    inside = iny[:, :, None] & inx[:, None, :]
    b = im2[np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :]]
    zero = (slice(None), slice(R, R + win), slice(R, R + win))
    cnt = inside[zero].sum(axis=(1, 2))
    mean_b = np.where(cnt > 0, np.where(inside[zero], b[zero], 0.0).sum(axis=(1, 2)) / np.maximum(cnt, 1), 0.0)
    b = np.where(inside, b - mean_b[:, None, None], 0.0)
    ea = (a * a).sum(axis=(1, 2))
    eb = (b[zero] * b[zero]).sum(axis=(1, 2))

    C = np.empty((n, nS, nS), np.float64)
    for sy in range(nS):
        for sx in range(nS):
            C[:, sy, sx] = np.einsum("nij,nij->n", a, b[:, sy:sy + win, sx:sx + win])
    return C, ea, eb, ox, oy, ~inside.all(axis=(1, 2)), (n_rows, n_cols)


def correlate_model(im1, im2, win: int, step: int, radius: int, offset=None, planes: bool = False):
    """Host model of photon_piv_correlate in f64.  im1, im2: [height, width]; offset: integer (ox, oy) per window,
    [n_rows, n_cols, 2] or [n][2], or None.  Returns (vectors [n_rows, n_cols, 4], flags [n_rows, n_cols] int32) and, with
    planes=True, the normalised planes [n_rows, n_cols, 2R+1, 2R+1] (row-major: sy, then sx) as a third item.
    A window is flat where an f64 energy is 0, which for finite pixels is where all pixels of a, or all in-image pixels of b
    at zero shift, are equal; the device decides that from the pixels' extremes and also calls flat a window whose f32
    energies are not above 0, a contrast below f32 that this model still correlates."""
    C, ea, eb, ox, oy, outside, grid = raw_planes(im1, im2, win, step, radius, offset)
    flat = (ea == 0.0) | (eb == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(ea * eb)
    return peak_outputs(C, int(radius), ox, oy, norm, flat, outside, grid, planes)


def _neighbours(field):
    """The 8 neighbours of every grid point: [8, n_rows, n_cols, ...], NaN beyond the grid's edge."""
    f = np.asarray(field, np.float64)
    pad = np.full((f.shape[0] + 2, f.shape[1] + 2) + f.shape[2:], np.nan)
    pad[1:-1, 1:-1] = f
    r, c = f.shape[:2]
    return np.stack([pad[1 + di:1 + di + r, 1 + dj:1 + dj + c] for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj])


def normalized_median_test(vectors, eps: float = 0.1, threshold: float = 2.0) -> np.ndarray:
    """Westerweel & Scarano (2005) on the 3 x 3 neighbourhood: per component, r = |u0 - median(u_i)| / (median(|u_i -
    median(u_i)|) + eps) over the valid (finite) neighbours; a vector is an outlier when sqrt(r_x^2 + r_y^2) > threshold,
    or when it is not finite.  vectors [n_rows, n_cols, >= 2] (dx, dy first); returns bool [n_rows, n_cols]."""
    v = np.asarray(vectors, np.float64)[..., :2]
    nb = _neighbours(v)                                            # [8, r, c, 2]
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)                                 # all-NaN neighbourhoods
        med = np.nanmedian(nb, axis=0)
        rm = np.nanmedian(np.abs(nb - med[None]), axis=0)
        r = np.abs(v - med) / (rm + float(eps))
    score = np.sqrt((r * r).sum(axis=-1))
    return ~np.isfinite(v).all(axis=-1) | (np.nan_to_num(score, nan=0.0) > float(threshold))


def predictor(vectors, flags, outliers) -> np.ndarray:
    """Integer window offsets for a second pass from pass-1 vectors: outliers and flat windows take the median of their
    valid 3 x 3 neighbours (0 where there is none), then every vector is rounded.  Returns int32 [n_rows, n_cols, 2]
    (ox, oy): the layout photon_piv_correlate's d_offset reads."""
    v = np.array(np.asarray(vectors, np.float64)[..., :2])
    bad = np.asarray(outliers, bool) | ((np.asarray(flags) & FLAG_FLAT) != 0) | ~np.isfinite(v).all(axis=-1)
    good = np.where(bad[..., None], np.nan, v)
    with np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        repl = np.nanmedian(_neighbours(good), axis=0)
    v[bad] = repl[bad]
    return np.ascontiguousarray(np.rint(np.nan_to_num(v, nan=0.0)).astype(np.int32))


def sensor_displacements(vectors, camera) -> np.ndarray:
    """Measured (dx, dy) -- image columns, rows -- in the (x, y) pixel axes of deflections.to_pixels and
    piv_pairs.image_displacements: (dx, dy) for the 4-pixel splat, (-dx, dy) for the erf splat (a camera with
    implement_diffraction; its column axis is x-flipped).  ``camera``: a camera dict or a call.  Returns [..., 2] f64."""
    v = np.asarray(vectors, np.float64)[..., :2]
    flip = -1.0 if bool(deflections._camera(camera).get("implement_diffraction", False)) else 1.0
    return np.stack([flip * v[..., 0], v[..., 1]], axis=-1)


def image_positions(pos_px, camera) -> np.ndarray:
    """deflections.to_pixels positions [..., 2] -> image index coordinates (column, row) [..., 2] of the spot's centroid:
    (x - 1, y - 1) for the 4-pixel splat (its taps land one row and one column before their pixel), (N - 2 - x, y) for the
    erf splat (x-flipped), N = x_pixel_number."""
    cam = deflections._camera(camera)
    p = np.asarray(pos_px, np.float64)
    if bool(cam.get("implement_diffraction", False)):
        return np.stack([int(cam["x_pixel_number"]) - 2 - p[..., 0], p[..., 1]], axis=-1)
    return np.stack([p[..., 0] - 1.0, p[..., 1] - 1.0], axis=-1)


def window_truth(positions, displacements, shape, win: int, step: int, min_count: int = 5):
    """The truth of each window: the mean displacement of the particles whose frame-1 centroid (x = column, y = row, pixel
    index coordinates) lies in it.  Returns (mean [n_rows, n_cols, 2], count [n_rows, n_cols]); NaN where fewer than
    min_count particles lie in the window."""
    p = np.asarray(positions, np.float64).reshape(-1, 2)
    d = np.asarray(displacements, np.float64).reshape(-1, 2)
    ok = np.isfinite(p).all(axis=1) & np.isfinite(d).all(axis=1)
    p, d = p[ok], d[ok]
    n_rows, n_cols = grid_shape(shape, win, step)
    total = np.zeros((n_rows, n_cols, 2))
    count = np.zeros((n_rows, n_cols), np.int64)
    # window (i, j) holds column c when j step <= c + 1/2 < j step + win (the pixel a centroid falls in), likewise rows
    col, row = np.floor(p[:, 0] + 0.5).astype(np.int64), np.floor(p[:, 1] + 0.5).astype(np.int64)
    for i in range(n_rows):
        in_r = (row >= i * step) & (row < i * step + win)
        if not in_r.any():
            continue
        for j in range(n_cols):
            m = in_r & (col >= j * step) & (col < j * step + win)
            count[i, j] = m.sum()
            if count[i, j]:
                total[i, j] = d[m].sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / count[..., None]
    mean[count < min_count] = np.nan
    return mean, count


def particle_image(shape, x, y, diameter: float = 2.5, intensity=1.0) -> np.ndarray:
    """An analytic particle image [height, width] f64: Gaussian spots of e^-2 diameter `diameter` pixels (sigma = d / 4)
    centred at column x, row y (index coordinates), each integrated exactly over the pixels (erf), out to 2 d."""
    h, w = (int(v) for v in shape)
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    amp = np.broadcast_to(np.asarray(intensity, np.float64), x.shape)
    from scipy.special import erf
    s = np.sqrt(2.0) * diameter / 4.0
    half = int(np.ceil(2.0 * diameter))
    off = np.arange(-half, half + 1)
    cols = np.floor(x + 0.5).astype(np.int64)[:, None] + off
    rows = np.floor(y + 0.5).astype(np.int64)[:, None] + off
    ex = 0.5 * (erf((cols + 0.5 - x[:, None]) / s) - erf((cols - 0.5 - x[:, None]) / s))
    ey = 0.5 * (erf((rows + 0.5 - y[:, None]) / s) - erf((rows - 0.5 - y[:, None]) / s))
    vals = amp[:, None, None] * ey[:, :, None] * ex[:, None, :]
    rr = np.broadcast_to(rows[:, :, None], vals.shape)
    cc = np.broadcast_to(cols[:, None, :], vals.shape)
    ok = (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
    img = np.zeros((h, w))
    np.add.at(img, (rr[ok], cc[ok]), vals[ok])
    return img
