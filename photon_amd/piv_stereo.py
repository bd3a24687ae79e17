"""Stereo PIV (pure numpy: usable without a GPU): two cameras on one light sheet, three displacement components.

The device forms are photon_piv_dewarp and photon_piv_stereo_reconstruct (include/parallel_ray_tracing.h, section 19;
``PhotonLibrary.piv_dewarp`` / ``piv_stereo_reconstruct`` on raw device pointers, ``PhotonLibrary.dewarp`` and
``PhotonLibrary.correlate_stereo`` on arrays).  This module holds what the C side has no part in and the host models:

* the camera model -- Soloff's polynomial from world (X, Y, Z) to image (x, y), 19 terms per coordinate: ``fit_camera``
  (least squares on a calibration target), ``map_points``, ``jacobian`` (analytic, in section 19b's operation order) and
  ``plane_coefficients`` (the camera folded at a plane into what the dewarp kernel takes);
* ``dewarp_model_f32`` (the kernel's operations in numpy f64 and f32: the device equals it bit for bit) and ``dewarp_model``
  (f64 throughout, from piv_deformation.bspline_coefficients_model); ``sensor_points``, ``bspline_sample``: their shared parts;
* ``reconstruct_model``: section 19b in numpy, operation by operation;
* ``correlate_stereo_model``: the model of the driver's "deform" chain;
* generators for the tests and tools: ``pinhole`` (a perspective camera to calibrate against), ``calibration_target``,
  ``centred_plane`` and ``particle_pair`` (Gaussian particle images of a 3-C flow in a Gaussian sheet, per camera), and
  the three synthetic pairs the tests and tools/piv_stereo.py measure (``CASES``, ``case_pair``, ``case_figures``).

A camera is a dict centre[3], scale[3], cx[19], cy[19] (f64); a plane a dict x0, y0, pitch, z, width, height: dewarped
pixel (row i, column j) is the world point (x0 + j pitch, y0 + i pitch, z).

Self-calibration (Wieneke 2005; section 19c): a sheet that is not where the calibration target stood shows as a disparity
between the two cameras' dewarped frames of one instant.  ``triangulate_model`` (the model of
photon_piv_stereo_triangulate) turns that disparity field into world points, ``fit_sheet`` fits Z = a + b X + c Y to them,
``sheet_frame`` and ``move_camera`` re-express both cameras in coordinates in which the sheet is the plane's z, and
``self_calibrate_model`` runs the rounds (the model of ``PhotonLibrary.self_calibrate_stereo``).  ``sheet_frames`` and
``sheet_pair`` render particles in a displaced sheet; ``SELFCAL_CASE`` and ``selfcal_figures`` are the case the tests and
the tool measure.

The reconstruction is first order: the Jacobian is taken at the plane, at the window centre, not at the half-displaced
particle positions.  A sheet that is not where the calibration says is found and corrected by the self-calibration above,
before ``correlate_stereo`` and by the caller: the reconstruction itself applies no correction.  What does not exist: an
estimate of the sheet's thickness from the width of the disparity peak, and any correction under a dewarp mask beyond
leaving those nodes out of the sheet fit.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc
from . import piv_deformation as pd

N_TERMS = 19
FLAG_DEGENERATE = 64        # reconstruct: the two views do not span three components (pivot ratio <= MIN_PIVOT_RATIO)
FLAG_NOT_FINITE = 128       # reconstruct: a dx or dy of either camera is not finite
MIN_PIVOT_RATIO = 1e-12


# ---- the camera --------------------------------------------------------------------------------------------------------------
def _terms(q) -> np.ndarray:
    """The 19 terms of section 19 at the normalised points q [..., 3] -> [..., 19]."""
    X, Y, Z = q[..., 0], q[..., 1], q[..., 2]
    return np.stack([np.ones_like(X), X, Y, Z, X * X, X * Y, Y * Y, X * Z, Y * Z, Z * Z, X * X * X, X * X * Y, X * Y * Y, Y * Y * Y,
                     X * X * Z, X * Y * Z, Y * Y * Z, X * (Z * Z), Y * (Z * Z)], axis=-1)


def camera(centre, scale, cx, cy) -> dict:
    cam = dict(centre=np.array(centre, np.float64), scale=np.array(scale, np.float64), cx=np.array(cx, np.float64),
               cy=np.array(cy, np.float64))
    if cam["centre"].shape != (3,) or cam["scale"].shape != (3,) or cam["cx"].shape != (N_TERMS,) or cam["cy"].shape != (N_TERMS,):
        raise ValueError("a camera is centre[3], scale[3], cx[19], cy[19]")
    if not all(np.isfinite(v).all() for v in cam.values()) or (cam["scale"] == 0).any():
        raise ValueError("a camera's values must be finite and its scale not 0")
    return cam


def identity_camera() -> dict:
    """x = X, y = Y."""
    cx, cy = np.zeros(N_TERMS), np.zeros(N_TERMS)
    cx[1] = cy[2] = 1.0
    return camera(np.zeros(3), np.ones(3), cx, cy)


def _normalised(cam, P):
    return (np.asarray(P, np.float64) - cam["centre"]) / cam["scale"]


def map_points(cam, P) -> np.ndarray:
    """Image points [..., 2] = (x, y) in pixels of the world points P [..., 3]."""
    t = _terms(_normalised(cam, P))
    return np.stack([t @ cam["cx"], t @ cam["cy"]], axis=-1)


def fit_camera(world, image):
    """Least-squares fit (numpy.linalg.lstsq) of a camera to calibration points: world [n, 3], image [n, 2] in pixels; the
    target needs at least three Z positions and four positions along X and Y.  centre and scale are the middle and the
    half range of the world points per axis.  Returns (camera, rms residual, max residual), the residuals in pixels."""
    world, image = np.asarray(world, np.float64).reshape(-1, 3), np.asarray(image, np.float64).reshape(-1, 2)
    if world.shape[0] != image.shape[0] or world.shape[0] < N_TERMS:
        raise ValueError(f"fit_camera needs the same number (>= {N_TERMS}) of world and image points")
    lo, hi = world.min(axis=0), world.max(axis=0)
    centre, scale = (lo + hi) / 2.0, np.where(hi > lo, (hi - lo) / 2.0, 1.0)
    t = _terms((world - centre) / scale)
    sol, _, rank, _ = np.linalg.lstsq(t, image, rcond=None)
    if rank < N_TERMS:
        raise ValueError(f"the calibration points determine only {rank} of the {N_TERMS} terms")
    cam = camera(centre, scale, sol[:, 0], sol[:, 1])
    res = np.linalg.norm(map_points(cam, world) - image, axis=-1)
    return cam, float(np.sqrt(np.mean(res * res))), float(res.max())


def jacobian(cam, P) -> np.ndarray:
    """The analytic d(x, y) / d(X, Y, Z) [..., 2, 3] at the world points P [..., 3], in section 19b's operation order."""
    q = _normalised(cam, P)
    X, Y, Z = q[..., 0], q[..., 1], q[..., 2]
    o, l = np.zeros_like(X), np.ones_like(X)
    XX, YY, ZZ, X2, Y2, Z2 = X * X, Y * Y, Z * Z, 2.0 * X, 2.0 * Y, 2.0 * Z
    D = ((o, l, o, o, X2, Y, o, Z, o, o, 3.0 * XX, X2 * Y, YY, o, X2 * Z, Y * Z, o, ZZ, o),
         (o, o, l, o, o, X, Y2, o, Z, o, o, XX, X2 * Y, 3.0 * YY, o, X * Z, Y2 * Z, o, ZZ),
         (o, o, o, l, o, o, o, X, Y, Z2, o, o, o, o, XX, X * Y, YY, X2 * Z, Y2 * Z))
    J = np.empty(X.shape + (2, 3))
    for axis in range(3):
        sx, sy = o, o
        for k in range(N_TERMS):
            sx = sx + cam["cx"][k] * D[axis][k]
            sy = sy + cam["cy"][k] * D[axis][k]
        J[..., 0, axis] = sx / cam["scale"][axis]
        J[..., 1, axis] = sy / cam["scale"][axis]
    return J


# ---- the plane -----------------------------------------------------------------------------------------------------------------
def plane(x0, y0, pitch, z, width, height) -> dict:
    p = dict(x0=float(x0), y0=float(y0), pitch=float(pitch), z=float(z), width=int(width), height=int(height))
    if not all(np.isfinite(p[k]) for k in ("x0", "y0", "pitch", "z")) or p["pitch"] <= 0 or p["width"] < 1 or p["height"] < 1:
        raise ValueError("a plane needs finite x0, y0, z, a pitch > 0 and a size >= 1")
    return p


def centred_plane(width: int, height: int, pitch: float, z: float = 0.0) -> dict:
    """The plane whose grid is centred on the world origin."""
    return plane(-(int(width) - 1) / 2.0 * pitch, -(int(height) - 1) / 2.0 * pitch, pitch, z, width, height)


def plane_points(pl, rows=None, cols=None) -> np.ndarray:
    """World points [len(rows), len(cols), 3] of the dewarped pixels (rows x cols; None: all; fractions allowed)."""
    rows = np.arange(pl["height"], dtype=np.float64) if rows is None else np.asarray(rows, np.float64)
    cols = np.arange(pl["width"], dtype=np.float64) if cols is None else np.asarray(cols, np.float64)
    P = np.empty((rows.size, cols.size, 3))
    P[..., 0] = (pl["x0"] + cols * pl["pitch"])[None, :]
    P[..., 1] = (pl["y0"] + rows * pl["pitch"])[:, None]
    P[..., 2] = pl["z"]
    return P


def window_centres(pl, win: int, step: int) -> np.ndarray:
    """World points [n_rows, n_cols, 3] of the window centres of section 5's grid on the plane, as section 19b takes them."""
    n_rows, n_cols = pc.grid_shape((pl["height"], pl["width"]), win, step)
    half = (int(win) - 1) / 2.0
    P = np.empty((n_rows, n_cols, 3))
    P[..., 0] = (pl["x0"] + (np.arange(n_cols) * int(step) + half) * pl["pitch"])[None, :]
    P[..., 1] = (pl["y0"] + (np.arange(n_rows) * int(step) + half) * pl["pitch"])[:, None]
    P[..., 2] = pl["z"]
    return P


def plane_coefficients(cam, pl):
    """The camera folded at the plane's z and grid, as photon_piv_dewarp takes it (section 19a's arithmetic and order):
    (poly f64 [2, 10], the bivariate cubics of x and y in (u, v) = the normalised (X, Y); grid f64 [4] = u0, du, v0, dv with
    u = u0 + j du at column j and v = v0 + i dv at row i)."""
    w = (pl["z"] - cam["centre"][2]) / cam["scale"][2]
    poly = np.empty((2, 10))
    for n, c in enumerate((cam["cx"], cam["cy"])):
        poly[n] = [(c[9] * w + c[3]) * w + c[0], (c[17] * w + c[7]) * w + c[1], (c[18] * w + c[8]) * w + c[2], c[14] * w + c[4],
                   c[15] * w + c[5], c[16] * w + c[6], c[10], c[11], c[12], c[13]]
    grid = np.array([(pl["x0"] - cam["centre"][0]) / cam["scale"][0], pl["pitch"] / cam["scale"][0],
                     (pl["y0"] - cam["centre"][1]) / cam["scale"][1], pl["pitch"] / cam["scale"][1]])
    return poly, grid


def _cubic(k, u, v):
    a0 = ((k[9] * v + k[5]) * v + k[2]) * v + k[0]
    a1 = (k[8] * v + k[4]) * v + k[1]
    a2 = k[7] * v + k[3]
    return ((k[6] * u + a2) * u + a1) * u + a0


def folded_points(poly, grid, out_shape):
    """(x, y), f64 [out_height, out_width]: the source coordinates of every output pixel, in the kernel's f64 operations."""
    poly, grid = np.asarray(poly, np.float64), np.asarray(grid, np.float64)
    oh, ow = (int(v) for v in out_shape)
    u = (grid[0] + np.arange(ow, dtype=np.float64) * grid[1])[None, :]
    v = (grid[2] + np.arange(oh, dtype=np.float64) * grid[3])[:, None]
    with np.errstate(all="ignore"):
        return np.broadcast_to(_cubic(poly[0], u, v), (oh, ow)), np.broadcast_to(_cubic(poly[1], u, v), (oh, ow))


def outside_mask(poly, grid, out_shape, shape) -> np.ndarray:
    """bool [out_height, out_width]: the output pixels whose source coordinate is not within [0, width - 1] x [0, height - 1]
    of a source of `shape` (height, width) -- NaN included --, decided as the kernel decides it."""
    x, y = folded_points(poly, grid, out_shape)
    with np.errstate(invalid="ignore"):
        return ~((x >= 0.0) & (x <= shape[1] - 1.0) & (y >= 0.0) & (y <= shape[0] - 1.0))


# ---- the dewarp ----------------------------------------------------------------------------------------------------------------
def _bspline_weights_f32(t):
    one, two, three, four, sixth = (np.float32(v) for v in (1, 2, 3, 4, np.float32(1) / np.float32(6)))
    u = one - t
    t2, u2 = t * t, u * u
    return [u2 * u * sixth, (four - three * t2 * (two - t)) * sixth, (four - three * u2 * (two - u)) * sixth, t2 * t * sixth]


def _stack(a, dtype):
    a = np.asarray(a, dtype)
    if a.ndim not in (2, 3):
        raise ValueError("frames must be [height, width] or [n, height, width]")
    return a.reshape((-1,) + a.shape[-2:]), a.ndim == 2


def sensor_points(poly, grid, out_shape, shape):
    """Where every output pixel lands on a source of `shape` (height, width), as piv_camera.hpp's sensor_point decides it:
    (inside bool, ix, iy int64 = floor(x), floor(y), tx, ty f64 = x - floor(x), y - floor(y)), each [out_height, out_width]; a
    pixel outside (NaN included) holds what (0, 0) gives.  The dewarp's taps and piv_mart's footprint both start here."""
    x, y = folded_points(poly, grid, out_shape)
    inside = ~outside_mask(poly, grid, out_shape, shape)
    x, y = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    fx, fy = np.floor(x), np.floor(y)
    return inside, fx.astype(np.int64), fy.astype(np.int64), x - fx, y - fy


def _taps(poly, grid, out_shape, shape):
    h, w = shape
    inside, ix, iy, tx, ty = sensor_points(poly, grid, out_shape, shape)
    return inside, tx, ty, [pd.mirror_index(ix - 1 + t, w) for t in range(4)], [pd.mirror_index(iy - 1 + t, h) for t in range(4)]


def bspline_sample(c, tx, ty, xi, yi):
    """The 16-tap sum in f64 at _taps' fractions and indices, rows in order, each summed left to right: c [..., height, width]."""
    wx, wy = pd._bspline_weights(tx), pd._bspline_weights(ty)
    acc = np.zeros(c.shape[:-2] + tx.shape)
    for t in range(4):
        acc = acc + wy[t] * (((wx[0] * c[..., yi[t], xi[0]] + wx[1] * c[..., yi[t], xi[1]]) + wx[2] * c[..., yi[t], xi[2]]) + wx[3] * c[..., yi[t], xi[3]])
    return acc


def dewarp_model_f32(coef, poly, grid, out_shape):
    """Host model of photon_piv_dewarp in the kernel's own operations, f64 for the coordinate and f32 behind the fraction:
    coef f32 [n, height, width] or [height, width] (section 7a's coefficients), poly and grid from plane_coefficients.
    Returns (frames f32 [n, out_height, out_width] or [out_height, out_width], mask u8 [out_height, out_width], 1 = outside
    the source).  The device returns these bits."""
    c, single = _stack(coef, np.float32)
    inside, tx, ty, xi, yi = _taps(poly, grid, out_shape, c.shape[-2:])
    wx, wy = _bspline_weights_f32(tx.astype(np.float32)), _bspline_weights_f32(ty.astype(np.float32))
    out = np.zeros((c.shape[0],) + tuple(inside.shape), np.float32)
    for f in range(c.shape[0]):
        acc = np.zeros(inside.shape, np.float32)
        for t in range(4):
            s = ((wx[0] * c[f][yi[t], xi[0]] + wx[1] * c[f][yi[t], xi[1]]) + wx[2] * c[f][yi[t], xi[2]]) + wx[3] * c[f][yi[t], xi[3]]
            acc = acc + wy[t] * s
        out[f] = np.where(inside, acc, np.float32(0))
    return (out[0] if single else out), (~inside).astype(np.uint8)


def dewarp_model(frames, poly, grid, out_shape):
    """The dewarp in f64 throughout, from the frames themselves ([n, height, width] or [height, width]) through
    piv_deformation.bspline_coefficients_model: (frames f64, mask u8) shaped as dewarp_model_f32's."""
    a, single = _stack(frames, np.float64)
    inside, tx, ty, xi, yi = _taps(poly, grid, out_shape, a.shape[-2:])
    out = np.zeros((a.shape[0],) + tuple(inside.shape))
    for f in range(a.shape[0]):
        out[f] = np.where(inside, bspline_sample(pd.bspline_coefficients_model(a[f]), tx, ty, xi, yi), 0.0)
    return (out[0] if single else out), (~inside).astype(np.uint8)


# ---- the reconstruction --------------------------------------------------------------------------------------------------------
def _solve(L, r):
    l00, l10, l20, l11, l21, l22 = L
    y0 = r[0] / l00
    y1 = (r[1] - l10 * y0) / l11
    y2 = ((r[2] - l20 * y0) - l21 * y1) / l22
    z2 = y2 / l22
    z1 = (y1 - l21 * z2) / l11
    return ((y0 - l10 * z1) - l20 * z2) / l00, z1, z2


def reconstruct_model(field1, field2, cameras, pl, win: int, step: int, flags1=None, flags2=None, sigma1=None, sigma2=None):
    """Host model of photon_piv_stereo_reconstruct, operation by operation (section 19b).  field1, field2 [n_rows, n_cols, >= 2]
    (dx, dy first, dewarped pixels; taken as given -- the device reads f32) on section 5's grid of the plane; flags int
    [n_rows, n_cols] or None; sigma [n_rows, n_cols, 2] both or neither.  Returns (out f64 [n_rows, n_cols, 8] = dX, dY, dZ, residual, sigma_X, sigma_Y, sigma_Z,
    pivot ratio; flags int32 [n_rows, n_cols] with 64 = degenerate and 128 = a vector that is not finite)."""
    grid = pc.grid_shape((pl["height"], pl["width"]), win, step)
    f = [np.asarray(x, np.float64)[..., :2] for x in (field1, field2)]
    if any(x.shape != grid + (2,) for x in f):
        raise ValueError(f"the fields must be [{grid[0]}, {grid[1]}, >= 2]: the grid of the plane, win {win}, step {step}")
    if (sigma1 is None) != (sigma2 is None):
        raise ValueError("sigma1 and sigma2 come together or not at all")
    P, pitch = window_centres(pl, win, step), pl["pitch"]
    J = [jacobian(cam, P) for cam in cameras]
    A = [J[c][..., r, :] for c in range(2) for r in range(2)]                      # 4 rows of [n_rows, n_cols, 3]
    with np.errstate(all="ignore"):
        b = [J[c][..., r, 0] * (pitch * f[c][..., 0]) + J[c][..., r, 1] * (pitch * f[c][..., 1]) for c in range(2) for r in range(2)]
        N = [[((A[0][..., p] * A[0][..., q] + A[1][..., p] * A[1][..., q]) + A[2][..., p] * A[2][..., q]) + A[3][..., p] * A[3][..., q]
              for q in range(3)] for p in range(3)]
        r = [((A[0][..., p] * b[0] + A[1][..., p] * b[1]) + A[2][..., p] * b[2]) + A[3][..., p] * b[3] for p in range(3)]
        d0 = N[0][0]
        l00 = np.sqrt(d0)
        l10, l20 = N[1][0] / l00, N[2][0] / l00
        d1 = N[1][1] - l10 * l10
        l11 = np.sqrt(d1)
        l21 = (N[2][1] - l20 * l10) / l11
        d2 = (N[2][2] - l20 * l20) - l21 * l21
        L = (l00, l10, l20, l11, l21, np.sqrt(d2))
        ratio = np.minimum(np.minimum(d0, d1), d2) / np.maximum(np.maximum(d0, d1), d2)
        good = (ratio > MIN_PIVOT_RATIO) & (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0)
        D = _solve(L, r)
        ss = np.zeros(grid)
        for m in range(4):
            e = ((A[m][..., 0] * D[0] + A[m][..., 1] * D[1]) + A[m][..., 2] * D[2]) - b[m]
            ss = ss + e * e
        out = np.full(grid + (8,), np.nan)
        out[..., 0], out[..., 1], out[..., 2], out[..., 3], out[..., 7] = D[0], D[1], D[2], np.sqrt(ss), ratio
        if sigma1 is not None:
            sg = [np.asarray(s, np.float64) for s in (sigma1, sigma2)]
            one, zero = np.ones(grid), np.zeros(grid)
            inv = [_solve(L, [one if p == col else zero for p in range(3)]) for col in range(3)]
            var = [np.zeros(grid) for _ in range(3)]
            for c in range(2):
                s = [pitch * sg[c][..., 0], pitch * sg[c][..., 1]]
                for p in range(3):
                    M = [(inv[0][p] * A[2 * c + rr][..., 0] + inv[1][p] * A[2 * c + rr][..., 1]) + inv[2][p] * A[2 * c + rr][..., 2]
                         for rr in range(2)]
                    for m in range(2):
                        g = M[0] * J[c][..., 0, m] + M[1] * J[c][..., 1, m]
                        var[p] = var[p] + (g * g) * (s[m] * s[m])
            for p in range(3):
                out[..., 4 + p] = np.sqrt(var[p])
    finite = np.isfinite(f[0]).all(axis=-1) & np.isfinite(f[1]).all(axis=-1)
    out[~finite, :7] = np.nan
    out[~good] = np.nan
    flags = np.zeros(grid, np.int32)
    for x in (flags1, flags2):
        if x is not None:
            flags |= np.asarray(x, np.int32)
    flags |= np.where(good, 0, FLAG_DEGENERATE).astype(np.int32) | np.where(finite, 0, FLAG_NOT_FINITE).astype(np.int32)
    return out, flags


def correlate_stereo_model(cam1_frames, cam2_frames, cameras, pl, win: int = 32, step: int = 16, radius=None, iterations: int = 3):
    """Host model of PhotonLibrary.correlate_stereo with evaluate="deform" in f64: dewarp_model per camera,
    piv_deformation.correlate_deform_model on each dewarped pair (under the dewarp mask where a pixel is outside), then
    reconstruct_model.  Returns (out [n_rows, n_cols, 8], flags, (vectors1, vectors2))."""
    shape = (pl["height"], pl["width"])
    vectors, status = [], []
    for cam, frames in zip(cameras, (cam1_frames, cam2_frames)):
        d, mask = dewarp_model(frames, *plane_coefficients(cam, pl), shape)
        v, s = pd.correlate_deform_model(d[0], d[1], win, step, radius, iterations, mask=mask if mask.any() else None)
        vectors.append(v)
        status.append(s)
    out, flags = reconstruct_model(vectors[0], vectors[1], cameras, pl, win, step, status[0], status[1])
    return out, flags, tuple(vectors)


# ---- self-calibration: the sheet from the disparity of the two views (section 19c) ---------------------------------------------
UNUSABLE = pc.FLAG_EDGE_PEAK | pc.FLAG_FLAT | 16 | FLAG_DEGENERATE | FLAG_NOT_FINITE       # 16: masked out; bit 4 (outside) stays in
MAX_TRIANGULATE_ITERATIONS = 16


def _image(cam, P):
    """(x, y) of the world points P [..., 3] in section 19c's order: each coordinate summed from 0.0 over the 19 terms."""
    t = _terms(_normalised(cam, P))
    x = y = np.zeros(t.shape[:-1])
    for k in range(N_TERMS):
        x = x + cam["cx"][k] * t[..., k]
        y = y + cam["cy"][k] * t[..., k]
    return x, y


def triangulate_model(disparity, cameras, pl, win: int, step: int, iterations: int, flags=None):
    """Host model of photon_piv_stereo_triangulate, operation by operation (section 19c).  disparity [n_rows, n_cols, >= 2]
    (dx, dy first: the displacement from camera 1's dewarped frame to camera 2's of the same instant, in dewarped pixels;
    taken as given -- the device reads f32) on section 5's grid of the plane; flags int [n_rows, n_cols] or None.  Returns
    (out f64 [n_rows, n_cols, 6] = X, Y, Z of the world point both cameras saw, the triangulation error in image pixels, the
    length of the last Gauss-Newton step in world units, the smallest pivot ratio of the iterations; flags int32 with 64 = an
    iteration was degenerate and 128 = dx or dy not finite, the first five outputs NaN for either)."""
    grid = pc.grid_shape((pl["height"], pl["width"]), win, step)
    d = np.asarray(disparity, np.float64)[..., :2]
    if d.shape != grid + (2,):
        raise ValueError(f"the disparity must be [{grid[0]}, {grid[1]}, >= 2]: the grid of the plane, win {win}, step {step}")
    if not 1 <= int(iterations) <= MAX_TRIANGULATE_ITERATIONS:
        raise ValueError(f"iterations must be within [1, {MAX_TRIANGULATE_ITERATIONS}]")
    if len(cameras) != 2:
        raise ValueError("the triangulation takes two cameras")
    P, pitch = window_centres(pl, win, step), pl["pitch"]
    finite = np.isfinite(d).all(axis=-1)
    with np.errstate(all="ignore"):
        hx, hy = (pitch / 2.0) * d[..., 0], (pitch / 2.0) * d[..., 1]
        P1, P2 = P.copy(), P.copy()
        P1[..., 0], P1[..., 1] = P[..., 0] - hx, P[..., 1] - hy
        P2[..., 0], P2[..., 1] = P[..., 0] + hx, P[..., 1] + hy
        x = (*_image(cameras[0], P1), *_image(cameras[1], P2))                      # x1, y1, x2, y2

        def residual(W):
            m = (*_image(cameras[0], W), *_image(cameras[1], W))
            return [x[k] - m[k] for k in range(4)]

        W = P.copy()
        alive, good = finite.copy(), np.ones(grid, bool)         # alive: still iterating; a node that is not keeps what it has
        lowest = np.full(grid, np.nan)
        s = [np.full(grid, np.nan) for _ in range(3)]
        for it in range(int(iterations)):
            todo = alive | ((it == 0) & ~finite)                                    # a vector that is not finite: the start point's ratio
            r = residual(W)
            J = [jacobian(cam, W) for cam in cameras]
            A = [J[c][..., q, :] for c in range(2) for q in range(2)]
            N = [[((A[0][..., p] * A[0][..., q] + A[1][..., p] * A[1][..., q]) + A[2][..., p] * A[2][..., q]) + A[3][..., p] * A[3][..., q]
                  for q in range(3)] for p in range(3)]
            g = [((A[0][..., p] * r[0] + A[1][..., p] * r[1]) + A[2][..., p] * r[2]) + A[3][..., p] * r[3] for p in range(3)]
            d0 = N[0][0]
            l00 = np.sqrt(d0)
            l10, l20 = N[1][0] / l00, N[2][0] / l00
            d1 = N[1][1] - l10 * l10
            l11 = np.sqrt(d1)
            l21 = (N[2][1] - l20 * l10) / l11
            d2 = (N[2][2] - l20 * l20) - l21 * l21
            ratio = np.minimum(np.minimum(d0, d1), d2) / np.maximum(np.maximum(d0, d1), d2)
            ok = (ratio > MIN_PIVOT_RATIO) & (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0)
            lowest = np.where(todo, np.where(ok & (it > 0), np.where(ratio < lowest, ratio, lowest), ratio), lowest)
            good &= ~(todo & ~ok)
            alive &= ok
            ds = _solve((l00, l10, l20, l11, l21, np.sqrt(d2)), g)
            for p in range(3):
                s[p] = np.where(alive, ds[p], s[p])
                W[..., p] = np.where(alive, W[..., p] + ds[p], W[..., p])
        r = residual(W)
        ss = np.zeros(grid)
        for m in range(4):
            ss = ss + r[m] * r[m]
        out = np.full(grid + (6,), np.nan)
        out[..., :3], out[..., 3], out[..., 4], out[..., 5] = W, np.sqrt(ss), np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]), lowest
    out[~(finite & good), :5] = np.nan
    result = np.zeros(grid, np.int32) if flags is None else np.array(flags, np.int32)
    result |= np.where(good, 0, FLAG_DEGENERATE).astype(np.int32) | np.where(finite, 0, FLAG_NOT_FINITE).astype(np.int32)
    return out, result


def usable_nodes(flags) -> np.ndarray:
    """bool: the nodes the sheet fit may use -- none of the bits 1 (edge peak), 2 (flat), 16 (masked out), 64, 128."""
    return (np.asarray(flags) & UNUSABLE) == 0


def fit_sheet(points, flags, error=None):
    """Z = a + b X + c Y by least squares over the usable nodes (usable_nodes; finite X, Y, Z) of points [..., >= 3] with
    flags [...]: three fixed rounds of rejection, each dropping the nodes whose residual lies more than 3 x 1.4826 x MAD
    from the residuals' median (differences at rounding level, 1e-12 of the coordinates, never count), then the final fit.  error [...] (the triangulation error, optional): a node whose error
    is not finite is left out from the start.
    Returns ((a, b, c), rms residual, nodes used); raises ValueError when fewer than 6 nodes remain or X or Y has no spread."""
    pts = np.asarray(points, np.float64)
    pts = pts.reshape(-1, pts.shape[-1])[:, :3]
    keep = usable_nodes(flags).reshape(-1) & np.isfinite(pts).all(axis=-1)
    if keep.shape[0] != pts.shape[0]:
        raise ValueError("points and flags must describe the same nodes")
    if error is not None:
        keep &= np.isfinite(np.asarray(error, np.float64).reshape(-1))

    def fit(sel):
        if sel.sum() < 6:
            raise ValueError(f"the sheet fit needs at least 6 usable nodes, {int(sel.sum())} remain")
        X, Y, Z = pts[sel].T
        if np.ptp(X) == 0.0 or np.ptp(Y) == 0.0:
            raise ValueError("the usable nodes have no spread in X or in Y: no sheet can be fitted")
        mx, my = X.mean(), Y.mean()
        sol = np.linalg.lstsq(np.stack([np.ones_like(X), X - mx, Y - my], axis=-1), Z, rcond=None)[0]
        abc = np.array([sol[0] - sol[1] * mx - sol[2] * my, sol[1], sol[2]])
        return abc, pts[:, 2] - (abc[0] + abc[1] * pts[:, 0] + abc[2] * pts[:, 1])

    floor = 1e-12 * (1.0 + float(np.abs(pts[keep]).max())) if keep.any() else 0.0          # rounding is no outlier: exact points have MAD 0
    for _ in range(3):
        abc, res = fit(keep)
        med = np.median(res[keep])
        keep = keep & (np.abs(res - med) <= max(3.0 * 1.4826 * np.median(np.abs(res[keep] - med)), floor))
    abc, res = fit(keep)
    return (float(abc[0]), float(abc[1]), float(abc[2])), float(np.sqrt(np.mean(res[keep] ** 2))), int(keep.sum())


def sheet_frame(sheet, pl):
    """(R, O, C) of coordinates in which the sheet Z = a + b X + c Y is the plane's own z: e3 = (-b, -c, 1) normalised, e1 =
    the world X axis minus its part along e3, normalised, e2 = e3 x e1, R = [e1 e2 e3] as columns; C = the plane's centre (x_c,
    y_c, z), O = (x_c, y_c, a + b x_c + c y_c).  A point W' of the new coordinates is the old world point O + R (W' - C)."""
    a, b, c = (float(v) for v in sheet)
    e3 = np.array([-b, -c, 1.0])
    e3 /= np.linalg.norm(e3)
    e1 = np.array([1.0, 0.0, 0.0]) - e3[0] * e3
    e1 /= np.linalg.norm(e1)
    R = np.stack([e1, np.cross(e3, e1), e3], axis=1)
    xc, yc = pl["x0"] + (pl["width"] - 1) / 2.0 * pl["pitch"], pl["y0"] + (pl["height"] - 1) / 2.0 * pl["pitch"]
    return R, np.array([xc, yc, a + b * xc + c * yc]), np.array([xc, yc, pl["z"]])


def to_world(frame, P) -> np.ndarray:
    """The old world points O + R (P - C) of the points P [..., 3] given in a frame (R, O, C)."""
    R, O, C = frame
    return O + (np.asarray(P, np.float64) - C) @ np.asarray(R).T


def compose_frames(outer, inner):
    """The frame that takes `inner`'s coordinates to `outer`'s world: O1 + R1 (O2 + R2 (W - C) - C) = (O1 + R1 (O2 - C)) + R1 R2 (W - C)."""
    (R1, O1, C), (R2, O2, _) = outer, inner
    return R1 @ R2, O1 + R1 @ (O2 - C), C


def frame_sheet(frame):
    """(a, b, c) of the plane Z' = z of a frame (R, O, C), in the world the frame maps to."""
    R, O, _ = frame
    b, c = -R[0, 2] / R[2, 2], -R[1, 2] / R[2, 2]
    return float(O[2] - b * O[0] - c * O[1]), float(b), float(c)


def move_camera(cam, R, O, C, pl):
    """The camera in the coordinates of the frame (R, O, C): fit_camera on calibration_target(pl, 9, (-1, 0, 1)) against the
    camera's images of the old world points O + R (target - C).  Returns (camera, rms, max) as fit_camera does: the refit's
    residual says whether the moved camera is still within the 19-term family."""
    target = calibration_target(pl, 9, (-1.0, 0.0, 1.0))
    return fit_camera(target, map_points(cam, to_world((R, O, C), target)))


def windows_touching(mask, win: int, step: int) -> np.ndarray:
    """bool [n_rows, n_cols]: the windows of section 5's grid that hold a nonzero pixel of mask [height, width]."""
    mask = np.asarray(mask) != 0
    n_rows, n_cols = pc.grid_shape(mask.shape, win, step)
    return np.array([[mask[i * step:i * step + win, j * step:j * step + win].any() for j in range(n_cols)] for i in range(n_rows)])


def selfcal_round(points, flags, disparity, outside, cameras, pl, win: int, step: int):
    """The host half of one self-calibration round, shared by the model and the device driver: the nodes whose window
    touches a pixel that is outside either camera (outside: the two dewarp masks) leave with flag 16; fit_sheet on the rest;
    sheet_frame; move_camera on both cameras.  Returns (cameras, frame (R, O, C), the round's report entry)."""
    flags = np.array(flags, np.int32)
    for mask in outside:
        flags[windows_touching(mask, win, step)] |= 16
    points, d = np.asarray(points, np.float64), np.asarray(disparity, np.float64)[..., :2]
    ok = usable_nodes(flags) & np.isfinite(points[..., :5]).all(axis=-1)
    if not ok.any():
        raise ValueError("self-calibration: no usable disparity vector")
    sheet, rms, used = fit_sheet(points, flags, points[..., 3])
    frame = sheet_frame(sheet, pl)
    moved = [move_camera(cam, *frame, pl) for cam in cameras]
    entry = dict(disparity_rms=float(np.sqrt(np.mean(d[ok] ** 2))), sheet=sheet, sheet_rms=rms, nodes=used,
                 error_median=float(np.median(points[..., 3][ok])), step_max=float(points[..., 4][ok].max()),
                 refit=tuple((m[1], m[2]) for m in moved))
    return tuple(m[0] for m in moved), frame, entry


def selfcal_report(entries, frame) -> dict:
    """What self-calibration returns beside the cameras: the rounds' entries, the accumulated frame (R, O, C) from the final
    coordinates to the original calibration's world, and the sheet that frame describes in that world."""
    return dict(rounds=list(entries), R=frame[0], O=frame[1], C=frame[2], sheet=frame_sheet(frame))


def identity_frame(pl):
    return sheet_frame((pl["z"], 0.0, 0.0), pl)


def self_calibrate_model(cam1_frames, cam2_frames, cameras, pl, win: int = 64, step: int = 32, radius=None, rounds: int = 3,
                         iterations: int = 4, tolerance: float = 0.05):
    """Host model of PhotonLibrary.self_calibrate_stereo in f64.  cam1_frames, cam2_frames [N, height, width]: frame k of both
    is the same instant.  Per round, with the current cameras: dewarp_model per camera, piv_ensemble.correlate_ensemble_model
    of the two dewarped stacks (the disparity field), triangulate_model, selfcal_round; the rounds end early once the rms
    disparity of the usable nodes is below `tolerance` px (that round's correction is still applied).  Returns (cameras,
    report): report["rounds"][k] = disparity_rms, sheet (a, b, c) in that round's coordinates, sheet_rms, nodes,
    error_median, step_max, refit ((rms, max) per camera); report["R"], ["O"], ["C"] the accumulated frame and
    report["sheet"] the sheet in the original calibration's world."""
    from . import piv_ensemble as pe
    radius = int(win) // 2 if radius is None else int(radius)
    if int(rounds) < 1:
        raise ValueError("rounds must be >= 1")
    shape = (pl["height"], pl["width"])
    cameras, frame, entries = tuple(cameras), identity_frame(pl), []
    for _ in range(int(rounds)):
        dewarped = [dewarp_model(f, *plane_coefficients(cam, pl), shape) for cam, f in zip(cameras, (cam1_frames, cam2_frames))]
        vectors, status, _ = pe.correlate_ensemble_model(dewarped[0][0], dewarped[1][0], win, step, radius)
        points, flags = triangulate_model(vectors, cameras, pl, win, step, iterations, status)
        cameras, moved, entry = selfcal_round(points, flags, vectors, (dewarped[0][1], dewarped[1][1]), cameras, pl, win, step)
        frame = compose_frames(frame, moved)
        entries.append(entry)
        if entry["disparity_rms"] < tolerance:
            break
    return cameras, selfcal_report(entries, frame)


# ---- generators ----------------------------------------------------------------------------------------------------------------
class Pinhole:
    """A perspective camera to calibrate against: it sits `distance` from the world origin, rotated by theta about the Y
    axis and raised by phi (radians), looks at the origin, and images it at the sensor's centre + offset (x, y) with
    `px_per_mm` pixels per world unit there.  shape: the sensor (height, width)."""

    def __init__(self, theta, phi, distance, px_per_mm, shape, offset=(0.0, 0.0)):
        self.shape = (int(shape[0]), int(shape[1]))
        self.position = distance * np.array([np.sin(theta) * np.cos(phi), np.sin(phi), np.cos(theta) * np.cos(phi)])
        self.forward = -self.position / distance
        self.right = np.cross([0.0, 1.0, 0.0], -self.forward)
        self.right /= np.linalg.norm(self.right)
        self.up = np.cross(-self.forward, self.right)
        self.focal = float(px_per_mm) * float(distance)
        self.principal = np.array([(self.shape[1] - 1) / 2.0 + offset[0], (self.shape[0] - 1) / 2.0 + offset[1]])

    def project(self, P) -> np.ndarray:
        v = np.asarray(P, np.float64) - self.position
        depth = v @ self.forward
        return np.stack([self.principal[0] + self.focal * (v @ self.right) / depth, self.principal[1] + self.focal * (v @ self.up) / depth], axis=-1)


def pinhole(theta, phi, distance, px_per_mm, shape, offset=(0.0, 0.0)) -> Pinhole:
    return Pinhole(theta, phi, distance, px_per_mm, shape, offset)


def calibration_target(pl, n: int = 9, z=(-1.0, 0.0, 1.0), margin: float = 0.05) -> np.ndarray:
    """World points [n n len(z), 3] of a dot target that covers the plane (and `margin` of its size beyond) at the offsets z
    from the plane's own."""
    xs = pl["x0"] + np.linspace(-margin, 1.0 + margin, n) * (pl["width"] - 1) * pl["pitch"]
    ys = pl["y0"] + np.linspace(-margin, 1.0 + margin, n) * (pl["height"] - 1) * pl["pitch"]
    X, Y, Z = np.meshgrid(xs, ys, pl["z"] + np.asarray(z, np.float64), indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=-1)


def _project(cam, P):
    return cam.project(P) if hasattr(cam, "project") else map_points(cam, P)


def _render(xy, amplitude, shape, diameter, reach: int = 4) -> np.ndarray:
    """Gaussian particle images of e^-2 diameter `diameter` px at the image points xy [n, 2], sampled at the pixel centres."""
    h, w = shape
    img = np.zeros((h, w))
    cx, cy = np.rint(xy[:, 0]).astype(np.int64), np.rint(xy[:, 1]).astype(np.int64)
    for oy in range(-reach, reach + 1):
        for ox in range(-reach, reach + 1):
            ix, iy = cx + ox, cy + oy
            ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
            r2 = (ix[ok] - xy[ok, 0]) ** 2 + (iy[ok] - xy[ok, 1]) ** 2
            np.add.at(img, (iy[ok], ix[ok]), amplitude[ok] * np.exp(-8.0 * r2 / diameter ** 2))
    return img


def particle_pair(cameras, flow, pl, seed: int, shape=(224, 256), density: float = 0.035, diameter: float = 2.5,
                  sheet_sigma: float = 0.75, margin: float = 4.0):
    """Two exposures per camera of particles that move with `flow`: particles scattered uniformly in the slab of the plane
    (`margin` world units beyond its sides, 2.5 sheet_sigma to either side of its z; `density` per dewarped pixel of the
    plane), particle k at P_k - flow(P_k) / 2 in the first exposure and P_k + flow(P_k) / 2 in the second, lit by a Gaussian
    sheet profile exp(-(Z - z)^2 / (2 sheet_sigma^2)) at its position in each exposure, imaged as a Gaussian of e^-2 diameter
    `diameter` px through each of `cameras` (Pinhole objects or fitted cameras).  flow(P [n, 3]) -> [n, 3] world units.
    Returns one f32 stack [2, height, width] per camera."""
    rng = np.random.default_rng(seed)
    lo = np.array([pl["x0"] - margin, pl["y0"] - margin, pl["z"] - 2.5 * sheet_sigma])
    hi = np.array([pl["x0"] + (pl["width"] - 1) * pl["pitch"] + margin, pl["y0"] + (pl["height"] - 1) * pl["pitch"] + margin,
                   pl["z"] + 2.5 * sheet_sigma])
    n = int(round(density * (hi[0] - lo[0]) * (hi[1] - lo[1]) / pl["pitch"] ** 2))
    P = rng.uniform(lo, hi, (n, 3))
    brightness = rng.uniform(0.5, 1.0, n)
    half = 0.5 * np.asarray(flow(P), np.float64)
    out = []
    for cam in cameras:
        frames = []
        for Q in (P - half, P + half):
            lit = brightness * np.exp(-((Q[:, 2] - pl["z"]) ** 2) / (2.0 * sheet_sigma ** 2))
            frames.append(_render(_project(cam, Q), lit, shape, diameter))
        out.append(np.stack(frames).astype(np.float32))
    return tuple(out)


def _sheet_particles(rng, pl, sheet, density, sheet_sigma, margin):
    """Particles scattered uniformly over the plane's extent (`margin` beyond its sides) within 2.5 sheet_sigma of the sheet
    Z = a + b X + c Y, `density` per dewarped pixel: (P [n, 3], brightness [n])."""
    a, b, c = sheet
    lo = np.array([pl["x0"] - margin, pl["y0"] - margin])
    hi = np.array([pl["x0"] + (pl["width"] - 1) * pl["pitch"] + margin, pl["y0"] + (pl["height"] - 1) * pl["pitch"] + margin])
    n = int(round(density * (hi[0] - lo[0]) * (hi[1] - lo[1]) / pl["pitch"] ** 2))
    XY = rng.uniform(lo, hi, (n, 2))
    Z = a + b * XY[:, 0] + c * XY[:, 1] + rng.uniform(-2.5 * sheet_sigma, 2.5 * sheet_sigma, n)
    return np.concatenate([XY, Z[:, None]], axis=1), rng.uniform(0.5, 1.0, n)


def _sheet_light(Q, sheet, sheet_sigma):
    a, b, c = sheet
    return np.exp(-((Q[:, 2] - (a + b * Q[:, 0] + c * Q[:, 1])) ** 2) / (2.0 * sheet_sigma ** 2))


def sheet_frames(cameras, pl, sheet, n_frames: int, seed: int, shape=(224, 256), density: float = 0.035, diameter: float = 2.5,
                 sheet_sigma: float = 0.3, margin: float = 4.0):
    """n_frames simultaneous single exposures per camera of particles in a Gaussian sheet around Z = a + b X + c Y (sheet =
    (a, b, c), in the cameras' world): every instant has its own particles, lit by exp(-(Z - sheet(X, Y))^2 / (2
    sheet_sigma^2)) and imaged as particle_pair images them.  What self-calibration takes: frame k of both cameras shows the
    same particles.  Returns one f32 stack [n_frames, height, width] per camera."""
    rng = np.random.default_rng(seed)
    out = [[] for _ in cameras]
    for _ in range(int(n_frames)):
        P, brightness = _sheet_particles(rng, pl, sheet, density, sheet_sigma, margin)
        lit = brightness * _sheet_light(P, sheet, sheet_sigma)
        for frames, cam in zip(out, cameras):
            frames.append(_render(_project(cam, P), lit, shape, diameter))
    return tuple(np.stack(frames).astype(np.float32) for frames in out)


def sheet_pair(cameras, flow, pl, sheet, seed: int, shape=(224, 256), density: float = 0.035, diameter: float = 2.5,
               sheet_sigma: float = 0.3, margin: float = 4.0):
    """particle_pair on a sheet that is not the plane: two exposures per camera of particles around Z = a + b X + c Y that
    move with `flow`, particle k at P_k - flow(P_k) / 2 and P_k + flow(P_k) / 2, lit by the sheet's profile at its position
    in each exposure.  Returns one f32 stack [2, height, width] per camera."""
    rng = np.random.default_rng(seed)
    P, brightness = _sheet_particles(rng, pl, sheet, density, sheet_sigma, margin)
    half = 0.5 * np.asarray(flow(P), np.float64)
    out = []
    for cam in cameras:
        frames = [_render(_project(cam, Q), brightness * _sheet_light(Q, sheet, sheet_sigma), shape, diameter) for Q in (P - half, P + half)]
        out.append(np.stack(frames).astype(np.float32))
    return tuple(out)


# ---- the synthetic stereo pairs of the tests and of tools/piv_stereo.py ---------------------------------------------------------
CASE_PLANE = centred_plane(192, 160, 0.2)       # 38.4 x 32 mm at 0.2 mm per dewarped pixel
CASE_SENSOR = (224, 256)
CASE_GRID = dict(win=32, step=16, radius=8, iterations=3)
CASE_ANGLES = {"symmetric": ((30.0, 0.0), (-30.0, 0.0)), "asymmetric": ((35.0, 5.0), (-20.0, -3.0))}       # (theta, phi) in degrees


def uniform_flow(P):
    return np.broadcast_to(np.array([0.5, -0.3, 0.4]), np.shape(P))


def shear_flow(P):
    P = np.asarray(P, np.float64)
    return np.stack([np.full(P.shape[:-1], 0.3), -0.2 + 0.01 * P[..., 0], 0.02 * P[..., 0] + 0.01 * P[..., 1]], axis=-1)


CASES = {"uniform": ("symmetric", uniform_flow, 7), "shear": ("symmetric", shear_flow, 8), "asymmetric": ("asymmetric", uniform_flow, 9)}


def calibrated_pair(kind: str, distance: float = 300.0, px_per_mm: float = 5.0):
    """((pinhole, fitted camera, rms, max residual) per camera) of CASE_ANGLES[kind]: pinholes at `distance` mm with
    `px_per_mm` at the origin, fitted on the 9 x 9 x 3 target (Z = -1, 0, 1) over CASE_PLANE."""
    target = calibration_target(CASE_PLANE, 9, (-1.0, 0.0, 1.0))
    out = []
    for theta, phi in CASE_ANGLES[kind]:
        view = pinhole(np.deg2rad(theta), np.deg2rad(phi), distance, px_per_mm, CASE_SENSOR)
        out.append((view, *fit_camera(target, view.project(target))))
    return tuple(out)


def case_pair(name: str):
    """(cam1 frames, cam2 frames, the two fitted cameras) of CASES[name]: f32 [2, 224, 256] each, 0.035 particles per pixel,
    rendered through the pinholes themselves."""
    kind, flow, seed = CASES[name]
    views = calibrated_pair(kind)
    f1, f2 = particle_pair([v[0] for v in views], flow, CASE_PLANE, seed, shape=CASE_SENSOR, density=0.035)
    return f1, f2, tuple(v[1] for v in views)


def case_figures(name: str, out, vectors1):
    """Of a stereo result on CASES[name] (out [9, 11, 8], camera 1's field [9, 11, >= 2]), over the interior nodes, in dewarped
    pixels: (rms error of dX, dY, dZ; rms error of dX read from camera 1 alone; median and largest stereo residual)."""
    truth = CASES[name][1](window_centres(CASE_PLANE, CASE_GRID["win"], CASE_GRID["step"]))
    inner = (slice(1, -1), slice(1, -1))
    err = (np.asarray(out)[..., :3] - truth)[inner] / CASE_PLANE["pitch"]
    alone = (np.asarray(vectors1, np.float64)[..., 0] - truth[..., 0] / CASE_PLANE["pitch"])[inner]
    res = np.asarray(out)[..., 3][inner]
    return np.sqrt(np.mean(err ** 2, axis=(0, 1))), float(np.sqrt(np.mean(alone ** 2))), float(np.median(res)), float(res.max())


# ---- the self-calibration case of the tests and of tools/piv_stereo.py --self-calibrate ----------------------------------------
def selfcal_flow(P):
    P = np.asarray(P, np.float64)
    return np.stack([0.3 + 0.05 * P[..., 0], -0.2 + 0.01 * P[..., 1], np.full(P.shape[:-1], 0.2)], axis=-1)


SELFCAL_CASE = dict(plane=CASE_PLANE, kind="symmetric", sheet_sigma=0.3, sheet=(0.8, 0.02, -0.015), flow=selfcal_flow, n_frames=8, density=0.12,
                    seed=3, pair_seed=42, disparity=dict(win=64, step=32, radius=16), evaluation=dict(CASE_GRID, iterations=2))


def selfcal_inputs():
    """Of SELFCAL_CASE: (the calibrated views as calibrated_pair returns them; the two stacks of simultaneous frames that
    self-calibration takes; the two-exposure pair of the flow on the displaced sheet; the same flow on the aligned sheet)."""
    case = SELFCAL_CASE
    views = calibrated_pair(case["kind"])
    pinholes, pl = [v[0] for v in views], case["plane"]
    common = dict(shape=CASE_SENSOR, sheet_sigma=case["sheet_sigma"])
    frames = sheet_frames(pinholes, pl, case["sheet"], case["n_frames"], case["seed"], density=case["density"], **common)
    pair = sheet_pair(pinholes, case["flow"], pl, case["sheet"], case["pair_seed"], **common)
    aligned = sheet_pair(pinholes, case["flow"], pl, (pl["z"], 0.0, 0.0), case["pair_seed"], **common)
    return views, frames, pair, aligned


def selfcal_figures(out, frame=None):
    """Of a stereo result on SELFCAL_CASE's evaluation grid (out [9, 11, 8]) computed with cameras that live in `frame` (R, O,
    C; None: the original calibration's world), over the interior nodes, in dewarped pixels: (rms error of dX, dY, dZ; the
    median stereo residual).  The truth at a node is the flow at the node's world point, in the frame's components:
    flow(O + R (node - C)) . R."""
    case = SELFCAL_CASE
    pl, grid = case["plane"], case["evaluation"]
    R, O, C = identity_frame(pl) if frame is None else frame
    truth = case["flow"](to_world((R, O, C), window_centres(pl, grid["win"], grid["step"]))) @ np.asarray(R)
    inner = (slice(1, -1), slice(1, -1))
    err = (np.asarray(out)[..., :3] - truth)[inner] / pl["pitch"]
    return np.sqrt(np.mean(err ** 2, axis=(0, 1))), float(np.median(np.asarray(out)[..., 3][inner]))
