"""Stereo PIV (pure numpy: usable without a GPU): two cameras on one light sheet, three displacement components.

The device forms are photon_piv_dewarp and photon_piv_stereo_reconstruct (include/parallel_ray_tracing.h, section 19;
``PhotonLibrary.piv_dewarp`` / ``piv_stereo_reconstruct`` on raw device pointers, ``PhotonLibrary.dewarp`` and
``PhotonLibrary.correlate_stereo`` on arrays).  This module holds what the C side has no part in and the host models:

* the camera model -- Soloff's polynomial from world (X, Y, Z) to image (x, y), 19 terms per coordinate: ``fit_camera``
  (least squares on a calibration target), ``map_points``, ``jacobian`` (analytic, in section 19b's operation order) and
  ``plane_coefficients`` (the camera folded at a plane into what the dewarp kernel takes);
* ``dewarp_model_f32`` (the kernel's operations in numpy f64 and f32: the device equals it bit for bit) and ``dewarp_model``
  (f64 throughout, from piv_deformation.bspline_coefficients_model);
* ``reconstruct_model``: section 19b in numpy, operation by operation;
* ``correlate_stereo_model``: the model of the driver's "deform" chain;
* generators for the tests and tools: ``pinhole`` (a perspective camera to calibrate against), ``calibration_target``,
  ``centred_plane`` and ``particle_pair`` (Gaussian particle images of a 3-C flow in a Gaussian sheet, per camera), and
  the three synthetic pairs the tests and tools/piv_stereo.py measure (``CASES``, ``case_pair``, ``case_figures``).

A camera is a dict centre[3], scale[3], cx[19], cy[19] (f64); a plane a dict x0, y0, pitch, z, width, height: dewarped
pixel (row i, column j) is the world point (x0 + j pitch, y0 + i pitch, z).

The reconstruction is first order: the Jacobian is taken at the plane, at the window centre, not at the half-displaced
particle positions; and nothing corrects a sheet that is not where the calibration says (no disparity correction).
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


def _taps(poly, grid, out_shape, shape):
    h, w = shape
    x, y = folded_points(poly, grid, out_shape)
    inside = ~outside_mask(poly, grid, out_shape, shape)
    x, y = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    fx, fy = np.floor(x), np.floor(y)
    xi = [pd.mirror_index(fx.astype(np.int64) - 1 + t, w) for t in range(4)]
    yi = [pd.mirror_index(fy.astype(np.int64) - 1 + t, h) for t in range(4)]
    return inside, x - fx, y - fy, xi, yi


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
    wx, wy = pd._bspline_weights(tx), pd._bspline_weights(ty)
    out = np.zeros((a.shape[0],) + tuple(inside.shape))
    for f in range(a.shape[0]):
        c = pd.bspline_coefficients_model(a[f])
        acc = np.zeros(inside.shape)
        for t in range(4):
            acc = acc + wy[t] * (((wx[0] * c[yi[t], xi[0]] + wx[1] * c[yi[t], xi[1]]) + wx[2] * c[yi[t], xi[2]]) + wx[3] * c[yi[t], xi[3]])
        out[f] = np.where(inside, acc, 0.0)
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
