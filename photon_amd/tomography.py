"""Tomographic BOS: the 3-D field from several views' projected density (pure numpy, f64: usable without a GPU).

The device form is section 9 of include/parallel_ray_tracing.h (``PhotonLibrary.tomo_project``, ``tomo_backproject``,
``tomo_reconstruct``).  This module holds

* ``ray_taps``: the taps of the definition -- Joseph's method: per ray the grid planes along its dominant axis, four
  bilinear taps in each -- by the same f64 operations in the same order as the device;
* ``project_model``, ``backproject_model``, ``reconstruct_model``: the projector A, its adjoint and the conjugate-gradient
  solver of section 9 on those taps (vectorised over the rays, a loop over the planes, sums by ``np.bincount``, which adds
  in array order: the projector's sums run in the order of the definition);
* section 10, tomography from the deflections themselves: ``deflection_taps`` (the same taps with the weights of the
  projector's derivative under a parallel shift of the ray along two transverse vectors), ``deflect_model``,
  ``deflect_adjoint_model`` and ``reconstruct_deflections_model``;
* the geometry that carries a camera's measurement into it: ``view_rays`` (the world chief rays of a camera's grid nodes),
  ``view_frames`` (the world directions along which the camera measures its two deflection components) and ``grid_of`` (a
  volume's grid in the same frame).

Arrays over the voxels are indexed [z, y, x] (x fastest), as the volumes are; dims = (nx, ny, nz).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

CHECK_EVERY = 8                 # PHOTON_TOMO_CHECK_EVERY
DEFAULT_MAX_ITER = 100


def check_arguments(dims, spacing, origin, n_rays, lam=0.0, tol=0.0, max_iter=0, frames=None):
    """The arguments sections 9 and 10 refuse, as a ValueError (null pointers aside).  frames: section 10's (t1, t2), which
    must both be there and hold three values per ray."""
    nx, ny, nz = (int(v) for v in dims)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"nx, ny and nz must be >= 2, not {nx} x {ny} x {nz}")
    if nx * ny * nz > 2 ** 31 - 1:
        raise ValueError(f"{nx} x {ny} x {nz} is more than INT_MAX voxels")
    if int(n_rays) < 1:
        raise ValueError("n_rays must be >= 1")
    spacing, origin = np.asarray(spacing, np.float64), np.asarray(origin, np.float64)
    if spacing.shape != (3,) or origin.shape != (3,):
        raise ValueError("spacing and origin must hold three values each")
    if not (np.isfinite(spacing).all() and (spacing > 0).all()):
        raise ValueError(f"every spacing must be finite and > 0, not {spacing}")
    if not np.isfinite(origin).all():
        raise ValueError(f"every origin must be finite, not {origin}")
    if not lam >= 0:
        raise ValueError(f"lam must be >= 0, not {lam}")
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0, not {tol}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter must be >= 0, not {max_iter}")
    if frames is not None:
        if len(frames) != 2 or any(t is None for t in frames):
            raise ValueError("t1 and t2 must both be given")
        if any(np.shape(t) != (int(n_rays), 3) for t in frames):
            raise ValueError("t1 and t2 must both be [n_rays, 3]")


def _rays(origins, dirs):
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and dirs must both be [n_rays, 3]")
    return o, d


class Taps(NamedTuple):
    """Every tap of a set of rays through a grid, for an operator of K = len(weights) components per ray (section 9's
    projector: 1; section 10's pair: 2): tap i adds weights[k][i] * f[voxel[i]] to component k of ray[i].  The taps of one
    ray follow each other in the order of the definition (planes ascending, four taps per plane); planes[r] is the number
    of counted planes of ray r."""
    ray: np.ndarray
    voxel: np.ndarray
    weights: tuple
    planes: np.ndarray
    n_voxels: int


DeflectionTaps = Taps           # the name section 10's taps had as a type of their own: kept for callers' annotations


def _walk(dims, spacing, origin, o, d, frames=()):
    """Steps 1 to 3 of section 9 for rays o, d [n, 3], every step the definition's f64 operation: yields per dominant axis a
    and plane kappa the rays r that count it, their four voxels [len(r), 4], f_b, f_c, g_b, g_c and scale, and for every
    tau [n, 3] of `frames` section 10's (p_u, p_v) of those rays (a ray with a tau that is not finite is a miss)."""
    n = tuple(int(v) for v in dims)
    h = tuple(float(v) for v in np.asarray(spacing, np.float64))
    g = tuple(float(v) for v in np.asarray(origin, np.float64))
    stride = (1, n[0], n[0] * n[1])
    with np.errstate(all="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        hit = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(length) & (length > 0)
        e = d / length[:, None]
    for tau in frames:
        hit = hit & np.isfinite(tau).all(axis=1)
    mag = np.abs(e)
    axis = np.zeros(o.shape[0], np.int64)
    top = mag[:, 0].copy()
    for a in (1, 2):
        more = mag[:, a] > top
        axis[more] = a
        top = np.where(more, mag[:, a], top)
    for a, (b, c) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        idx = np.nonzero(hit & (axis == a))[0]
        if idx.size == 0:
            continue
        oa, ob, oc = o[idx, a], o[idx, b], o[idx, c]
        ea, eb, ec = e[idx, a], e[idx, b], e[idx, c]
        scale = h[a] / top[idx]
        rates = []
        for tau in frames:
            r = tau[idx, a] / ea
            rates.append((((tau[idx, b] - r * eb) / h[b]) * scale, ((tau[idx, c] - r * ec) / h[c]) * scale))
        for kappa in range(n[a]):
            plane = g[a] + float(kappa) * h[a]
            t = (plane - oa) / ea
            u = ((ob + t * eb) - g[b]) / h[b]
            v = ((oc + t * ec) - g[c]) / h[c]
            ok = (u >= 0.0) & (u <= n[b] - 1) & (v >= 0.0) & (v <= n[c] - 1)
            if not ok.any():
                continue
            u, v, s, r = u[ok], v[ok], scale[ok], idx[ok]
            ib, ic = np.minimum(np.floor(u), n[b] - 2), np.minimum(np.floor(v), n[c] - 2)
            fb, fc = u - ib, v - ic
            hb, hc = 1.0 - fb, 1.0 - fc
            base = kappa * stride[a] + ib.astype(np.int64) * stride[b] + ic.astype(np.int64) * stride[c]
            voxels = np.stack([base, base + stride[b], base + stride[c], base + stride[b] + stride[c]], axis=1)
            yield r, voxels, fb, fc, hb, hc, s, [(pu[ok], pv[ok]) for pu, pv in rates]


def _taps(dims, spacing, origin, origins, dirs, frames=None) -> Taps:
    """The taps of section 9's projector (frames None) or of section 10's D_t1 and D_t2 (frames = (t1, t2)), every step the
    definition's f64 operation."""
    o, d = _rays(origins, dirs)
    check_arguments(dims, spacing, origin, o.shape[0])
    if frames is not None:
        frames = _frames(*frames, o.shape[0])
    n = tuple(int(v) for v in dims)
    rays, voxels = [], []
    weights = tuple([] for _ in (frames or (None,)))
    planes = np.zeros(o.shape[0], np.int64)
    for r, vox, fb, fc, gb, gc, s, rates in _walk(dims, spacing, origin, o, d, frames=frames or ()):
        voxels.append(vox)
        rays.append(np.repeat(r, 4).reshape(-1, 4))
        planes[r] += 1
        if frames is None:
            weights[0].append(np.stack([(gb * gc) * s, (fb * gc) * s, (gb * fc) * s, (fb * fc) * s], axis=1))
        for out, (pu, pv) in zip(weights, rates):
            gcu, gbv, fcu, fbv = gc * pu, gb * pv, fc * pu, fb * pv
            out.append(np.stack([-gcu - gbv, gcu - fbv, gbv - fcu, fcu + fbv], axis=1))
    if not rays:
        empty = np.zeros(0, np.int64)
        return Taps(empty, empty, tuple(np.zeros(0) for _ in weights), planes, n[0] * n[1] * n[2])
    return Taps(np.concatenate(rays).ravel(), np.concatenate(voxels).ravel(), tuple(np.concatenate(w).ravel() for w in weights),
                planes, n[0] * n[1] * n[2])


def ray_taps(dims, spacing, origin, origins, dirs) -> Taps:
    """The taps of section 9's projector, every step the definition's f64 operation."""
    return _taps(dims, spacing, origin, origins, dirs)


def _frames(t1, t2, n_rays):
    if t1 is None or t2 is None:
        raise ValueError("t1 and t2 must both be given")
    t1 = np.ascontiguousarray(t1, np.float64).reshape(-1, 3)
    t2 = np.ascontiguousarray(t2, np.float64).reshape(-1, 3)
    check_arguments((2, 2, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), n_rays, frames=(t1, t2))
    return t1, t2


def deflection_taps(dims, spacing, origin, origins, dirs, t1, t2) -> Taps:
    """The taps of section 10's D_t1 and D_t2 (the derivative of section 9's projector under a parallel shift of the ray
    along t1, t2 [n_rays, 3]), every step the definition's f64 operation."""
    return _taps(dims, spacing, origin, origins, dirs, frames=(t1, t2))


def _forward(taps: Taps, f: np.ndarray) -> tuple:
    """Op f over the voxels: one array over the rays per component."""
    return tuple(np.bincount(taps.ray, w * f[taps.voxel], minlength=taps.planes.size) for w in taps.weights)


def _adjoint(taps: Taps, ys) -> np.ndarray:
    """Op^T ys over the voxels, one value per tap: w_1 y_1 (+ w_2 y_2)."""
    value = taps.weights[0] * ys[0][taps.ray]
    for w, y in zip(taps.weights[1:], ys[1:]):
        value = value + w * y[taps.ray]
    return np.bincount(taps.voxel, value, minlength=taps.n_voxels)


def _field(f):
    f = np.asarray(f, np.float64)
    if f.ndim != 3:
        raise ValueError("f must be [nz, ny, nx]")
    return f


def _adjoint_model(ys, dims, v, taps):
    nx, ny, nz = (int(n) for n in dims)
    out = _adjoint(taps, [np.asarray(y, np.float64).ravel() for y in ys]).reshape(nz, ny, nx)
    return out if v is None else np.asarray(v, np.float64).reshape(nz, ny, nx) + out


def project_model(f, spacing, origin, origins, dirs, taps: Optional[Taps] = None) -> np.ndarray:
    """Host model of photon_tomo_project: P = A f, f [nz, ny, nx].  taps: ray_taps of the same grid and rays, when the
    caller has them."""
    f = _field(f)
    if taps is None:
        taps = ray_taps(f.shape[::-1], spacing, origin, origins, dirs)
    return _forward(taps, f.ravel())[0]


def backproject_model(y, dims, spacing, origin, origins, dirs, v=None, taps: Optional[Taps] = None) -> np.ndarray:
    """Host model of photon_tomo_backproject: v + A^T y as a new array [nz, ny, nx] (v None = 0)."""
    if taps is None:
        taps = ray_taps(dims, spacing, origin, origins, dirs)
    return _adjoint_model((y,), dims, v, taps)


def graph_laplacian(q: np.ndarray) -> np.ndarray:
    """G^T G q on [nz, ny, nx]: per voxel the sum over its neighbours inside the grid of (q_c - q_n), added in the order
    -x, +x, -y, +y, -z, +z."""
    lap = np.zeros_like(q)
    lap[:, :, 1:] += q[:, :, 1:] - q[:, :, :-1]
    lap[:, :, :-1] += q[:, :, :-1] - q[:, :, 1:]
    lap[:, 1:, :] += q[:, 1:, :] - q[:, :-1, :]
    lap[:, :-1, :] += q[:, :-1, :] - q[:, 1:, :]
    lap[1:, :, :] += q[1:, :, :] - q[:-1, :, :]
    lap[:-1, :, :] += q[:-1, :, :] - q[1:, :, :]
    return lap


def _conjugate_gradients(normal, b, m, reg, shape, tol, max_iter):
    """The iteration of section 9 on  m (normal + reg G^T G) m x = b  from x = 0: normal(q) = Op^T W Op q over the voxels.
    Returns (x, iterations, rho, |b|)."""
    x = np.zeros(b.size)
    r = b
    q = r.copy()
    rho = float(np.dot(r, r))
    bnorm = np.sqrt(rho)
    it = 0
    if bnorm > 0:
        while True:
            if it % CHECK_EVERY == 0 and tol > 0 and np.sqrt(rho) <= tol * bnorm:
                break
            if it == max_iter:
                break
            s = np.where(m, normal(q) + reg * graph_laplacian(q.reshape(shape)).ravel(), 0.0)
            qs = float(np.dot(q, s))
            alpha = rho / qs if qs != 0 else 0.0
            x = x + alpha * q
            r = r - alpha * s
            rho_new = float(np.dot(r, r))
            beta = rho_new / rho if rho != 0 else 0.0
            q = r + beta * q
            rho = rho_new
            it += 1
    return x, it, rho, bnorm


def _stats(it, rho, bnorm, tol, m, used):
    return dict(iterations=it, converged=int(bool(bnorm == 0 or np.sqrt(rho) <= tol * bnorm)), unknowns=int(m.sum()),
                rays_used=int(used.sum()), residual=float(np.sqrt(rho) / bnorm) if bnorm > 0 else 0.0)


def _support(support, dims):
    nx, ny, nz = (int(n) for n in dims)
    m = np.ones(nx * ny * nz, bool) if support is None else np.asarray(support).ravel() != 0
    if m.shape != (nx * ny * nz,):
        raise ValueError("support must have the shape of the grid")
    return m


def _reconstruct(data, names, dims, w, support, reg, tol, max_iter, taps: Taps):
    """The solver of sections 9 and 10 on the taps of either: data the K arrays over the rays (`names` for the message), reg
    the weight of G^T G."""
    nx, ny, nz = (int(n) for n in dims)
    data = [np.asarray(a, np.float64).ravel() for a in data]
    w = np.ones_like(data[0]) if w is None else np.asarray(w, np.float64).ravel()
    if any(a.shape != taps.planes.shape for a in data + [w]):
        raise ValueError(f"{names} and w must hold one value per ray")
    m = _support(support, dims)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(w) & (w > 0)
        for a in data:
            ok = ok & np.isfinite(a)
    weight = np.where(ok, w, 0.0)
    wdata = [np.where(ok, w * np.where(ok, a, 0.0), 0.0) for a in data]

    def normal(q):
        return _adjoint(taps, [np.where(weight > 0, weight * a, 0.0) for a in _forward(taps, q)])

    x, it, rho, bnorm = _conjugate_gradients(normal, np.where(m, _adjoint(taps, wdata), 0.0), m, reg, (nz, ny, nx), tol, max_iter)
    return x.reshape(nz, ny, nx), _stats(it, rho, bnorm, tol, m, (weight > 0) & (taps.planes > 0))


def reconstruct_model(p, dims, spacing, origin, origins, dirs, w=None, support=None, lam: float = 1.0, tol: float = 1e-6,
                      max_iter: int = DEFAULT_MAX_ITER, taps: Optional[Taps] = None):
    """Host model of photon_tomo_reconstruct (section 9: the same iteration and check cadence).  p, w [n_rays] (w None =
    1); support [nz, ny, nx] (None = every voxel).  Returns (f [nz, ny, nx], stats dict: iterations, converged, unknowns,
    rays_used, residual)."""
    o, d = _rays(origins, dirs)
    check_arguments(dims, spacing, origin, o.shape[0], lam, tol, max_iter)
    if taps is None:
        taps = ray_taps(dims, spacing, origin, o, d)
    h = float(np.min(np.asarray(spacing, np.float64)))
    return _reconstruct((p,), "p", dims, w, support, float(lam) * (h * h), tol, max_iter, taps)


# ---- section 10: the operator pair of the deflections -----------------------------------------------------------------------
def deflect_model(f, spacing, origin, origins, dirs, t1, t2, taps: Optional[Taps] = None):
    """Host model of photon_tomo_deflect: (g1, g2) = (D_t1 f, D_t2 f), f [nz, ny, nx].  taps: deflection_taps of the same
    grid, rays and vectors, when the caller has them."""
    f = _field(f)
    if taps is None:
        taps = deflection_taps(f.shape[::-1], spacing, origin, origins, dirs, t1, t2)
    return _forward(taps, f.ravel())


def deflect_adjoint_model(y1, y2, dims, spacing, origin, origins, dirs, t1, t2, v=None, taps: Optional[Taps] = None) -> np.ndarray:
    """Host model of photon_tomo_deflect_adjoint: v + D_t1^T y1 + D_t2^T y2 as a new array [nz, ny, nx] (v None = 0)."""
    if taps is None:
        taps = deflection_taps(dims, spacing, origin, origins, dirs, t1, t2)
    return _adjoint_model((y1, y2), dims, v, taps)


def reconstruct_deflections_model(g1, g2, dims, spacing, origin, origins, dirs, t1, t2, w=None, support=None, lam: float = 1.0,
                                  tol: float = 1e-6, max_iter: int = DEFAULT_MAX_ITER, taps: Optional[Taps] = None):
    """Host model of photon_tomo_reconstruct_deflections (section 10: section 9's iteration on the operator pair, lam on
    G^T G without h^2).  g1, g2, w [n_rays] (w None = 1); support [nz, ny, nx] (None = every voxel: the solution has zero
    mean).  Returns (f [nz, ny, nx], stats dict) as reconstruct_model does."""
    o, d = _rays(origins, dirs)
    check_arguments(dims, spacing, origin, o.shape[0], lam, tol, max_iter)
    t1, t2 = _frames(t1, t2, o.shape[0])
    if taps is None:
        taps = deflection_taps(dims, spacing, origin, o, d, t1, t2)
    return _reconstruct((g1, g2), "g1, g2", dims, w, support, float(lam), tol, max_iter, taps)


# ---- geometry ------------------------------------------------------------------------------------------------------------
WORLD_Z_SHIFT = 750e3           # camera z = world z + z_offset + 750e3 (photon_amd/csrc/device_optics.hpp)


def rotate_about(points, rotation, pivot=None) -> np.ndarray:
    """R (x - pivot) + pivot for points [..., 3] (pivot None = the origin)."""
    R = np.asarray(rotation, np.float64).reshape(3, 3)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64)
    return (np.asarray(points, np.float64) - c) @ R.T + c


def view_rays(call, target_xy, rotation=None, pivot=None):
    """The world chief rays of a camera's grid nodes: (origins, dirs), each [..., 3] like X_t.  target_xy = (X_t, Y_t), the
    nodes' target-plane points (bos_density.node_geometry).  The chief-ray model of bos_density.chief_ray_projection: from
    the target point at object_distance straight through the lens centre; carried into the world frame as the device
    carries its rays (z -= z_offset + 750e3, then the camera's inverse_rotation_matrix), then rotated by `rotation` (3 x 3)
    about `pivot` (None = the world origin) when one is given.  The origins are the target points."""
    Xt, Yt = (np.asarray(a, np.float64) for a in target_xy)
    z_lens = float(call.z_offset)
    target = np.stack([Xt, Yt, np.full(Xt.shape, z_lens + float(call.object_distance))], axis=-1)
    lens = np.array([0.0, 0.0, z_lens])
    shift = np.array([0.0, 0.0, float(call.z_offset) + WORLD_Z_SHIFT])
    inv = np.asarray(call.camera.get("inverse_rotation_matrix", np.eye(3)), np.float32).astype(np.float64).reshape(3, 3)
    origins = (target - shift) @ inv.T
    dirs = np.broadcast_to(lens - shift, target.shape) @ inv.T - origins
    if rotation is not None:
        R = np.asarray(rotation, np.float64).reshape(3, 3)
        origins, dirs = rotate_about(origins, R, pivot), dirs @ R.T
    return origins, dirs


def view_frames(call, target_xy, rotation=None):
    """The world directions along which bos_density.gradients_from_displacements measures gx and gy at a camera's grid
    nodes: (t1, t2), each [..., 3] like X_t.  gx and gy run along the grid's columns and rows, which lie along the camera's
    X and Y axes in the sense of bos_density.axis_signs; the axes are carried into the world frame as view_rays carries its
    directions (the camera's inverse_rotation_matrix, then `rotation`) and are the same at every node: section 10's operator
    keeps only the part of each that is perpendicular to the node's ray."""
    from .bos_density import axis_signs
    Xt = np.asarray(target_xy[0], np.float64)
    inv = np.asarray(call.camera.get("inverse_rotation_matrix", np.eye(3)), np.float32).astype(np.float64).reshape(3, 3)
    axes = (np.asarray(axis_signs(call.camera))[:, None] * np.eye(3)[:2]) @ inv.T
    if rotation is not None:
        axes = axes @ np.asarray(rotation, np.float64).reshape(3, 3).T
    return tuple(np.ascontiguousarray(np.broadcast_to(axes[j], Xt.shape + (3,))) for j in range(2))


def grid_of(volume_info):
    """(dims (nx, ny, nz), spacing, origin) of a Volume (its info()) in the frame of view_rays: the bounds a volume reports
    are world coordinates already."""
    v = volume_info
    return ((int(v.nx), int(v.ny), int(v.nz)), np.array([float(s) for s in v.grid_spacing]),
            np.array([float(s) for s in v.min_bound]))


def line_distance_sq(origins, dirs, point) -> np.ndarray:
    """Squared distance from `point` to each line origins + t dirs."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    rel = np.asarray(point, np.float64) - o
    along = (rel * d).sum(axis=-1) / (d * d).sum(axis=-1)
    return ((rel - along[..., None] * d) ** 2).sum(axis=-1)
