"""Projected density from a BOS displacement field: weighted least-squares integration of a gradient field (pure numpy:
usable without a GPU).

The device form is photon_integrate_gradient (include/parallel_ray_tracing.h, section 6; ``PhotonLibrary.integrate_gradient``
on arrays, ``PhotonLibrary.integrate_gradient_ptr`` on raw device pointers).  This module holds

* ``integrate_model``: its f64 host model -- the definition of section 6 and the same Jacobi-PCG iteration, check cadence,
  NaN and anchor rules;
* ``solve_direct``: a dense least-squares minimiser of the same energy for small grids, built from the edge list and not
  from the normal equations: an independent reference;
* ``weights_from_correlation``: 0 for median-test outliers, flat windows and vectors that are not finite, 1 otherwise;
* ``weights_from_uncertainty``: the same zeros, and w = median(sigma^2) / sigma^2 (capped) elsewhere, sigma the displacement
  uncertainty per vector of section 11 (photon_amd.piv_uncertainty); ``gradient_uncertainty`` and
  ``projected_density_uncertainty`` carry sigma through the physics and through section 6's minimiser to an error bar on phi;
* the physics that turns a displacement field into the gradient of the projected density, and its truth:
  ``displacement_factor``, ``node_geometry``, ``gradients_from_displacements``, ``chief_ray_projection``;
* ``reconstruct``: correlate an image pair on the device, weigh, convert, integrate; ``reconstruct_tracked`` and
  ``reconstruct_flow``: the same from tracked dots and from dense optical flow.

Physics (the paraxial BOS relation photon states as epsilon = Delta pitch / (M Z_D), d(rho)/dx = epsilon n_0 / (K dz)).
With P = int (rho - rho_0) ds (kg/m^3 um) along the chief ray and the gradient taken along world x, y in the volume's
mid-plane, the dot shift in the axes of ``deflections.to_pixels`` is  d = F grad P,  F = (M Z_D / pitch) (K / n_0),
n_0 = K rho_0 + 1, M = image_distance / object_distance, Z_D = object_distance - (origin_z + extent_z / 2): the distance
from the target to the volume's mid-plane (the z convention of a volume that lies origin_z .. origin_z + extent_z in
front of the lens).  Rays bend toward higher density; the dot seen through the volume moves along +F grad P on the
sensor, which the lens has inverted.

Grid geometry.  Node (i, j) is correlation window (i, j) at its centre (row, column index coordinates).  Its to_pixels
position (x - 1, y - 1 for the 4-pixel splat; N - 2 - x, y for the erf splat: piv_correlation.image_positions inverted)
gives the sensor point, the lens inverts it onto the target plane, X_t = -x_sensor / M, and the chief ray from X_t to the
lens centre crosses the mid-plane at s X_t, s = (origin_z + extent_z / 2) / object_distance.  Node spacing:
h = s step pitch / M.  Columns run along world -x for the 4-pixel splat and +x for the erf splat; rows along world -y.
"""
from __future__ import annotations

import numpy as np

CHECK_EVERY = 8                 # PHOTON_INTEGRATE_CHECK_EVERY: the residual is checked every this many iterations
K_GLADSTONE_DALE = 0.225e-3     # m^3 / kg (air)
RHO_0 = 1.225                   # kg / m^3


def default_max_iter(nx: int, ny: int) -> int:
    """The iteration cap when none is given: 20 max(nx, ny) (Jacobi-PCG needs about 3 n on a smooth field)."""
    return 20 * max(int(nx), int(ny))


def check_arguments(nx, ny, hx, hy, tol, max_iter):
    """The arguments photon_integrate_gradient refuses, as a ValueError (null pointers aside)."""
    nx, ny = int(nx), int(ny)
    if nx < 2 or ny < 2:
        raise ValueError(f"nx and ny must be >= 2, not {nx} x {ny}")
    if nx * ny > 2 ** 31 - 1:
        raise ValueError(f"{ny} x {nx} is more than INT_MAX nodes")
    for name, h in (("hx", hx), ("hy", hy)):
        if not (np.isfinite(h) and h > 0):
            raise ValueError(f"{name} must be finite and > 0, not {h}")
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0, not {tol}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter must be >= 0, not {max_iter}")


def _inputs(gx, gy, w, fixed, value):
    gx = np.asarray(gx, np.float64)
    gy = np.asarray(gy, np.float64)
    if gx.ndim != 2 or gx.shape != gy.shape:
        raise ValueError("gx and gy must be two 2-d arrays of one shape")
    ny, nx = gx.shape
    w = np.ones_like(gx) if w is None else np.asarray(w, np.float64)
    if fixed is None:
        fixed = np.zeros((ny, nx), bool)
        fixed[0, :] = fixed[-1, :] = fixed[:, 0] = fixed[:, -1] = True
    else:
        fixed = np.asarray(fixed) != 0
    value = np.zeros_like(gx) if value is None else np.asarray(value, np.float64)
    for name, a in (("w", w), ("fixed", fixed), ("value", value)):
        if a.shape != gx.shape:
            raise ValueError(f"{name} must have the shape of gx, {gx.shape}")
    return gx, gy, w, fixed, value


def edges(gx, gy, w=None, fixed=None, value=None, hx=1.0, hy=1.0):
    """The edges of the definition: (wh, th) of (i,j)->(i,j+1), [ny, nx-1]; (wv, tv) of (i,j)->(i+1,j), [ny-1, nx]; and
    the inputs (fixed mask, values) with the defaults applied."""
    gx, gy, w, fixed, value = _inputs(gx, gy, w, fixed, value)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(gx) & np.isfinite(gy) & np.isfinite(w) & (w > 0)
    live = valid & ~(fixed & ~np.isfinite(value))
    with np.errstate(invalid="ignore"):
        wh = np.where(live[:, :-1] & live[:, 1:], np.minimum(w[:, :-1], w[:, 1:]), 0.0)
        wv = np.where(live[:-1, :] & live[1:, :], np.minimum(w[:-1, :], w[1:, :]), 0.0)
        th = np.where(wh > 0, float(hx) * ((gx[:, :-1] + gx[:, 1:]) * 0.5), 0.0)
        tv = np.where(wv > 0, float(hy) * ((gy[:-1, :] + gy[1:, :]) * 0.5), 0.0)
    return wh, th, wv, tv, fixed, value


def reachable(wh, wv, fixed):
    """Unknown nodes that reach a fixed node through edges of positive weight: bool [ny, nx]."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ny, nx = fixed.shape
    k = np.arange(ny * nx).reshape(ny, nx)
    a = np.concatenate([k[:, :-1][wh > 0], k[:-1, :][wv > 0]])
    b = np.concatenate([k[:, 1:][wh > 0], k[1:, :][wv > 0]])
    g = coo_matrix((np.ones(a.size), (a, b)), shape=(ny * nx, ny * nx))
    _, label = connected_components(g, directed=False)
    anchored = np.zeros(label.max() + 1, bool)
    anchored[label[fixed.ravel()]] = True
    return (anchored[label] & ~fixed.ravel()).reshape(ny, nx)


def _laplacian(wh, wv):
    """A p on the whole grid (the caller keeps p = 0 off the solved nodes) and the diagonal, in the device's order."""
    ny, nx = wh.shape[0], wv.shape[1]
    wW = np.zeros((ny, nx)); wW[:, 1:] = wh
    wE = np.zeros((ny, nx)); wE[:, :-1] = wh
    wN = np.zeros((ny, nx)); wN[1:, :] = wv
    wS = np.zeros((ny, nx)); wS[:-1, :] = wv
    diag = ((wW + wE) + wN) + wS

    def apply(p):
        q = diag * p
        q[:, 1:] -= wh * p[:, :-1]
        q[:, :-1] -= wh * p[:, 1:]
        q[1:, :] -= wv * p[:-1, :]
        q[:-1, :] -= wv * p[1:, :]
        return q
    return apply, diag, (wW, wE, wN, wS)


def integrate_model(gx, gy, w=None, fixed=None, value=None, hx=1.0, hy=1.0, tol=1e-8, max_iter=None):
    """Host model of photon_integrate_gradient in f64.  Arrays [ny, nx] (gx along +column, gy along +row); w None = 1,
    fixed None = the outer frame, value None = 0.  Returns (phi [ny, nx], stats dict: iterations, converged, unknowns,
    unreachable, residual)."""
    gx, gy, w, fixed, value = _inputs(gx, gy, w, fixed, value)
    ny, nx = gx.shape
    max_iter = default_max_iter(nx, ny) if max_iter is None else int(max_iter)
    check_arguments(nx, ny, hx, hy, tol, max_iter)
    wh, th, wv, tv, fixed, value = edges(gx, gy, w, fixed, value, hx, hy)
    solve = reachable(wh, wv, fixed)
    apply, diag, (wW, wE, wN, wS) = _laplacian(wh, wv)

    # right-hand side in the device's order: W, E, N, S; a fixed neighbour adds w value
    vfix = np.where(fixed & np.isfinite(value), value, 0.0)
    b = np.zeros((ny, nx))
    b[:, 1:] += wh * th + np.where(fixed[:, :-1], wh * vfix[:, :-1], 0.0)
    b[:, :-1] += -(wh * th) + np.where(fixed[:, 1:], wh * vfix[:, 1:], 0.0)
    b[1:, :] += wv * tv + np.where(fixed[:-1, :], wv * vfix[:-1, :], 0.0)
    b[:-1, :] += -(wv * tv) + np.where(fixed[1:, :], wv * vfix[1:, :], 0.0)

    x = np.zeros((ny, nx))
    r = np.where(solve, b, 0.0)
    safe = np.where(solve, diag, 1.0)
    z = np.where(solve, r / safe, 0.0)
    p = np.zeros((ny, nx))
    rz = float(np.dot(r.ravel(), z.ravel()))
    rr = float(np.dot(r.ravel(), r.ravel()))
    bnorm = np.sqrt(rr)
    it, rz_old = 0, 0.0
    if bnorm > 0:
        while True:
            if it % CHECK_EVERY == 0 and tol > 0 and np.sqrt(rr) <= tol * bnorm:
                break
            if it == max_iter:
                break
            beta = 0.0 if it == 0 or rz_old == 0 else rz / rz_old
            p = z + beta * p
            q = np.where(solve, apply(p), 0.0)
            pq = float(np.dot(p.ravel(), q.ravel()))
            alpha = rz / pq if pq != 0 else 0.0
            x = x + alpha * p
            r = np.where(solve, r - alpha * q, 0.0)
            z = np.where(solve, r / safe, 0.0)
            rz_old, rz = rz, float(np.dot(r.ravel(), z.ravel()))
            rr = float(np.dot(r.ravel(), r.ravel()))
            it += 1
    phi = np.where(fixed, value, np.where(solve, x, np.nan))
    stats = dict(iterations=it, converged=int(bool(bnorm == 0 or np.sqrt(rr) <= tol * bnorm)),
                 unknowns=int(solve.sum()), unreachable=int((~fixed & ~solve).sum()),
                 residual=float(np.sqrt(rr) / bnorm) if bnorm > 0 else 0.0)
    return phi, stats


def solve_direct(gx, gy, w=None, fixed=None, value=None, hx=1.0, hy=1.0):
    """The minimiser of E = sum_e w_e (phi_b - phi_a - t_e)^2 by a dense weighted least-squares solve over the edge list
    (small grids: a few thousand unknowns at most).  Same output conventions as integrate_model."""
    wh, th, wv, tv, fixed, value = edges(gx, gy, w, fixed, value, hx, hy)
    ny, nx = fixed.shape
    solve = reachable(wh, wv, fixed)
    k = np.arange(ny * nx).reshape(ny, nx)
    a = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    bb = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    we = np.concatenate([wh.ravel(), wv.ravel()])
    te = np.concatenate([th.ravel(), tv.ravel()])
    s = solve.ravel()
    use = (we > 0) & (s[a] | s[bb])
    a, bb, we, te = a[use], bb[use], we[use], te[use]
    col = -np.ones(ny * nx, np.int64)
    col[s] = np.arange(int(s.sum()))
    D = np.zeros((a.size, int(s.sum())))
    rhs = te.copy()
    vals = value.ravel()
    for sign, node in ((1.0, bb), (-1.0, a)):
        unk = s[node]
        D[np.nonzero(unk)[0], col[node[unk]]] += sign
        rhs[~unk] -= sign * vals[node[~unk]]
    sq = np.sqrt(we)
    sol = np.linalg.lstsq(D * sq[:, None], rhs * sq, rcond=None)[0] if D.shape[1] else np.zeros(0)
    phi = np.where(fixed, value, np.nan).ravel()
    phi[s] = sol
    return phi.reshape(ny, nx)


def weights_from_correlation(vectors, flags, outliers) -> np.ndarray:
    """Integration weights from a correlation: 0 for median-test outliers, flat windows and vectors that are not finite,
    1 otherwise.  vectors [n_rows, n_cols, >= 2], flags [n_rows, n_cols], outliers bool [n_rows, n_cols]."""
    from .piv_correlation import FLAG_FLAT
    v = np.asarray(vectors, np.float64)[..., :2]
    bad = np.asarray(outliers, bool) | ((np.asarray(flags) & FLAG_FLAT) != 0) | ~np.isfinite(v).all(axis=-1)
    return np.where(bad, 0.0, 1.0)


def weights_from_uncertainty(sigma, flags, outliers, floor: float = 0.25) -> np.ndarray:
    """Integration weights w = 1 / sigma^2, scaled to a median of 1.  sigma [n_rows, n_cols, 2] = (sigma_x, sigma_y) px
    (``PhotonLibrary.displacement_uncertainty``), flags and outliers as weights_from_correlation takes them.  The weight is 0
    wherever weights_from_correlation gives 0 (median-test outliers, flat windows) and where sigma is not finite.  On the
    kept nodes, with s^2 = sigma_x^2 + sigma_y^2 and m^2 the median of s^2 over them, w = m^2 / max(s^2, (floor m)^2): the
    median weight is 1, so the solver's `tol` keeps its meaning, and no node outweighs the median by more than
    1 / floor^2 (a sigma of nearly 0 is an artefact of a window with hardly any noise in it, not 1000 times the
    information).  Equal sigma everywhere reproduces weights_from_correlation."""
    sg = np.asarray(sigma, np.float64)[..., :2]
    floor = float(floor)
    if not (np.isfinite(floor) and 0.0 < floor <= 1.0):
        raise ValueError(f"floor must lie in (0, 1], not {floor}")
    keep = weights_from_correlation(sg, flags, outliers) > 0
    s2 = (sg * sg).sum(axis=-1)
    w = np.zeros(s2.shape)
    if keep.any():
        m2 = float(np.median(s2[keep]))
        w[keep] = m2 / np.maximum(s2[keep], floor * floor * m2) if m2 > 0 else 1.0
    return w


# ---- physics ------------------------------------------------------------------------------------------------------------
def _magnification(call) -> float:
    return float(call.image_distance) / float(call.object_distance)


def displacement_factor(call, origin_z: float, extent_z: float, K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0) -> float:
    """F of d = F grad P: pixels of dot shift per (kg/m^3 um of P per um), F = (M Z_D / pitch) (K / n_0)."""
    Z_D = float(call.object_distance) - (float(origin_z) + 0.5 * float(extent_z))
    n_0 = K * rho_0 + 1.0
    return _magnification(call) * Z_D / float(call.camera["pixel_pitch"]) * (K / n_0)


def axis_signs(camera) -> tuple:
    """World direction of the grid's column and row axes: (-1, -1) for the 4-pixel splat, (+1, -1) for the erf splat."""
    from . import deflections
    return (1.0 if bool(deflections._camera(camera).get("implement_diffraction", False)) else -1.0), -1.0


def node_geometry(shape, win: int, step: int, call, origin_z: float, extent_z: float):
    """The integration grid of a correlation on an image of `shape`: (target-plane points (X_t, Y_t), mid-plane points
    (X, Y), each [n_rows, n_cols] world microns, spacing h = s step pitch / M)."""
    from . import piv_correlation as pc
    cam = call.camera
    rows, cols = pc.window_centres(shape, win, step)
    pitch = float(cam["pixel_pitch"])
    if bool(cam.get("implement_diffraction", False)):
        x_tp, y_tp = int(cam["x_pixel_number"]) - 2 - cols, rows
    else:
        x_tp, y_tp = cols + 1.0, rows + 1.0
    xs = x_tp * pitch - (int(cam["x_pixel_number"]) / 2 - 1) * pitch
    ys = y_tp * pitch - (int(cam["y_pixel_number"]) / 2 - 1) * pitch
    M = _magnification(call)
    Xt, Yt = -xs / M, -ys / M
    s = (float(origin_z) + 0.5 * float(extent_z)) / float(call.object_distance)
    return (Xt, Yt), (s * Xt, s * Yt), s * step * pitch / M


def gradients_from_displacements(disp_px, camera, factor: float):
    """Dot shifts in the to_pixels axes [..., 2] -> (gx, gy): the gradient of P along the grid's columns and rows."""
    d = np.asarray(disp_px, np.float64)
    sx, sy = axis_signs(camera)
    return sx * d[..., 0] / factor, sy * d[..., 1] / factor


def gradient_uncertainty(sigma_px, camera, factor: float):
    """Displacement uncertainties [..., 2] = (sigma_x, sigma_y) px -> (sigma_gx, sigma_gy): gradients_from_displacements'
    linear map by absolute value (the axis flips of the splats change no standard deviation)."""
    s = np.abs(np.asarray(sigma_px, np.float64))
    return s[..., 0] / abs(float(factor)), s[..., 1] / abs(float(factor))


def projected_density_uncertainty(sigma_gx, sigma_gy, w=None, fixed=None, hx=1.0, hy=1.0):
    """The standard deviation of section 6's minimiser phi from those of its input gradients, by linear propagation: for
    fixed weights phi = J_x g_x + J_y g_y + const, and with the nodes' errors independent
    sigma_phi^2(k) = sum_j J_x[k, j]^2 sigma_gx[j]^2 + J_y[k, j]^2 sigma_gy[j]^2.  Arrays [ny, nx] as integrate_model takes
    them (w None = 1, fixed None = the outer frame); a node whose sigma is not finite counts as invalid, like a gradient
    that is not finite.  Returns sigma_phi [ny, nx]: 0 on the fixed nodes, NaN where phi is NaN.
    Limits: J is built densely over the edge list like solve_direct (the pseudo-inverse of an edges x unknowns matrix): a few
    thousand unknowns, host only.  The nodes are treated as independent although overlapping windows share pixels (at 50 %
    overlap neighbouring vectors correlate, and the true error bar of a smooth phi is wider than this one); the weights are
    taken as given, not as functions of the data; the uncertainty of the fixed values is not included."""
    wh, _, wv, _, fixed, _ = edges(sigma_gx, sigma_gy, w, fixed, None, hx, hy)
    sgx, sgy = np.asarray(sigma_gx, np.float64), np.asarray(sigma_gy, np.float64)
    ny, nx = fixed.shape
    solve = reachable(wh, wv, fixed)
    s = solve.ravel()
    k = np.arange(ny * nx).reshape(ny, nx)
    nh = wh.size
    a = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    b = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    we = np.concatenate([wh.ravel(), wv.ravel()])
    horizontal = np.arange(a.size) < nh
    use = (we > 0) & (s[a] | s[b])
    a, b, we, horizontal = a[use], b[use], we[use], horizontal[use]
    n_unknown = int(s.sum())
    out = np.where(fixed, 0.0, np.nan).ravel()
    if n_unknown:
        col = -np.ones(ny * nx, np.int64)
        col[s] = np.arange(n_unknown)
        D = np.zeros((a.size, n_unknown))
        for sign, node in ((1.0, b), (-1.0, a)):
            unk = s[node]
            D[np.nonzero(unk)[0], col[node[unk]]] += sign
        sq = np.sqrt(we)
        M = np.linalg.pinv(D * sq[:, None]) * sq[None, :]           # phi = M t over the edges' targets t
        var = np.zeros(n_unknown)
        for sel, h, sg in ((horizontal, float(hx), sgx), (~horizontal, float(hy), sgy)):
            # t_e = h (g_a + g_b) / 2: column j of J collects the edges that touch node j
            J = np.zeros((n_unknown, ny * nx))
            for node in (a[sel], b[sel]):
                np.add.at(J.T, node, (0.5 * h * M[:, sel]).T)
            touched = np.abs(J).sum(axis=0) > 0
            var += (J[:, touched] ** 2) @ (sg.ravel()[touched] ** 2)
        out[s] = np.sqrt(var)
    return out.reshape(ny, nx)


def chief_ray_projection(rho_fn, target_xy, object_distance: float, z_range, rho_0: float = RHO_0, samples: int = 2000):
    """The truth: P = int (rho - rho_0) ds along each node's chief ray, from its target-plane point (X_t, Y_t) at distance
    object_distance toward the lens centre, across z in z_range = (z0, z1) (midpoint rule, `samples` steps).
    rho_fn(x, y, z) takes and returns arrays (world microns; z measured from the lens).  Returns [...] like X_t."""
    Xt, Yt = (np.asarray(a, np.float64) for a in target_xy)
    z0, z1 = (float(v) for v in z_range)
    L = float(object_distance)
    dz = (z1 - z0) / samples
    zs = z0 + (np.arange(samples) + 0.5) * dz
    out = np.empty(Xt.shape)
    stretch = np.sqrt(1.0 + (Xt / L) ** 2 + (Yt / L) ** 2)
    for idx in np.ndindex(Xt.shape):
        x, y = Xt[idx] * zs / L, Yt[idx] * zs / L
        out[idx] = (np.asarray(rho_fn(x, y, zs), np.float64) - rho_0).sum() * dz * stretch[idx]
    return out


def gaussian_projection(r2, amplitude: float, sigma: float):
    """P of a Gaussian blob amplitude exp(-|r|^2 / 2 sigma^2) integrated along a straight line at squared distance r2."""
    return amplitude * sigma * np.sqrt(2.0 * np.pi) * np.exp(-np.asarray(r2, np.float64) / (2.0 * sigma ** 2))


def measured_gradients(vectors, flags, shape, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16,
                       weights: str = "median", K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0, sigma=None):
    """What a correlation measures, before any integration: (gx, gy, w, target-plane nodes (X_t, Y_t), mid-plane nodes
    (X, Y), spacing h).  gx, gy [n_rows, n_cols]: int grad (rho - rho_0) ds along each node's chief ray, along the grid's
    columns and rows; w the weights (`weights`: "median" = weights_from_correlation after the normalised median test,
    "unit" = 1 wherever the vector is finite, "uncertainty" = weights_from_uncertainty with the same zeros as "median"
    and `sigma` [n_rows, n_cols, 2], the vectors' uncertainty from ``PhotonLibrary.displacement_uncertainty``)."""
    from . import piv_correlation as pc
    if weights == "median":
        w = weights_from_correlation(vectors, flags, pc.normalized_median_test(vectors))
    elif weights == "unit":
        w = np.where(np.isfinite(np.asarray(vectors, np.float64)[..., :2]).all(axis=-1), 1.0, 0.0)
    elif weights == "uncertainty":
        if sigma is None:
            raise ValueError("weights='uncertainty' needs sigma, the uncertainty of the vectors")
        bad = weights_from_correlation(vectors, flags, pc.normalized_median_test(vectors)) == 0
        w = weights_from_uncertainty(sigma, flags, bad)
    else:
        raise ValueError(f"weights must be 'median', 'unit' or 'uncertainty', not {weights!r}")
    gx, gy = gradients_from_displacements(pc.sensor_displacements(vectors, call.camera), call.camera,
                                          displacement_factor(call, origin_z, extent_z, K, rho_0))
    target, mid, h = node_geometry(shape, win, step, call, origin_z, extent_z)
    return gx, gy, w, target, mid, h


def integrate_vectors(lib, vectors, flags, shape, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16,
                      weights: str = "median", tol: float = 1e-8, K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0, sigma=None):
    """Projected density from a correlation's vectors [n_rows, n_cols, >= 2] and flags on an image of `shape`: weights
    (`weights`: "median" = weights_from_correlation after the normalised median test, "unit" = 1 wherever the vector is
    finite, "uncertainty" = weights_from_uncertainty of `sigma`, the vectors' uncertainty), gradients, integration on the
    device with the frame fixed at P = 0 (the frame must lie where the density is ambient).  Returns (phi [n_rows, n_cols]
    kg/m^3 um, mid-plane nodes (X, Y), stats dict)."""
    gx, gy, w, _, mid, h = measured_gradients(vectors, flags, shape, call, origin_z, extent_z, win, step, weights, K, rho_0, sigma)
    phi, stats = lib.integrate_gradient(gx, gy, w, hx=h, hy=h, tol=tol)
    return phi, mid, stats


def _pair_uncertainty(lib, im1, im2, vectors, win, step, weights, reach):
    """sigma of the vectors measured on the pair when the weights ask for it (None otherwise)."""
    return lib.displacement_uncertainty(im1, im2, vectors, win=win, step=step, reach=reach)[0] if weights == "uncertainty" else None


def reconstruct(lib, im1, im2, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16, passes: int = 2,
                weights: str = "median", tol: float = 1e-8, K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0, reach: int = 2, mask=None):
    """Projected density from a BOS image pair (im1 without, im2 through the volume; torch device tensors or numpy):
    ``PhotonLibrary.correlate`` (`passes`), with weights="uncertainty" ``PhotonLibrary.displacement_uncertainty`` of the
    measured vectors on the same pair (`reach`), then integrate_vectors.  Returns (phi, mid-plane nodes (X, Y), stats).
    mask: pixels outside the dot pattern or behind a model, as ``PhotonLibrary.correlate`` takes them; a masked-out window's
    NaN vector gets weight 0, and a node without a live edge stays NaN."""
    vectors, flags = lib.correlate(im1, im2, win=win, step=step, passes=passes, **({} if mask is None else {"mask": mask}))
    sigma = _pair_uncertainty(lib, im1, im2, vectors, win, step, weights, reach)
    return integrate_vectors(lib, vectors, flags, tuple(int(v) for v in im1.shape), call, origin_z, extent_z, win, step, weights, tol, K, rho_0,
                             sigma)


def deflection_data(lib, im1, im2, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16, passes: int = 2,
                    weights: str = "median", K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0, reach: int = 2, mask=None):
    """The deflections of a BOS image pair, for tomography without the per-view integral (``reconstruct`` up to, but
    excluding, the integration): ``PhotonLibrary.correlate`` (`passes`), with weights="uncertainty"
    ``PhotonLibrary.displacement_uncertainty`` (`reach`), then measured_gradients.  Returns (g1, g2, w,
    target-plane nodes (X_t, Y_t)), g1 = gx and g2 = gy [n_rows, n_cols]: the data of
    ``PhotonLibrary.tomo_reconstruct_deflections`` with the rays of tomography.view_rays and the vectors of
    tomography.view_frames at the same nodes.  mask: as ``reconstruct`` takes it (weight 0 on masked-out nodes)."""
    vectors, flags = lib.correlate(im1, im2, win=win, step=step, passes=passes, **({} if mask is None else {"mask": mask}))
    gx, gy, w, target, _, _ = measured_gradients(vectors, flags, tuple(int(v) for v in im1.shape), call, origin_z, extent_z, win, step,
                                                 weights, K, rho_0, _pair_uncertainty(lib, im1, im2, vectors, win, step, weights, reach))
    return gx, gy, w, target


def reconstruct_tracked(lib, im1, im2, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16, threshold: float = 0.25,
                        relative: bool = True, min_count: int = 3, predict: bool = True, weights: str = "median", tol: float = 1e-8,
                        K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0, **track):
    """Projected density from a BOS image pair by dot tracking: ``PhotonLibrary.track_dots`` (`threshold`, `relative` and
    the keywords in `track`: box_radius, sigma_w, iterations, background, radius, max_dots) with the pairs averaged onto
    the (win, step) grid at the frame-1 anchor, windows of fewer than `min_count` dots taking weight 0, then
    integrate_vectors as ``reconstruct`` calls it.  predict: the pairing starts from one validated pass of window
    correlation on the same grid (``PhotonLibrary.correlation_predictor``) -- without it a shift that approaches the
    spacing of the dots pairs some of them with a neighbour, and those windows spoil the integral.  Returns (phi,
    mid-plane nodes (X, Y), stats)."""
    if predict and "predictor" not in track:
        track["predictor"] = (lib.correlation_predictor(im1, im2, win, step), win, step)
    res = lib.track_dots(im1, im2, threshold, relative=relative, grid=(win, step, min_count, 0), **track)
    return integrate_vectors(lib, res["vectors"], res["flags"], tuple(int(v) for v in im1.shape), call, origin_z, extent_z, win, step,
                             weights, tol, K, rho_0)


def reconstruct_flow(lib, im1, im2, call, origin_z: float, extent_z: float, win: int = 32, step: int = 16, alpha2: float = 5.0,
                     warps: int = 3, iterations: int = 48, tol: float = 1e-8, K: float = K_GLADSTONE_DALE, rho_0: float = RHO_0):
    """Projected density from a BOS image pair by dense optical flow: one iteration of ``PhotonLibrary.correlate_deform`` on
    the (win, step) grid as the predictor, ``PhotonLibrary.optical_flow`` from it (`alpha2`, `warps`, `iterations`), the
    dense field read at the window centres, then the integration of ``integrate_vectors``.  The weights are the
    predictor's: 0 where its correlation is flat or not finite or fails the normalised median test -- the flow starts from
    that vector and cannot be trusted to recover there -- 1 elsewhere.  Returns (phi, mid-plane nodes (X, Y), stats)."""
    from . import piv_correlation as pc
    pred, status = lib.correlate_deform(im1, im2, win=win, step=step, iterations=1)
    _, grid = lib.optical_flow(im1, im2, predictor=pred[..., :2], win=win, step=step, alpha2=alpha2, warps=warps, iterations=iterations,
                               return_grid=True)
    w = weights_from_correlation(pred, status, pc.normalized_median_test(pred))
    gx, gy, _, _, mid, h = measured_gradients(grid, status, tuple(int(v) for v in im1.shape), call, origin_z, extent_z, win, step, "unit", K,
                                              rho_0)
    phi, stats = lib.integrate_gradient(gx, gy, w, hx=h, hy=h, tol=tol)
    return phi, mid, stats
