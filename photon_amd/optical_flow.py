"""Dense optical flow on an image pair (pure numpy: usable without a GPU).

The device forms are photon_piv_field_to_pixels, photon_piv_deform_dense, photon_optflow_terms and photon_optflow_iterate
(include/parallel_ray_tracing.h, section 12; ``PhotonLibrary.field_to_pixels`` / ``piv_deform_dense`` / ``optflow_terms`` /
``optflow_iterate`` on raw device pointers, ``PhotonLibrary.optical_flow`` on arrays).  This module holds

* ``terms_model`` and ``iterate_model``: the data terms and the Jacobi sweeps in numpy float32, operation for operation as
  section 12 states them (the device returns their bits);
* ``euler_lagrange_direct``: a sparse direct solve of the linear system the sweeps relax, on small images;
* ``optical_flow_model``: the driver's model, on the f64 coefficients and the f64 dense warp of piv_deformation;
* ``sample_at_window_centres``: a dense field read at section 5's window centres, for the consumers that take a grid.

Horn & Schunck (1981) with the linearisation about a predictor u0 (Brox et al. 2004): on the pair warped half-way by
u0 the increment du minimises  sum (Ix du + Iy dv + It)^2 + alpha2 |grad (u0 + du)|^2; the sweeps run on the total
u = u0 + du, and the pair is warped again by the result.  There is no pyramid: the predictor has to be within about a
particle diameter of the truth.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc
from . import piv_deformation as pd

F32 = np.float32


def _along(m: np.ndarray, axis: int, offset: int) -> np.ndarray:
    n = m.shape[axis]
    return np.take(m, pd.mirror_index(np.arange(n) + offset, n), axis=axis)


def _derivative(m: np.ndarray, axis: int) -> np.ndarray:
    return ((_along(m, axis, -2) - _along(m, axis, 2)) + F32(8) * (_along(m, axis, 1) - _along(m, axis, -1))) / F32(12)


def check_terms_arguments(shape, gain, alpha2):
    """The arguments photon_optflow_terms refuses, as a ValueError (null pointers aside)."""
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"the images must be 2-d and not empty, not {tuple(shape)}")
    for name, v in (("gain", gain), ("alpha2", alpha2)):
        if not (np.isfinite(F32(v)) and F32(v) > 0):
            raise ValueError(f"{name} must be finite and > 0, not {v}")


def terms_model(w1, w2, u0=None, gain: float = 1.0, alpha2: float = 5.0) -> np.ndarray:
    """Host model of photon_optflow_terms in f32.  w1, w2 [height, width]: the matched pair; u0 [height, width, 2] the field
    they were warped by, or None for zero.  Returns f32 [height, width, 4] = (Ix, Iy, c, w)."""
    w1, w2 = np.asarray(w1, F32), np.asarray(w2, F32)
    if w1.shape != w2.shape:
        raise ValueError("w1 and w2 must have one shape")
    check_terms_arguments(w1.shape, gain, alpha2)
    u0 = np.zeros(w1.shape + (2,), F32) if u0 is None else np.asarray(u0, F32)
    if u0.shape != w1.shape + (2,):
        raise ValueError(f"u0 must be {w1.shape + (2,)}, not {u0.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = F32(gain) * w1, F32(gain) * w2
        m = (a + b) * F32(0.5)
        ix, iy = _derivative(m, 1), _derivative(m, 0)
        it = b - a
        c = (it - ix * u0[..., 0]) - iy * u0[..., 1]
        w = F32(1) / ((F32(alpha2) + ix * ix) + iy * iy)
    return np.stack([ix, iy, c, w], axis=-1).astype(F32)


def _clamped_neighbours(a: np.ndarray):
    """a(q-1), a(q+1), a(r-1), a(r+1) of a [height, width] plane, indices clamped to the image."""
    e = np.pad(a, 1, mode="edge")
    return e[1:-1, :-2], e[1:-1, 2:], e[:-2, 1:-1], e[2:, 1:-1]


def iterate_model(terms, u, iterations: int) -> np.ndarray:
    """Host model of photon_optflow_iterate in f32: `iterations` Jacobi sweeps from u [height, width, 2] with the terms
    [height, width, 4] of terms_model.  Returns f32 [height, width, 2]."""
    t, u = np.asarray(terms, F32), np.array(u, F32)
    if int(iterations) < 0:
        raise ValueError(f"iterations must be >= 0, not {iterations}")
    if t.ndim != 3 or t.shape[2] != 4 or u.shape != t.shape[:2] + (2,):
        raise ValueError("terms must be [height, width, 4] and u [height, width, 2]")
    ix, iy, c, w = (t[..., k] for k in range(4))
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(int(iterations)):
            (ul, ur, uu, ud), (vl, vr, vu, vd) = _clamped_neighbours(u[..., 0]), _clamped_neighbours(u[..., 1])
            ub, vb = ((ul + ur) + (uu + ud)) * F32(0.25), ((vl + vr) + (vu + vd)) * F32(0.25)
            rho = ((ix * ub + iy * vb) + c) * w
            u = np.stack([ub - ix * rho, vb - iy * rho], axis=-1)
    return u


def euler_lagrange_direct(terms) -> np.ndarray:
    """The fixed point of the sweeps by a sparse direct solve in f64 (small images): with A the 4-neighbour average of
    iterate_model (indices clamped), the unknowns (u, v) satisfy  u - A u + Ix w (Ix A u + Iy A v + c) = 0  and the same
    with Iy for v.  Returns f64 [height, width, 2]."""
    from scipy.sparse import bmat, coo_matrix, diags, identity
    from scipy.sparse.linalg import spsolve
    t = np.asarray(terms, np.float64)
    h, w = t.shape[:2]
    n = h * w
    k = np.arange(n).reshape(h, w)
    nb = [np.pad(k, 1, mode="edge")[sl] for sl in ((slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)),
                                                   (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)))]
    A = coo_matrix((np.full(4 * n, 0.25), (np.tile(k.ravel(), 4), np.concatenate([b.ravel() for b in nb]))), shape=(n, n)).tocsr()
    ix, iy, c, wt = (t[..., j].ravel() for j in range(4))
    eye = identity(n, format="csr")
    system = bmat([[eye - A + diags(ix * wt * ix) @ A, diags(ix * wt * iy) @ A],
                   [diags(iy * wt * ix) @ A, eye - A + diags(iy * wt * iy) @ A]], format="csc")
    sol = spsolve(system, -np.concatenate([ix * wt * c, iy * wt * c]))
    return np.stack([sol[:n].reshape(h, w), sol[n:].reshape(h, w)], axis=-1)


def sample_at_window_centres(dense, win: int, step: int) -> np.ndarray:
    """A dense field [height, width, 2] read at section 5's window centres ((win - 1) / 2 + i step, bilinear between the
    pixels): f64 [n_rows, n_cols, 2], the grid every consumer of a correlation takes."""
    d = np.asarray(dense, np.float64)
    if d.ndim != 3 or d.shape[2] != 2:
        raise ValueError("the dense field must be [height, width, 2]")
    h, w = d.shape[:2]
    n_rows, n_cols = pc.grid_shape((h, w), win, step)

    def taps(n_pix, n):
        x = (int(win) - 1) / 2.0 + np.arange(n) * int(step)
        i0 = np.minimum(np.floor(x).astype(np.int64), n_pix - 1)
        return i0, np.minimum(i0 + 1, n_pix - 1), x - i0
    i0, i1, fy = taps(h, n_rows)
    j0, j1, fx = taps(w, n_cols)
    fy, fx = fy[:, None, None], fx[None, :, None]
    top = d[i0][:, j0] + fx * (d[i0][:, j1] - d[i0][:, j0])
    bot = d[i1][:, j0] + fx * (d[i1][:, j1] - d[i1][:, j0])
    return top + fy * (bot - top)


def predictor_shape(predictor_shape_, shape, win: int, step: int) -> str:
    """'dense' for [height, width, 2], 'grid' for [n_rows, n_cols, >= 2] on section 5's grid; anything else: ValueError."""
    h, w = (int(v) for v in shape)
    ps = tuple(int(v) for v in predictor_shape_)
    if ps == (h, w, 2):
        return "dense"
    if len(ps) == 3 and ps[2] >= 2 and ps[:2] == pc.grid_shape((h, w), win, step):
        return "grid"
    r, c = pc.grid_shape((h, w), win, step)
    raise ValueError(f"the predictor must be [{h}, {w}, 2] (dense) or [{r}, {c}, >= 2] (the grid of win {win}, step {step}), not {list(ps)}")


def check_driver_arguments(alpha2, warps, iterations):
    if not (np.isfinite(alpha2) and alpha2 > 0):
        raise ValueError(f"alpha2 must be finite and > 0, not {alpha2}")
    if int(warps) < 0 or int(iterations) < 0:
        raise ValueError(f"warps and iterations must be >= 0, not {warps}, {iterations}")


def optical_flow_model(im1, im2, predictor=None, win: int = 32, step: int = 16, alpha2: float = 5.0, warps: int = 3,
                       iterations: int = 48, return_grid: bool = False):
    """Host model of PhotonLibrary.optical_flow.  predictor: a vector grid [n_rows, n_cols, >= 2] of (win, step), spread to
    the pixels by piv_deformation.dense_field; or a dense field [height, width, 2]; or None: one iteration of
    correlate_deform_model.  The images are scaled by gain = 1 / std(im1), so that alpha2 has one meaning whatever the
    exposure; per warp both frames are warped half-way by the current field (f64 coefficients, f64 warp, the result rounded
    to f32), then terms_model and `iterations` sweeps of iterate_model.  Returns the dense field f32 [height, width, 2]; with
    return_grid also sample_at_window_centres of it."""
    im1, im2 = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    if im1.ndim != 2 or im1.shape != im2.shape:
        raise ValueError("im1 and im2 must be two 2-d images of one shape")
    check_driver_arguments(alpha2, warps, iterations)
    if predictor is None:
        predictor = pd.correlate_deform_model(im1, im2, win, step, iterations=1)[0][..., :2]
    if predictor_shape(np.shape(predictor), im1.shape, win, step) == "grid":
        predictor = pd.dense_field(predictor, im1.shape, win, step)
    u = np.asarray(predictor, F32)
    gain = 1.0 / float(np.std(im1.astype(F32), dtype=np.float64))
    c1, c2 = pd.bspline_coefficients_model(im1), pd.bspline_coefficients_model(im2)
    for _ in range(int(warps)):
        w1, w2 = pd.deform_dense_model(c1, u, -0.5).astype(F32), pd.deform_dense_model(c2, u, 0.5).astype(F32)
        u = iterate_model(terms_model(w1, w2, u, gain, alpha2), u, iterations)
    return (u, sample_at_window_centres(u, win, step)) if return_grid else u
