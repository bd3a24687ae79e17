"""Shared cases of the gradient-integration tests (test_bos_density.py, test_bos_density_gpu.py): random weighted grids,
biquadratic fields, the analytic Gaussian projection, and the rendered BOS scene of an off-centre Gaussian blob."""
import os

import numpy as np

from photon_amd import bos_density as bd


def random_case(seed: int, ny: int, nx: int, nan_frac: float = 0.03, zero_frac: float = 0.08, fixed_frac=None):
    """A random weighted problem: gradients, weights with zeros, NaN gradients, and a random fixed mask with values (None
    = the default frame, 0 values)."""
    rng = np.random.default_rng(seed)
    gx, gy = rng.normal(size=(2, ny, nx))
    w = rng.uniform(0.1, 3.0, (ny, nx))
    w[rng.random((ny, nx)) < zero_frac] = 0.0
    gx[rng.random((ny, nx)) < nan_frac] = np.nan
    gy[rng.random((ny, nx)) < nan_frac] = np.nan
    if fixed_frac is None:
        return dict(gx=gx, gy=gy, w=w, fixed=None, value=None)
    fixed = (rng.random((ny, nx)) < fixed_frac).astype(np.uint8)
    value = rng.normal(size=(ny, nx))
    return dict(gx=gx, gy=gy, w=w, fixed=fixed, value=value)


def biquadratic(ny: int, nx: int, hx: float, hy: float):
    """phi of degree <= 2 in x and in y separately, its exact gradient (gx along columns, gy along rows)."""
    y, x = np.meshgrid(np.arange(ny) * hy - 0.4 * ny * hy, np.arange(nx) * hx - 0.6 * nx * hx, indexing="ij")
    phi = 1.0 + x - 2.0 * y + 0.5 * x * x + 0.3 * x * y - 0.7 * y * y + 0.1 * x * x * y * y - 0.2 * x * x * y
    gx = 1.0 + x + 0.3 * y + 0.2 * x * y * y - 0.4 * x * y
    gy = -2.0 + 0.3 * x - 1.4 * y + 0.2 * x * x * y - 0.2 * x * x
    return phi, gx, gy


def gaussian_case(n: int, sigma: float = 1.2, extent: float = 10.0, amplitude: float = 1.0):
    """The analytic Gaussian projection A sigma sqrt(2 pi) exp(-r^2 / 2 sigma^2) on an n x n grid over `extent`, its exact
    gradient, and the spacing."""
    h = extent / (n - 1)
    c = np.arange(n) * h - extent / 2
    y, x = np.meshgrid(c, c, indexing="ij")
    P = bd.gaussian_projection(x * x + y * y, amplitude, sigma)
    return P, -x / sigma ** 2 * P, -y / sigma ** 2 * P, h


# ---- the rendered BOS scene of an off-centre Gaussian blob -------------------------------------------------------------
N_PIX, WIN, STEP = 512, 32, 16
VOL_N, EXTENT, ORIGIN_Z = 128, 66300.0, 300000.0
BLOB = dict(centre=(2000.0, -1500.0, ORIGIN_Z + EXTENT / 2), sigma=2500.0, amplitude=2.0)
N_DOTS, DOT_POINTS, DOT_RAYS, DOT_DIAMETER = 6000, 16, 60, 250.0


def blob_rho(x, y, z):
    cx, cy, cz = BLOB["centre"]
    s = BLOB["sigma"]
    return bd.RHO_0 + BLOB["amplitude"] * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))


def blob_calls(photon, workdir: str, diffraction: bool, n_pix: int = N_PIX):
    """(call without the volume, call through the blob's NRRD) at an n_pix^2 sensor (the dot density of N_DOTS on
    N_PIX^2); the erf splat when diffraction."""
    from photon_amd import scenes
    h = EXTENT / (VOL_N - 1)
    origin = (-EXTENT / 2, -EXTENT / 2, ORIGIN_Z)
    path = os.path.join(workdir, "blob.nrrd")
    if not os.path.exists(path):
        photon.density_gaussian_write_nrrd(path, VOL_N, h, origin, bd.RHO_0, BLOB["amplitude"], BLOB["centre"], BLOB["sigma"])
    f = n_pix / N_PIX
    kw = dict(n_dots=int(N_DOTS * f * f), points_per_dot=DOT_POINTS, rays_per_source=DOT_RAYS, seed=11, field_half_width=2.8e4 * f,
              dot_diameter=DOT_DIAMETER, n_pixels=n_pix)
    calls = [scenes.bos_scene(**kw), scenes.bos_scene(density_grad_filename=path, **kw)]
    for c in calls:
        c.camera["implement_diffraction"] = bool(diffraction)
    return calls


def truth(call, n_pix: int = N_PIX):
    """The chief-ray projection of the analytic blob at the correlation grid's nodes, the mid-plane nodes and h."""
    target, mid, h = bd.node_geometry((n_pix, n_pix), WIN, STEP, call, ORIGIN_Z, EXTENT)
    P = bd.chief_ray_projection(blob_rho, target, call.object_distance, (ORIGIN_Z, ORIGIN_Z + EXTENT))
    return P, mid, h


def errors(phi, P, mid, h):
    """(relative L2 error over the nodes above 10 % of the peak where phi is finite, argmax offset from the blob's centre in
    grid steps (x, y), the share of those nodes left NaN: weight-0 nodes have no live edge)."""
    high = P > 0.1 * P.max()
    use = high & np.isfinite(phi)
    rel = float(np.linalg.norm((phi - P)[use]) / np.linalg.norm(P[use]))
    k = np.unravel_index(np.nanargmax(phi), phi.shape)
    off = ((mid[0][k] - BLOB["centre"][0]) / h, (mid[1][k] - BLOB["centre"][1]) / h)
    return rel, off, float(1.0 - use.sum() / high.sum())
