"""What the stereo PIV tests share (tests/test_piv_stereo.py on the CPU, tests/test_piv_stereo_gpu.py on the device): the two
calibrated camera pairs, the three accuracy pairs with the model chain's figures on them (computed once), and the folded
cameras, images and fields the dewarp and reconstruction cases run on.  Everything is cached and read-only."""
import functools

import numpy as np

from photon_amd import piv_stereo as ps

PLANE, SENSOR = ps.CASE_PLANE, ps.CASE_SENSOR
WIN, STEP, RADIUS, ITERATIONS = (ps.CASE_GRID[k] for k in ("win", "step", "radius", "iterations"))
ANGLES, ACCURACY = ps.CASE_ANGLES, ps.CASES


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def calibrated(kind):
    return ps.calibrated_pair(kind)


def cameras(kind):
    return tuple(c[1] for c in calibrated(kind))


@functools.lru_cache(maxsize=None)
def accuracy_pair(name):
    """(cam1 frames, cam2 frames) f32 [2, 224, 256] of one accuracy case."""
    return tuple(frozen(f) for f in ps.case_pair(name)[:2])


figures = ps.case_figures


@functools.lru_cache(maxsize=None)
def model_figures(name):
    f1, f2 = accuracy_pair(name)
    out, _, (v1, _) = ps.correlate_stereo_model(f1, f2, cameras(ACCURACY[name][0]), PLANE, WIN, STEP, RADIUS, ITERATIONS)
    return figures(name, out, v1)


# ---- dewarp ------------------------------------------------------------------------------------------------------------------
def image(shape, seed, n=1):
    """f32 [n, h, w]: smooth structure plus noise, values of order 1 with both signs."""
    rng = np.random.default_rng(seed)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    out = [np.sin(0.31 * x + 0.17 * y + k) + 0.5 * np.cos(0.23 * y - 0.11 * x) + rng.normal(0.0, 0.3, (h, w)) for k in range(n)]
    return frozen(np.stack(out).astype(np.float32))


UNIT_GRID = (0.0, 1.0, 0.0, 1.0)        # u = j, v = i


def affine(x0, xu, xv, y0, yu, yv):
    """(poly, grid) of x = x0 + xu j + xv i, y = y0 + yu j + yv i."""
    poly = np.zeros((2, 10))
    poly[0, :3], poly[1, :3] = (x0, xu, xv), (y0, yu, yv)
    return poly, np.array(UNIT_GRID)


def fit_to(src, out):
    """The output grid stretched over the whole source (src and out as (height, width))."""
    return affine(0.0, (src[1] - 1) / max(out[1] - 1, 1), 0.0, 0.0, 0.0, (src[0] - 1) / max(out[0] - 1, 1))


def full_camera(src, out, seed=3):
    """A camera with all 38 coefficients nonzero that maps the plane of `out` into most of `src`, folded off its centre
    plane (w = 0.35, so that every Z term enters): (poly, grid, camera, plane)."""
    rng = np.random.default_rng(seed)
    (h, w), (oh, ow) = src, out
    cx, cy = (rng.uniform(0.005, 0.02, 19) * rng.choice([-1.0, 1.0], 19) * s for s in (w, h))
    cx[0], cx[1], cy[0], cy[2] = 0.5 * (w - 1), 0.42 * w, 0.5 * (h - 1), 0.42 * h
    cam = ps.camera((0.5 * (ow - 1), 0.5 * (oh - 1), 0.3), (0.5 * ow, 0.5 * oh, 2.0), cx, cy)
    pl = ps.plane(0.0, 0.0, 1.0, 1.0, ow, oh)
    assert (cam["cx"] != 0).all() and (cam["cy"] != 0).all()
    return (*ps.plane_coefficients(cam, pl), cam, pl)


def overflowing():
    """x = j + 1e300 u^3 - 1e300 u v^2 with (u, v) = 1000 (j, i): 0 in column 0 of the first rows, huge beyond, +inf from
    column 14 on, and inf - inf = NaN where row and column are both >= 14; y = i."""
    poly = np.zeros((2, 10))
    poly[0, 1], poly[0, 6], poly[0, 8], poly[1, 2] = 1e-3, 1e300, -1e300, 1e-3
    return poly, np.array([0.0, 1000.0, 0.0, 1000.0])


SRC = (23, 37)                                          # height, width
OUTS = ((50, 19), (5, 130))                             # neither a multiple of the 4 x 64 block; each with one side beyond the source


def dewarp_cameras(src, out):
    """name -> (poly, grid) of the cameras every dewarp shape runs."""
    h, w = src
    oh, ow = out
    return {
        "fit": fit_to(src, out),
        "full": full_camera(src, out)[:2],
        "rotated": affine(0.0, 0.0, (w - 1) / max(oh - 1, 1), 0.0, (h - 1) / max(ow - 1, 1), 0.0),       # x from the row, y from the column
        "half": affine(0.25, 0.5, 0.0, 0.125, 0.0, 0.5),
        "double": affine(0.0, 2.0, 0.0, 0.0, 0.0, 2.0),
        "partly_outside": affine(-5.3, 1.0, 0.02, -1.7, 0.01, 0.9),
        "all_outside": affine(1000.0, 1.0, 0.0, 0.0, 0.0, 1.0),
        "overflow": overflowing(),
    }


# ---- reconstruction ----------------------------------------------------------------------------------------------------------
GRIDS = {"1x1": (32, 32), "1x7": (32, 128), "9x11": (160, 192)}        # plane (height, width) at win 32, step 16


def stereo_inputs(grid, seed=11):
    """Random fields [r, c, 4], flags and sigmas of the two cameras on the grid `grid` of GRIDS, with NaN vectors and
    section 5's flag bits sprinkled in (not on the 1 x 1 grid's only node): (plane, fields, flags, sigmas)."""
    h, w = GRIDS[grid]
    pl = ps.centred_plane(w, h, 0.2)
    r, c = (h - WIN) // STEP + 1, (w - WIN) // STEP + 1
    rng = np.random.default_rng(seed)
    fields = [rng.uniform(-3.0, 3.0, (r, c, 4)).astype(np.float32) for _ in range(2)]
    flags = [rng.choice([0, 0, 0, 1, 4, 8], (r, c)).astype(np.int32) for _ in range(2)]
    sigmas = [rng.uniform(0.02, 0.2, (r, c, 2)).astype(np.float32) for _ in range(2)]
    if r * c > 1:
        fields[0][0, 1, 0], flags[0][0, 1] = np.nan, 2
        fields[1][0, c - 1, 1], flags[1][0, c - 1] = np.inf, 2
        sigmas[0][0, 2, 1] = np.nan
    return pl, [frozen(f) for f in fields], [frozen(f) for f in flags], [frozen(s) for s in sigmas]
