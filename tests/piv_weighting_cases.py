"""Cases shared by tests/test_piv_weighting.py (CPU tier), tests/test_piv_weighting_gpu.py and
tests/test_zz_piv_weighting_perf_gpu.py: the weight tables, the flat-by-weight images, the driver pair, and the response
study -- a sinusoidal displacement of a wavelength near the window size, correlated with a top-hat and with a Gaussian
window."""
import functools

import numpy as np

import piv_deformation_cases as dc
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_multigrid as pm
from photon_amd import piv_weighting as pw


# ---- tables ---------------------------------------------------------------------------------------------------------------
def asymmetric(win: int) -> np.ndarray:
    """W = (1 + y)(1 + 2x) / win^2: no symmetry, so a transposed or mirrored table shows."""
    y, x = np.meshgrid(np.arange(win, dtype=np.float64), np.arange(win, dtype=np.float64), indexing="ij")
    return ((1.0 + y) * (1.0 + 2.0 * x) / win ** 2).astype(np.float32)


def holed(win: int) -> np.ndarray:
    """A Gaussian table with its four corner quarter-blocks at 0, one entry at -1 and one at NaN: the kernel and the model
    read all of them as 0."""
    w = pw.window_weights(win).copy()
    q = win // 4
    for ys in (slice(0, q), slice(win - q, win)):
        for xs in (slice(0, q), slice(win - q, win)):
            w[ys, xs] = 0.0
    w[win // 2, win // 3] = -1.0
    w[win // 3, win // 2 + 1] = np.nan
    return w


TABLES = {"gaussian": pw.window_weights, "asymmetric": asymmetric, "holed": holed}


def single(win: int, y: int, x: int) -> np.ndarray:
    w = np.zeros((win, win), np.float32)
    w[y, x] = 1.0
    return w


# ---- flat by weight ---------------------------------------------------------------------------------------------------------
def flat_by_weight():
    """(im1, im2, table) for win 16, step 16, R 4 on 16 x 32 noise: the table is 0 on its first four rows; window 0 of
    both frames is constant below them, so its only varying pixels sit under zero weights; window 1 is live everywhere."""
    rng = np.random.default_rng(11)
    im1, im2 = rng.random((16, 32)).astype(np.float32), rng.random((16, 32)).astype(np.float32)
    im1[4:, :16] = 0.3
    table = np.ones((16, 16), np.float32)
    table[:4] = 0.0
    return im1, im2, table


# ---- the drivers' pair --------------------------------------------------------------------------------------------------------
DRIVER_SHAPE = (97, 130)
DRIVER_KIND = "rotation"
DEFORM = dict(win=32, step=16, iterations=3)
MULTIGRID = dict(schedule=((32, 16), (16, 8)), iterations=(1, 2))


@functools.lru_cache(maxsize=None)
def driver_pair():
    im1, im2 = (c.astype(np.float32) for c in dc.pair(DRIVER_KIND, 1, DRIVER_SHAPE))
    for im in (im1, im2):
        im.setflags(write=False)
    return im1, im2


def driver_rms(vectors, win, step):
    return dc.interior_rms(vectors, DRIVER_KIND, DRIVER_SHAPE, win, step)


@functools.lru_cache(maxsize=None)
def driver_models():
    """The three drivers' models with weighting="gaussian" on driver_pair(), computed once: {name: (vectors, flags)}."""
    im1, im2 = driver_pair()
    return {"correlate": pw.correlate_weighted_model(im1, im2, pw.window_weights(32), 32, 16, 16),
            "correlate_deform": pd.correlate_deform_model(im1, im2, **DEFORM, weighting="gaussian"),
            "correlate_multigrid": pm.correlate_multigrid_model(im1, im2, **MULTIGRID, weighting="gaussian")}


# ---- the response study -----------------------------------------------------------------------------------------------------
R_SHAPE, R_WIN, R_STEP, R_RADIUS, R_RESIDUAL, R_ITERATIONS = (160, 256), 32, 8, 4, 4, 6
R_ARGS = dict(win=R_WIN, step=R_STEP, radius=R_RADIUS, residual_radius=R_RESIDUAL, smooth=False)
WAVELENGTHS = (24, 40)


@functools.lru_cache(maxsize=None)
def response_pair(lam: int, seed: int):
    """(im1, im2) f32: particles of 2.5 px at 0.04 per pixel, intensity 0.5 .. 1, displaced by dy = 1 px sin(2 pi x / lam),
    -dy / 2 in frame 1 and +dy / 2 in frame 2."""
    rng = np.random.default_rng(seed)
    h, w = R_SHAPE
    m = 24
    n = int(dc.PER_PIXEL * (h + 2 * m) * (w + 2 * m))
    x, y = rng.uniform(-m, w + m, n), rng.uniform(-m, h + m, n)
    amp = rng.uniform(0.5, 1.0, n)
    dy = np.sin(2.0 * np.pi * x / lam)
    im1 = pc.particle_image(R_SHAPE, x, y - dy / 2, dc.DIAMETER, amp).astype(np.float32)
    im2 = pc.particle_image(R_SHAPE, x, y + dy / 2, dc.DIAMETER, amp).astype(np.float32)
    for im in (im1, im2):
        im.setflags(write=False)
    return im1, im2


def amplitude(field, lam: int) -> float:
    """The least-squares amplitude of sin(2 pi x / lam) in the dy of a field on the study's grid, over the nodes at least two
    away from the border."""
    _, cols = pc.window_centres(R_SHAPE, R_WIN, R_STEP)
    s = np.sin(2.0 * np.pi * cols / lam)[2:-2, 2:-2]
    dy = np.asarray(field, np.float64)[2:-2, 2:-2, 1]
    assert np.isfinite(dy).all()
    return float((dy * s).sum() / (s * s).sum())


@functools.lru_cache(maxsize=None)
def model_response(lam: int, seed: int, weighting):
    """(amplitude after pass 0, after every iteration ...) of correlate_deform_model on the study's pair."""
    im1, im2 = response_pair(lam, seed)
    _, _, fields = pd.correlate_deform_model(im1, im2, **R_ARGS, iterations=R_ITERATIONS, history=True, weighting=weighting)
    return tuple(amplitude(f, lam) for f in fields)


def assert_response(uniform, gaussian):
    """The conditions of the study on {lam: amplitudes per pass} of the two windows (pass 0 first, the last iteration
    last): at 24 px the top hat answers with the wrong sign and the loop makes it worse, the Gaussian window stays positive
    on every pass and grows; at 40 px the Gaussian window's first pass recovers at least 0.15 more of the amplitude."""
    assert uniform[24][0] < 0.0 and uniform[24][-1] < uniform[24][0], uniform[24]
    assert min(gaussian[24]) > 0.0 and gaussian[24][-1] > gaussian[24][0], gaussian[24]
    assert gaussian[40][0] >= uniform[40][0] + 0.15, (gaussian[40][0], uniform[40][0])
