"""Cases shared by tests/test_piv_uncertainty.py (CPU tier) and tests/test_piv_uncertainty_gpu.py: the noisy matched pairs
the kernel is held to its model on, and the calibration pairs with a known displacement."""
import functools

import numpy as np

import piv_deformation_cases as dc
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_uncertainty as pu

# (shape, win, step): a tile that is no multiple of the window, a step that is none of the window, one single window,
# more rows than columns and the reverse, every window size; each at every reach of REACHES
GRIDS = [((64, 64), 16, 8), ((64, 64), 32, 8), ((64, 64), 64, 1), ((97, 130), 32, 16), ((130, 97), 16, 5), ((256, 256), 32, 16),
         ((256, 256), 64, 32)]
REACHES = (0, 1, 2, 3, 4)                      # every reach the entry point accepts: odd ones pad the LDS rows to reach + 1
CASES = [(shape, win, step, reach) for shape, win, step in GRIDS for reach in REACHES]
NOISE = 0.03


def case_id(case):
    (h, w), win, step, reach = case
    return f"{h}x{w}-win{win}-step{step}-K{reach}"


def frame(shape, seed=7):
    """Section 7's test image with a floor of 0.05: particles (0.03 per pixel, diameter 2.5) on uniform noise, f64."""
    rng = np.random.default_rng(seed)
    h, w = shape
    n = int(0.03 * h * w)
    return pc.particle_image(shape, rng.uniform(0, w, n), rng.uniform(0, h, n), 2.5, rng.uniform(0.5, 1.0, n)) + 0.05 * rng.random(shape)


@functools.lru_cache(maxsize=None)
def matched_pair(shape):
    """(im1, im2) f32: the same frame under two draws of Gaussian noise N(0, 0.03) -- a pair that is matched already."""
    f, rng = frame(shape), np.random.default_rng(8)
    return (f + rng.normal(0.0, NOISE, shape)).astype(np.float32), (f + rng.normal(0.0, NOISE, shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model(case):
    """(sigma, flags, stats, T) of the model on a case: computed once, shared, never written to."""
    shape, win, step, reach = case
    out = pu.uncertainty_model(*matched_pair(shape), win, step, reach)
    for a in out:
        a.setflags(write=False)
    return out


def n_terms(reach: int) -> int:
    """N = 1 + 2 |H_K|: the shifted sums in V, each counted as often as it enters."""
    return 1 + 2 * len(pu.half_neighbourhood(reach))


def energies(case):
    """sqrt(sum A^2 sum B^2) per window: the scale of C0 and C1."""
    shape, win, step, _ = case
    a, b = (np.lib.stride_tricks.sliding_window_view(im.astype(np.float64), (win, win))[::step, ::step] for im in matched_pair(shape))
    A, B = (x - x.mean(axis=(-2, -1), keepdims=True) for x in (a, b))
    return np.sqrt((A * A).sum(axis=(-2, -1)) * (B * B).sum(axis=(-2, -1)))


# ---- calibration: pairs with a known displacement and added image noise -----------------------------------------------
CAL_SEEDS = (1, 2, 3, 4)
CAL_BOUND = (0.6, 1.2)          # rms sigma / std(error) per component


@functools.lru_cache(maxsize=None)
def noisy_pair(kind: str, seed: int, noise: float):
    """piv_deformation_cases.pair plus Gaussian image noise from default_rng(1000 + seed), rounded to f32."""
    im1, im2 = dc.pair(kind, seed)
    rng = np.random.default_rng(1000 + seed)
    return (im1 + rng.normal(0.0, noise, im1.shape)).astype(np.float32), (im2 + rng.normal(0.0, noise, im2.shape)).astype(np.float32)


def interior_error(vectors, kind: str):
    """measured - truth over the interior nodes, the mean removed per component: [n, 2]."""
    e = (np.asarray(vectors, np.float64)[..., :2] - dc.truth(kind))[1:-1, 1:-1].reshape(-1, 2)
    return e - e.mean(axis=0)


def calibration(errors, sigmas):
    """(rms sigma / std(error) per component, share of |error| <= sigma per component) of pooled interior nodes: lists
    of [n, 2] arrays."""
    e, s = np.concatenate(errors), np.concatenate(sigmas)
    return np.sqrt((s * s).mean(axis=0)) / np.sqrt((e * e).mean(axis=0)), (np.abs(e) <= s).mean(axis=0)


@functools.lru_cache(maxsize=None)
def model_calibration(kind: str, noise: float, reach: int = 2):
    """The model chain on CAL_SEEDS: correlate_deform_model (3 iterations), displacement_uncertainty_model.  Returns (ratio
    [2], coverage [2], rms sigma)."""
    errors, sigmas = [], []
    for seed in CAL_SEEDS:
        im1, im2 = noisy_pair(kind, seed, noise)
        vec, _ = pd.correlate_deform_model(im1, im2, dc.WIN, dc.STEP, iterations=3)
        sigma, _, _, _ = pu.displacement_uncertainty_model(im1, im2, vec, dc.WIN, dc.STEP, reach)
        errors.append(interior_error(vec, kind))
        sigmas.append(sigma[1:-1, 1:-1].reshape(-1, 2))
    ratio, cover = calibration(errors, sigmas)
    return ratio, cover, float(np.sqrt(np.mean(np.concatenate(sigmas) ** 2)))
