"""Shared cases of the pre-processing tests (test_piv_preprocess.py, test_piv_preprocess_gpu.py; section 15 of
include/parallel_ray_tracing.h):

* the wall series the feature is for: N pairs of fresh particles under a Gaussian light sheet, in front of a stationary
  speckle three times as bright and an intensity ramp.  Correlated raw, every window locks on the wall at zero shift; with
  the stack's own minimum subtracted the particles are what is left;
* particle stacks with an offset, for the bit-for-bit and the f32-against-f64 tests.
"""
import functools

import numpy as np

from photon_amd import piv_correlation as pc
from photon_amd import piv_preprocess as pp

WALL_SHAPE, WALL_SHIFT, WALL_WIN, WALL_STEP, WALL_R, WALL_PAIRS = (96, 96), (2.3, -1.6), 32, 16, 6, 8
WALL_WITHIN = 0.3               # px: a window counts when its vector is this close to the true shift
WALL_RADIUS, WALL_FLOOR = 5, 0.05


@functools.lru_cache(maxsize=None)
def wall_series(seed: int, n_pairs: int = WALL_PAIRS):
    """(frames1, frames2) f32 [n_pairs, 96, 96], read-only.  Per pair: particles at 0.02 per pixel (diameter 2.5 px, amplitude
    0.5 to 1) shifted by WALL_SHIFT between the frames, under the sheet 0.15 + 0.85 exp(-((y - h/2) / (0.25 h))^2).  In every
    frame: the same wall speckle (0.02 blobs per pixel, diameter 2 px, amplitude 1.5 to 3), the ramp 0.5 x / w, and fresh
    uniform noise of 0.02."""
    rng = np.random.default_rng(seed)
    h, w = WALL_SHAPE
    n_wall = int(0.02 * h * w)
    wall = pc.particle_image(WALL_SHAPE, rng.uniform(0, w, n_wall), rng.uniform(0, h, n_wall), 2.0, 3.0 * rng.uniform(0.5, 1.0, n_wall))
    wall = wall + 0.5 * np.arange(w)[None, :] / w
    sheet = (0.15 + 0.85 * np.exp(-(((np.arange(h) - h / 2) / (0.25 * h)) ** 2)))[:, None]
    a, b = [], []
    for _ in range(n_pairs):
        n = int(0.02 * (h + 16) * (w + 16))
        x, y, amp = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n), rng.uniform(0.5, 1.0, n)
        a.append(sheet * pc.particle_image(WALL_SHAPE, x, y, 2.5, amp) + wall + 0.02 * rng.random(WALL_SHAPE))
        b.append(sheet * pc.particle_image(WALL_SHAPE, x + WALL_SHIFT[0], y + WALL_SHIFT[1], 2.5, amp) + wall + 0.02 * rng.random(WALL_SHAPE))
    a, b = np.stack(a).astype(np.float32), np.stack(b).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def near_truth(vectors, shift=WALL_SHIFT, within: float = WALL_WITHIN):
    """The number of vectors within `within` px of the true shift (a NaN vector is not)."""
    v = np.asarray(vectors, np.float64)
    with np.errstate(invalid="ignore"):
        return int((np.hypot(v[..., 0] - shift[0], v[..., 1] - shift[1]) < within).sum())


@functools.lru_cache(maxsize=None)
def wall_processed(seed: int, radius: int):
    """The wall series through the models: each stack minus its own minimum, then the filter (radius 0: none)."""
    return tuple(pp.preprocess_model_f32(s, pp.background_model(s, pp.MODE_MIN), radius, WALL_FLOOR if radius else None)
                 for s in wall_series(seed))


@functools.lru_cache(maxsize=None)
def particle_frames(shape, n_frames: int, seed: int, offset: float = 0.1):
    """f32 [n_frames, height, width], read-only: fresh particles per frame (0.03 per pixel) on a constant offset with uniform
    noise of 0.02 -- every pixel positive, the local contrast from nothing to a whole particle."""
    rng = np.random.default_rng(seed)
    h, w = shape
    out = []
    for _ in range(n_frames):
        n = max(int(0.03 * (h + 16) * (w + 16)), 1)
        out.append(pc.particle_image(shape, rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n), 2.5, rng.uniform(0.5, 1.0, n))
                   + offset + 0.02 * rng.random(shape))
    f = np.stack(out).astype(np.float32)
    f.setflags(write=False)
    return f
