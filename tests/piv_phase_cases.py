"""Case builders shared by tests/test_piv_phase.py (CPU tier) and tests/test_piv_phase_gpu.py: the particle pair on a
stationary background that amplitude correlation loses, the small pairs the device is held to value for value, and the
exactly periodic integer patterns whose cross spectrum is 0 in all but a few bins."""
import functools

import numpy as np

from photon_amd import piv_correlation as pc
from photon_amd import piv_phase as pp

# ---- the background pair: 2.5 px particles at 0.02 per pixel shifted by (2.3, -1.6) px, N(0, 0.02) noise per frame, and the
#      same smooth background 0.5 (1 + sin(x / 9) cos(y / 13)) in both frames
BG_SHAPE, BG_SHIFT, BG_WIN, BG_STEP, BG_RADIUS, BG_DIAMETER = (160, 160), (2.3, -1.6), 32, 16, 8, 2.5


@functools.lru_cache(maxsize=None)
def background_pair(seed: int = 1):
    rng = np.random.default_rng(seed)
    h, w = BG_SHAPE
    m = 8
    n = int(0.02 * (h + 2 * m) * (w + 2 * m))
    x, y = rng.uniform(-m, w + m, n), rng.uniform(-m, h + m, n)
    rows, cols = np.mgrid[:h, :w]
    background = 0.5 * (1.0 + np.sin(cols / 9.0) * np.cos(rows / 13.0))
    im1 = pc.particle_image(BG_SHAPE, x, y, BG_DIAMETER) + background + rng.normal(0.0, 0.02, BG_SHAPE)
    im2 = pc.particle_image(BG_SHAPE, x + BG_SHIFT[0], y + BG_SHIFT[1], BG_DIAMETER) + background + rng.normal(0.0, 0.02, BG_SHAPE)
    return im1.astype(np.float32), im2.astype(np.float32)


def valid(vectors, shift=BG_SHIFT, within: float = 0.5):
    """The vectors within `within` px of the true shift, bool [n_rows, n_cols] (a NaN vector is not)."""
    v = np.asarray(vectors, np.float64)
    with np.errstate(invalid="ignore"):
        return np.hypot(v[..., 0] - shift[0], v[..., 1] - shift[1]) < within


# ---- the small pairs of the device comparison
def particle_pair(shape, shift, seed, per_px=0.03, noise=0.02):
    rng = np.random.default_rng(seed)
    h, w = shape
    n = int(per_px * (h + 16) * (w + 16))
    x, y = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n)
    amp = rng.uniform(0.5, 1.0, n)
    im1 = pc.particle_image(shape, x, y, 2.5, amp) + noise * rng.random(shape)
    im2 = pc.particle_image(shape, x + shift[0], y + shift[1], 2.5, amp) + noise * rng.random(shape)
    return im1.astype(np.float32), im2.astype(np.float32)


# (win, R, step, (height, width), shift, with offsets, mode, window_sigma, diameter): every win with R = 1, a middle value and
# win/2 - 1, steps below and equal to win, image sides that are no multiple of the step, both modes, both weightings
DEVICE_CASES = [
    (16, 1, 8, (70, 90), (0.4, -0.3), False, 1, 4.0, 2.5),
    (16, 4, 16, (63, 101), (2.3, 1.6), True, 0, 0.0, 0.0),
    (16, 7, 5, (53, 61), (-3.2, 4.7), False, 1, 0.0, 2.5),
    (32, 1, 32, (97, 131), (0.2, 0.6), True, 1, 8.0, 0.0),
    (32, 8, 16, (101, 75), (-4.6, 2.2), True, 1, 8.0, 2.5),
    (32, 15, 12, (139, 131), (7.4, -5.9), False, 0, 8.0, 0.0),
    (64, 1, 40, (139, 190), (-0.6, 0.3), False, 0, 16.0, 2.5),
    (64, 16, 24, (130, 171), (5.5, 9.2), True, 1, 16.0, 2.5),
    (64, 31, 64, (140, 200), (-12.3, 17.8), True, 1, 0.0, 0.0),
]


def case_id(c):
    return f"w{c[0]}_r{c[1]}_s{c[2]}_{c[3][0]}x{c[3][1]}{'_off' if c[5] else ''}_m{c[6]}_g{c[7]:g}_d{c[8]:g}"


@functools.lru_cache(maxsize=None)
def device_case(index: int):
    """(im1, im2, offset or None, the f32 model's (vectors, flags, planes)) of DEVICE_CASES[index], computed once."""
    win, R, step, shape, shift, with_off, mode, sigma, diameter = DEVICE_CASES[index]
    im1, im2 = particle_pair(shape, shift, seed=1000 + index)
    off = None
    if with_off:            # up to 3 px either way: the windows along the image's edges are pushed off it
        off = np.random.default_rng(index).integers(-3, 4, size=pc.grid_shape(shape, win, step) + (2,)).astype(np.int32)
    want = pp.correlate_phase_model_f32(im1, im2, win, step, R, offset=off, mode=mode, window_sigma=sigma, diameter=diameter, planes=True)
    return im1, im2, off, want


# ---- exactly periodic integer patterns: all but 1 to 4 bins of the cross spectrum are 0 in f32
def periodic_pair(kind: str, shape=(96, 128)):
    rows, cols = np.mgrid[:shape[0], :shape[1]]
    if kind == "checkerboard":
        im1, im2 = (rows + cols) % 2, (rows + cols + 1) % 2
    elif kind == "stripes":
        im1, im2 = (cols % 4 < 2) * 3, ((cols + 1) % 4 < 2) * 3
    else:
        raise ValueError(kind)
    return im1.astype(np.float32), im2.astype(np.float32)
