"""Nine windows that between them take every branch of the peak tail the two window correlators share (flat, outside the
image, a peak on the plane's edge, clean), for tests/test_piv_correlation_gpu.py and tests/test_piv_phase_gpu.py: 48 x 48
noise, win 16, step 16, R 4."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def nine_windows():
    """(im1, im2 for section 5, im2 for section 13, section 13's offsets [3, 3, 2]), computed once."""
    rng = np.random.default_rng(7)
    im1, im2 = rng.random((48, 48)).astype(np.float32), rng.random((48, 48)).astype(np.float32)
    im2_phase = im2.copy()
    im1[:16, :16] = 0.25
    im2[16:32, 32:48] = 0.5
    im2_phase[0:14, 0:13] = 0.5
    off = np.zeros((3, 3, 2), np.int32)
    off[0, 0], off[1, 2], off[2, 1] = (-3, -2), (3, 0), (0, 2)
    return im1, im2, im2_phase, off
