"""Shared cases of the dot-tracking tests (test_dot_tracking.py, test_dot_tracking_gpu.py): the hand-made detection image,
isolated analytic dots, random point sets with a known pairing, and the analytic dot pairs of a Gaussian-blob gradient
field."""
import numpy as np

from photon_amd import piv_correlation as pc

# the analytic pairs of the chain tests: (dots per pixel, e^-2 diameter in pixels), seeds 1 .. 5 each
CHAIN_CASES = ((0.005, 4.0), (0.004, 5.4))
CHAIN_SEEDS = (1, 2, 3, 4, 5)
CHAIN = dict(threshold=0.25, box_radius=3, iterations=4, radius=3.0, relative=True)
MIN_TRACKED, MAX_WRONG = 0.80, 0.02


def hand_image():
    """(image f32 [9, 12], threshold, the exact peaks).  A plateau of two equal pixels (the first in row-major order
    counts), a maximum on the border (never a peak), a peak beside a NaN, a pixel equal to the threshold (no peak), an
    infinite pixel (no peak, and it hides its neighbours), and a diagonal plateau."""
    im = np.zeros((9, 12), np.float32)
    w = im.shape[1]
    im[1, 1] = im[1, 2] = 5.0                   # plateau along a row: (1, 1) precedes (1, 2)
    im[0, 6] = 9.0                              # on the border
    im[3, 5] = 4.0
    im[3, 6] = np.nan                           # a NaN neighbour passes
    im[5, 2] = 2.0                              # equal to the threshold
    im[5, 9] = np.inf
    im[6, 9] = 7.0                              # below an infinite neighbour
    im[6, 4] = im[7, 5] = 3.0                   # plateau along a diagonal: (6, 4) precedes (7, 5)
    im[7, 1] = 2.5
    return im, 2.0, [1 * w + 1, 3 * w + 5, 6 * w + 4, 7 * w + 1]


def isolated_dots(diameter: float, shape=(24, 24)):
    """25 images of one analytic dot at the sub-pixel offsets (-0.5 .. 0.5)^2 in steps of 0.25 from pixel (12, 12):
    (images f32 [25, h, w], centres [25, 2] = x, y)."""
    offs = np.linspace(-0.5, 0.5, 5)
    ims, xy = [], []
    for oy in offs:
        for ox in offs:
            ims.append(pc.particle_image(shape, [12.0 + ox], [12.0 + oy], diameter).astype(np.float32))
            xy.append((12.0 + ox, 12.0 + oy))
    return np.stack(ims), np.array(xy)


def point_sets(seed: int, n: int, shape=(200, 300), shift=(1.3, -0.7), extra2: int = 0, min_sep: float = 8.0):
    """Frame 1: n points at least min_sep apart; frame 2: the same points shifted, in a random order, plus extra2
    strangers.  Returns (dots1 f32 [n, 4], dots2 f32 [n + extra2, 4], truth [n]: the index in frame 2 of dot i)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    pts = []
    while len(pts) < n:
        c = rng.uniform((10, 10), (w - 10, h - 10))
        if all((c[0] - p[0]) ** 2 + (c[1] - p[1]) ** 2 >= min_sep ** 2 for p in pts):
            pts.append(c)
    p1 = np.array(pts).reshape(-1, 2)
    perm = rng.permutation(n + extra2)
    p2 = np.empty((n + extra2, 2))
    p2[perm[:n]] = p1 + np.asarray(shift)
    p2[perm[n:]] = rng.uniform((0, 0), (w, h), (extra2, 2))
    pad = lambda p: np.concatenate([p, np.ones((p.shape[0], 2))], axis=1).astype(np.float32)      # noqa: E731
    return pad(p1), pad(p2), perm[:n].astype(np.int32)


def blob_field(x, y, n_pix: int, peak: float = 1.5):
    """The shift of a Gaussian-blob gradient field centred on the image, sigma = n_pix / 6, |shift| = peak at r = sigma."""
    s = n_pix / 6.0
    cx = cy = (n_pix - 1) / 2.0
    g = peak * np.exp(0.5) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s)) / s
    return -(x - cx) * g, -(y - cy) * g


def analytic_pair(seed: int, density: float, diameter: float, n_pix: int = 512, peak: float = 1.5, noise: float = 0.01):
    """Random dots over the whole image, shifted by blob_field, Gaussian noise of `noise` x the brightest pixel on both
    frames.  Returns (im1, im2 f32, positions [n, 2] = x, y in frame 1, shifts [n, 2])."""
    rng = np.random.default_rng(seed)
    n = int(round(density * n_pix * n_pix))
    x, y = rng.uniform(0, n_pix, n), rng.uniform(0, n_pix, n)
    dx, dy = blob_field(x, y, n_pix, peak)
    im1 = pc.particle_image((n_pix, n_pix), x, y, diameter)
    im2 = pc.particle_image((n_pix, n_pix), x + dx, y + dy, diameter)
    sd = noise * im1.max()
    im1 = im1 + rng.normal(0.0, sd, im1.shape)
    im2 = im2 + rng.normal(0.0, sd, im2.shape)
    return im1.astype(np.float32), im2.astype(np.float32), np.stack([x, y], axis=1), np.stack([dx, dy], axis=1)


def chain_pairs(n_pix: int = 512):
    """The ten analytic pairs: yields (name, diameter, im1, im2, positions, shifts)."""
    for density, diameter in CHAIN_CASES:
        for seed in CHAIN_SEEDS:
            yield (f"{density} / {diameter} px, seed {seed}", diameter) + analytic_pair(seed, density, diameter, n_pix)


def detection_image(shape, seed: int, density: float = 0.005, diameter: float = 4.0, noise: float = 0.01):
    """One frame of dots of varying brightness on a noise floor, with a few NaN pixels: f32 [h, w]."""
    rng = np.random.default_rng(seed)
    h, w = shape
    n = max(1, int(density * h * w))
    im = pc.particle_image(shape, rng.uniform(0, w, n), rng.uniform(0, h, n), diameter, rng.uniform(0.5, 1.0, n))
    im = im + rng.normal(0.0, noise * im.max(), shape)
    im.ravel()[rng.integers(0, h * w, max(1, h * w // 5000))] = np.nan
    return im.astype(np.float32)
