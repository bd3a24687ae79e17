"""Case builders shared by tests/test_piv_deformation.py (CPU tier) and tests/test_piv_deformation_gpu.py: the analytic
particle pairs with a known displacement field, and the random vector grids of the validate step."""
import numpy as np

from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd

SHAPE, WIN, STEP, RADIUS = (256, 256), 32, 16, 16
SEEDS = (1, 2, 3, 4, 5)
PER_PIXEL, DIAMETER = 0.04, 2.5


def vortex(x, y, peak=5.3, core=30.0, centre=(127.5, 127.5)):
    """Lamb-Oseen-like vortex: tangential displacement A (1 - exp(-s^2)) / s, s = r / core, largest value `peak` px."""
    rx, ry = x - centre[0], y - centre[1]
    s = np.maximum(np.hypot(rx, ry) / core, 1e-12)
    v = peak / 0.6381726863 * (1.0 - np.exp(-s * s)) / s
    return -v * ry / (s * core), v * rx / (s * core)


def rotation(x, y, omega=0.05, centre=(127.5, 127.5)):
    return -omega * (y - centre[1]), omega * (x - centre[0])


def uniform(x, y, shift=(2.3, -1.4)):
    return np.full_like(x, shift[0]), np.full_like(y, shift[1])


FIELDS = {"vortex": vortex, "rotation": rotation, "uniform": uniform}


def pair(kind: str, seed: int, shape=SHAPE):
    """(im1, im2) f64: particles at p - d(p)/2 in frame 1 and p + d(p)/2 in frame 2 (the symmetric displacement)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    m = 24
    n = int(PER_PIXEL * (h + 2 * m) * (w + 2 * m))
    x, y = rng.uniform(-m, w + m, n), rng.uniform(-m, h + m, n)
    amp = rng.uniform(0.5, 1.0, n)
    dx, dy = FIELDS[kind](x, y)
    return (pc.particle_image(shape, x - dx / 2, y - dy / 2, DIAMETER, amp),
            pc.particle_image(shape, x + dx / 2, y + dy / 2, DIAMETER, amp))


def truth(kind: str, shape=SHAPE, win=WIN, step=STEP):
    """The displacement at the window centres, [n_rows, n_cols, 2]."""
    rows, cols = pc.window_centres(shape, win, step)
    return np.stack(FIELDS[kind](cols, rows), axis=-1)


def interior_rms(vectors, kind: str, shape=SHAPE, win=WIN, step=STEP):
    """RMS of |measured - truth| over the interior nodes (the outer ring of the grid left out: DESIGN.md 4.3d)."""
    e = np.asarray(vectors, np.float64)[1:-1, 1:-1, :2] - truth(kind, shape, win, step)[1:-1, 1:-1]
    return float(np.sqrt(np.mean((e * e).sum(axis=-1))))


def two_pass(correlate, im1, im2, win=WIN, step=STEP, radius=RADIUS):
    """The two-pass route of PhotonLibrary.correlate(passes=2) on any single-pass correlator(im1, im2, win, step, radius,
    offset) -> (vectors, flags)."""
    vec, flg = correlate(im1, im2, win, step, radius, None)
    off = pc.predictor(vec, flg, pc.normalized_median_test(vec))
    return correlate(im1, im2, win, step, radius, off)


def model_correlate(im1, im2, win, step, radius, offset):
    return pc.correlate_model(im1, im2, win, step, radius, offset=offset)


# ---- the validate step -------------------------------------------------------------------------------------------------
VALIDATE_GRIDS = [(2, 2), (2, 9), (3, 3), (1, 7), (7, 1), (5, 16), (16, 17), (17, 33), (31, 18), (40, 40), (63, 63), (64, 50), (127, 127)]


def validate_case(n_rows: int, n_cols: int, seed: int, with_pred: bool = True, outliers=0.05, nans=0.02, flats=0.02):
    """A smooth field plus noise, split into predictor and residual, with injected outliers, NaNs and flat flags.
    Returns (pred f32 [r, c, 2] or None, vectors f32 [r, c, 4], flags int32 [r, c])."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n_rows), np.arange(n_cols), indexing="ij")
    total = np.stack([3.0 * np.sin(0.21 * i + 0.1 * seed) + 0.08 * j, 2.0 * np.cos(0.17 * j) - 0.05 * i], axis=-1)
    total += rng.normal(0.0, 0.15, total.shape)
    bad = rng.random((n_rows, n_cols)) < outliers
    total[bad] += rng.uniform(-12.0, 12.0, (int(bad.sum()), 2))
    pred = (total + rng.normal(0.0, 0.4, total.shape)).astype(np.float32) if with_pred else None
    vec = np.empty((n_rows, n_cols, 4), np.float32)
    vec[..., :2] = total - (pred if with_pred else 0.0)
    vec[..., 2] = rng.uniform(0.3, 1.0, (n_rows, n_cols))
    vec[..., 3] = rng.uniform(1.0, 5.0, (n_rows, n_cols))
    nan = rng.random((n_rows, n_cols)) < nans
    vec[nan, rng.integers(0, 2, int(nan.sum()))] = np.nan
    vec[rng.random((n_rows, n_cols)) < 0.005, 0] = np.inf
    flags = rng.choice(np.array([0, 1, 4, 5], np.int32), size=(n_rows, n_cols), p=[0.85, 0.05, 0.05, 0.05])
    flat = rng.random((n_rows, n_cols)) < flats
    flags[flat] = pc.FLAG_FLAT
    vec[flat] = np.nan
    return pred, vec, flags.astype(np.int32)


def decided(score, threshold: float = 2.0, margin: float = 1e-9):
    """Nodes whose model score sqrt(r_x^2 + r_y^2) lies more than `margin` away from the threshold (NaN: no score, decided)."""
    with np.errstate(invalid="ignore"):
        s = np.sqrt(score)
    return ~(np.abs(s - threshold) <= margin)


def validate_cases():
    """(n_rows, n_cols, seed, with_pred) of every grid the device is held to, bit for bit."""
    return [(r, c, 100 + k, k % 3 != 0) for k, (r, c) in enumerate(VALIDATE_GRIDS)]
