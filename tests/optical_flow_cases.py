"""Cases shared by tests/test_optical_flow.py (CPU tier) and tests/test_optical_flow_gpu.py: random data terms, matched
pairs, the analytic pairs of piv_deformation_cases with their per-pixel truth, and the bounds both tiers are held to."""
import functools

import numpy as np

import piv_deformation_cases as dc
from photon_amd import optical_flow as of
from photon_amd import piv_deformation as pd

ALPHA2, WARPS, ITERATIONS = 5.0, 3, 48          # the driver's defaults: what the accuracy bounds refer to
BORDER = 24                                      # pixels left out a side by flow_rms
KINDS = ("vortex", "rotation", "uniform")

# |iterate_model after 4000 sweeps - euler_lagrange_direct| measured 1.4e-7 on (24, 20) and 1.1e-7 on (7, 31) (f32 sweeps
# against the f64 solve, fields of about 0.5 px; unchanged at 8000 sweeps): ten times that.
DIRECT_SHAPES, DIRECT_SWEEPS, DIRECT_BOUND = [(24, 20), (7, 31)], 4000, 1.4e-6

# (height, width) of the terms and the sweeps; the small sides exercise the mirror at reach 2 and the clamp
SHAPES = [(1, 1), (1, 9), (9, 1), (3, 4), (37, 53), (130, 97)]

# Bounds.  Ratio of the flow's error to the dense predictor's, per seed (the numpy prototype of the definition gave at most
# 0.36 on vortex and rotation, 0.94 on uniform).
RATIO_BOUND = {"vortex": 0.5, "rotation": 0.5, "uniform": 1.0}
# The device's error per field (px): the worst seed of optical_flow_model (printed by
# test_optical_flow.py::test_flow_improves_on_its_predictor), times 1.2.  The seeds spread by +-9 %, and the device
# differs from the model by the f32 warp and the f32 predictor only, about 1e-6 px.
MODEL_WORST = {"vortex": 0.0580, "rotation": 0.0232, "uniform": 0.0283}
DEVICE_BOUND = {k: 1.2 * v for k, v in MODEL_WORST.items()}


def random_terms(shape, seed: int, alpha2: float = ALPHA2):
    """(terms f32 [h, w, 4], u f32 [h, w, 2]): random finite derivatives and residuals with the weight that belongs to them,
    and a random start."""
    rng = np.random.default_rng(seed)
    h, w = shape
    ix, iy, c = (rng.normal(0.0, s, (h, w)).astype(np.float32) for s in (1.0, 1.0, 0.5))
    wt = np.float32(1) / ((np.float32(alpha2) + ix * ix) + iy * iy)
    return np.stack([ix, iy, c, wt], axis=-1).astype(np.float32), rng.normal(0.0, 2.0, (h, w, 2)).astype(np.float32)


def random_pair(shape, seed: int):
    """(w1, w2, u0) f32: two smooth random images that nearly match, and the field they are said to be warped by."""
    rng = np.random.default_rng(seed)
    h, w = shape
    base = rng.uniform(0.0, 900.0, (h, w))
    return (base.astype(np.float32), (base + rng.normal(0.0, 30.0, (h, w))).astype(np.float32),
            rng.normal(0.0, 1.5, (h, w, 2)).astype(np.float32))


def random_grid_field(shape, win: int, step: int, seed: int, nan_at=(0, 0), cols: int = 2):
    """A vector grid f32 [n_rows, n_cols, cols] of a few pixels with one NaN vector."""
    from photon_amd import piv_correlation as pc
    rng = np.random.default_rng(seed)
    r, c = pc.grid_shape(shape, win, step)
    f = rng.uniform(-3.0, 3.0, (r, c, cols)).astype(np.float32)
    f[min(nan_at[0], r - 1), min(nan_at[1], c - 1), 0] = np.nan
    return f


def pixel_truth(kind: str, shape=dc.SHAPE) -> np.ndarray:
    """The displacement at every pixel, [height, width, 2] (the field refers to the mid-point frame, as the pairs do)."""
    y, x = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    return np.stack(dc.FIELDS[kind](x, y), axis=-1)


def flow_rms(dense, kind: str, border: int = BORDER) -> float:
    """RMS of |u - truth| over the pixels at least `border` from the image's edge."""
    e = (np.asarray(dense, np.float64) - pixel_truth(kind, np.shape(dense)[:2]))[border:-border, border:-border]
    return float(np.sqrt(np.mean((e * e).sum(axis=-1))))


@functools.lru_cache(maxsize=None)
def pair32(kind: str, seed: int):
    """The analytic pair as the device takes it: f32."""
    im1, im2 = dc.pair(kind, seed)
    return im1.astype(np.float32), im2.astype(np.float32)


@functools.lru_cache(maxsize=None)
def model_errors(kind: str, seed: int):
    """(dense predictor error, flow error) px of optical_flow_model from one iteration of correlate_deform_model."""
    im1, im2 = pair32(kind, seed)
    grid = pd.correlate_deform_model(im1, im2, dc.WIN, dc.STEP, iterations=1)[0][..., :2]
    dense = pd.dense_field(grid, im1.shape, dc.WIN, dc.STEP)
    flow = of.optical_flow_model(im1, im2, dense, dc.WIN, dc.STEP, ALPHA2, WARPS, ITERATIONS)
    return flow_rms(dense, kind), flow_rms(flow, kind)


def print_table(title: str, rows):
    """rows: (kind, seed, predictor error, flow error)."""
    print(f"\n{title}\n  field     seed  predictor (px)  flow (px)  ratio")
    for kind, seed, p, f in rows:
        print(f"  {kind:9s} {seed:4d}  {p:14.4f}  {f:9.4f}  {f / p:5.2f}")
