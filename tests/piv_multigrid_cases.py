"""Case builders shared by tests/test_piv_multigrid.py (CPU tier) and tests/test_piv_multigrid_gpu.py: the grid changes of
the regrid step with their random fields, and the particle pair whose shift no 16-pixel window can find and whose
gradients no 32-pixel window resolves.  Every pair and every model result is computed once per process; the model results
are handed out read-only."""
import functools

import numpy as np

import piv_deformation_cases as dc
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_multigrid as pm

# ---- the regrid step -----------------------------------------------------------------------------------------------------
M = 20.0                                    # |v| <= M pixels
BOUND = 16.0 * 2.0 ** -24 * M               # three f32 roundings per lerp, two stages, differences up to 2 M
GRID_CHANGES = [((64, 32), (32, 16)), ((32, 16), (16, 8)), ((64, 32), (16, 8)), ((16, 8), (32, 16)), ((32, 16), (32, 8)), ((16, 5), (32, 7))]
SHAPES = [(64, 64), (97, 130), (130, 97), (200, 136)]
REGRID_CASES = [(shape, src, dst) for shape in SHAPES for src, dst in GRID_CHANGES]
# a 1 x n and an n x 1 source grid (and their destinations: several rows from one)
THIN_CASES = [((64, 200), (64, 32), (16, 8)), ((200, 64), (64, 32), (32, 16)), ((70, 150), (64, 20), (16, 5))]


def case_id(case):
    (h, w), (sw, ss), (dw, ds) = case
    return f"{h}x{w}_{sw}-{ss}_to_{dw}-{ds}"


def random_field(shape, src, seed, stride=2, bad=0.0):
    """f32 [n_rows, n_cols, stride] on the grid `src` of an image of `shape`: vectors with |v| <= M; stride 4: the other two
    floats are poison (NaN and a huge number, never to be read); bad: the share of nodes with a NaN or an inf component."""
    rng = np.random.default_rng(seed)
    r, c = pc.grid_shape(shape, *src)
    f = np.empty((r, c, stride), np.float32)
    v = rng.uniform(-M, M, (r, c, 2))
    f[..., :2] = v * np.minimum(1.0, M / np.maximum(np.hypot(v[..., 0], v[..., 1]), 1e-9))[..., None]
    if stride == 4:
        f[..., 2], f[..., 3] = np.nan, 3.0e38
    if bad > 0.0:
        hit = rng.random((r, c)) < bad
        hit.flat[0] = True
        f[hit, rng.integers(0, 2, int(hit.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(hit.sum()))
    return f


def centres(shape, grid):
    """(rows [n_rows], cols [n_cols]) of the window centres of `grid` = (win, step), f64."""
    win, step = grid
    r, c = pc.grid_shape(shape, win, step)
    return (win - 1) / 2.0 + step * np.arange(r, dtype=np.float64), (win - 1) / 2.0 + step * np.arange(c, dtype=np.float64)


# ---- the pair ------------------------------------------------------------------------------------------------------------
SHAPE = (192, 192)
SEEDS = (1, 2, 3)
METHODS = ("direct", "phase")
SCHEDULE, ITERATIONS = ((64, 32), (32, 16), (16, 8)), (1, 1, 2)
FINAL = SCHEDULE[-1]
UNIFORM = (13.3, -9.4)
RADIUS = {"direct": 24, "phase": None}              # of pass 0 at win 64
BASE_RADIUS = {"direct": 16, "phase": None}         # of the baseline correlate_deform(32, 16, iterations=3)


def displacement(x, y):
    """vortex(peak 7 px, core 24 px, about the image's centre) + a uniform shift beyond any 16-pixel window's radius."""
    vx, vy = dc.vortex(x, y, peak=7.0, core=24.0, centre=(95.5, 95.5))
    return vx + UNIFORM[0], vy + UNIFORM[1]


@functools.lru_cache(maxsize=None)
def pair(seed: int):
    """(im1, im2) f32, shared by every test of a process (nobody writes to them): piv_deformation_cases.pair's particles under
    `displacement`."""
    rng = np.random.default_rng(seed)
    h, w = SHAPE
    m = 24
    n = int(dc.PER_PIXEL * (h + 2 * m) * (w + 2 * m))
    x, y = rng.uniform(-m, w + m, n), rng.uniform(-m, h + m, n)
    amp = rng.uniform(0.5, 1.0, n)
    dx, dy = displacement(x, y)
    return tuple(pc.particle_image(SHAPE, x + s * dx / 2, y + s * dy / 2, dc.DIAMETER, amp).astype(np.float32) for s in (-1.0, 1.0))


def interior_rms(vectors, grid):
    """RMS of |measured - truth| over the interior nodes of `grid` = (win, step) (the outer ring left out, as in
    piv_deformation_cases.interior_rms)."""
    rows, cols = pc.window_centres(SHAPE, *grid)
    truth = np.stack(displacement(cols, rows), axis=-1)
    e = np.asarray(vectors, np.float64)[1:-1, 1:-1, :2] - truth[1:-1, 1:-1]
    return float(np.sqrt(np.mean((e * e).sum(axis=-1))))


def replaced_share(status):
    return float(((np.asarray(status) & pd.FLAG_REPLACED) != 0).mean())


def _frozen(result):
    for a in result:
        a.setflags(write=False)
    return result


@functools.lru_cache(maxsize=None)
def model_multigrid(seed: int, method: str):
    """(vectors, status) of correlate_multigrid_model on pair(seed) with the default schedule."""
    return _frozen(pm.correlate_multigrid_model(*pair(seed), SCHEDULE, ITERATIONS, radius=RADIUS[method], method=method))


@functools.lru_cache(maxsize=None)
def model_baseline(seed: int, method: str):
    """(vectors, status) of what the library had before: correlate_deform_model(32, 16, iterations=3) on pair(seed)."""
    return _frozen(pd.correlate_deform_model(*pair(seed), 32, 16, BASE_RADIUS[method], iterations=3, method=method))
