"""Shared cases of the tomography tests (test_tomography.py, test_tomography_gpu.py): a random ray set with hand-made
edge rays, and K rotated views of an off-centre Gaussian blob with their analytic projections.  Every case is built once
and shared: nobody writes into what these functions return."""
import functools

import numpy as np

from photon_amd import bos_density as bd
from photon_amd import tomography as tm


class Case:
    def __init__(self, dims, spacing, origin, origins, dirs):
        self.dims = tuple(int(n) for n in dims)
        self.spacing = np.asarray(spacing, np.float64)
        self.origin = np.asarray(origin, np.float64)
        self.origins = np.ascontiguousarray(origins, np.float64)
        self.dirs = np.ascontiguousarray(dirs, np.float64)
        self.n_rays = self.origins.shape[0]
        self.shape = self.dims[::-1]                      # [nz, ny, nx]
        self.grid = (self.dims, self.spacing, self.origin)

    @functools.cached_property
    def taps(self):
        return tm.ray_taps(*self.grid, self.origins, self.dirs)

    def nodes(self):
        """World coordinates (x, y, z) of the voxels, each [nz, ny, nx]."""
        ax = [self.origin[a] + np.arange(self.dims[a]) * self.spacing[a] for a in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return x, y, z


# ---- "random" -----------------------------------------------------------------------------------------------------------
N_RANDOM = 600
# the hand-made rays, in this order after the 600 random ones
EDGE_RAYS = ("miss_beside", "miss_diagonal", "grid_line", "upper_face", "corner", "tie_xy", "non_unit", "zero_dir", "nan_origin")


@functools.lru_cache(maxsize=None)
def random_case() -> Case:
    dims, spacing, origin = (13, 9, 11), np.array([700.0, 900.0, 1100.0]), np.array([-4000.0, -3500.0, -5600.0])
    rng = np.random.default_rng(5)
    o = rng.uniform(-9000.0, 9000.0, (N_RANDOM, 3))
    d = rng.uniform(-3000.0, 3000.0, (N_RANDOM, 3)) - o
    hi = origin + (np.array(dims) - 1) * spacing
    x3, y2, z4 = origin[0] + 3 * spacing[0], origin[1] + 2 * spacing[1], origin[2] + 4 * spacing[2]
    extra = {
        "miss_beside": ((20000.0, 0.0, -9000.0), (0.0, 0.0, 1.0)),               # parallel to z, beside the box
        "miss_diagonal": ((-9000.0, 9000.0, 9000.0), (1.0, 1.0, 0.2)),           # leaves before it reaches the box
        "grid_line": ((x3, y2, -9000.0), (0.0, 0.0, 1.0)),                       # along the grid line i = 3, j = 2
        "upper_face": ((-9000.0, hi[1], z4 + 100.0), (1.0, 0.0, 0.01)),          # lies in the face j = ny - 1 (u = n_b - 1)
        "corner": (tuple(origin - 3.0 * (hi - origin)), tuple(hi - origin)),     # the body diagonal: through two corners
        "tie_xy": ((-6000.0, -5000.0, 100.0), (1.0, 1.0, 0.0)),                  # |d_x| = |d_y|: the dominant axis is x
        "non_unit": ((-9000.0, 300.0, -200.0), (3.0e4, 1.0e3, 2.0e3)),
        "zero_dir": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
        "nan_origin": ((np.nan, 0.0, 0.0), (1.0, 0.0, 0.0)),
    }
    o = np.concatenate([o, np.array([extra[k][0] for k in EDGE_RAYS])])
    d = np.concatenate([d, np.array([extra[k][1] for k in EDGE_RAYS])])
    return Case(dims, spacing, origin, o, d)


def edge_ray(name: str) -> int:
    return N_RANDOM + EDGE_RAYS.index(name)


def random_field(case: Case, seed: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).normal(size=case.shape)


def random_problem(case: Case):
    """Random projections, weights (some 0, one NaN) and an 80 % support for the solver parity tests."""
    rng = np.random.default_rng(9)
    p = tm.project_model(rng.normal(size=case.shape), case.spacing, case.origin, case.origins, case.dirs, taps=case.taps)
    p = p + 0.05 * rng.normal(size=p.shape) * np.abs(p).max()
    w = rng.uniform(0.2, 2.0, p.shape)
    w[rng.random(p.shape) < 0.1] = 0.0
    w[7], p[11] = np.nan, np.inf
    support = (rng.random(case.shape) < 0.8).astype(np.uint8)
    return p, w, support


# ---- "views" and "large": K rotated views of an off-centre Gaussian blob ------------------------------------------------------
EXTENT, HALF = 24000.0, 12000.0
BLOB = dict(centre=np.array([1500.0, -1000.0, 800.0]), sigma=2500.0, amplitude=2.0)
K_VIEWS = 8
TARGET_Z, AIM = 40000.0, np.array([0.0, 0.0, -400000.0])


def rot_y(angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def view_case(n: int, n_side: int, k_views: int = K_VIEWS) -> Case:
    """Grid n^3 over EXTENT centred on 0; k_views views of n_side^2 rays: target points at +-0.98 HALF on the plane z =
    TARGET_Z aiming at AIM, view k rotated by R_y(pi k / k_views) about the origin."""
    t = np.linspace(-0.98 * HALF, 0.98 * HALF, n_side)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    o0 = np.stack([xx, yy, np.full(xx.shape, TARGET_Z)], axis=-1).reshape(-1, 3)
    d0 = AIM - o0
    o, d = [], []
    for k in range(k_views):
        R = rot_y(np.pi * k / k_views)
        o.append(o0 @ R.T)
        d.append(d0 @ R.T)
    h = EXTENT / (n - 1)
    return Case((n, n, n), (h, h, h), (-HALF, -HALF, -HALF), np.concatenate(o), np.concatenate(d))


@functools.lru_cache(maxsize=None)
def views_case(n: int = 24) -> Case:
    return view_case(n, 24)


@functools.lru_cache(maxsize=None)
def large_case() -> Case:
    return view_case(64, 64)


@functools.lru_cache(maxsize=None)
def dense_case() -> Case:
    """Rays four times as dense as the grid (16^3, 8 x 64^2 rays): neighbouring rays of a view's row meet in one voxel, which
    is what the device's adjoint merges before it adds (longest_lane_run)."""
    return view_case(16, 64)


@functools.lru_cache(maxsize=None)
def coarse_case(n: int) -> Case:
    """The dense rays on a grid of n^3, n = 2, 3, 4: up to a whole wave of adjacent lanes in one voxel, with the weights of
    ordinary rotated views."""
    return view_case(n, 64)


# ---- "runs": exact arithmetic, every lane layout of the adjoint's merge --------------------------------------------------------
# Rays parallel to a grid axis on a grid whose spacings and origin are powers of two or small integers, through points at
# quarter fractions of a cell: every weight is a multiple of 2^-5 (section 10: 2^-7) below 8, y holds whole numbers, and so
# every product and every partial sum of A^T y is exact in f64 -- the result has the same bits in any order of addition.
RUNS_GRID = ((8, 8, 4), (2.0, 4.0, 0.5), (-8.0, 16.0, 1.0))
RUNS_Z, RUNS_X, RUNS_X_BACK = (0.0, 0.0, 3.0), (5.0, 0.0, 0.0), (-5.0, 0.0, 0.0)      # directions of exact length
RUNS_OUTSIDE = -3                                           # a cell index beside the grid: the ray misses
# (direction, cell, lanes) in ray order; cell = the indices of the ray's cell along the two in-plane axes (x, y for a ray
# along z; y, z for one along x).  Ray r is lane r % 64 of wave r // 64.
RUNS_LAYOUT = (
    # wave 0: one cell, a run of 64
    (RUNS_Z, (3, 2), 64),
    # wave 1: runs of 1 .. 8, 12 and 16
    (RUNS_Z, (0, 0), 1), (RUNS_Z, (1, 3), 2), (RUNS_Z, (2, 6), 3), (RUNS_Z, (3, 2), 4), (RUNS_Z, (4, 5), 5), (RUNS_Z, (5, 1), 6),
    (RUNS_Z, (6, 4), 7), (RUNS_Z, (0, 5), 8), (RUNS_Z, (1, 1), 12), (RUNS_Z, (2, 4), 16),
    # wave 2: two cells in turn, A B A B ...: equal voxels that are never adjacent
    *(((RUNS_Z, (1, 1), 1), (RUNS_Z, (4, 3), 1)) * 32),
    # wave 3: 40 lanes of one cell with lanes 5, 17, 18 beside the grid (and y = 0 in lanes 9 and 30: RUNS_DEAD), then the
    # first half of a run of 48 that the wave boundary cuts into 24 + 24
    (RUNS_Z, (5, 4), 5), (RUNS_Z, (RUNS_OUTSIDE, 4), 1), (RUNS_Z, (5, 4), 11), (RUNS_Z, (RUNS_OUTSIDE, 4), 2), (RUNS_Z, (5, 4), 21),
    (RUNS_Z, (0, 6), 24),
    # wave 4: its second half, then runs of 33 and 7
    (RUNS_Z, (0, 6), 24), (RUNS_Z, (6, 0), 33), (RUNS_Z, (2, 5), 7),
    # wave 5: rays along x, runs of 40, 14 and 10 through all 8 planes
    (RUNS_X, (3, 1), 40), (RUNS_X, (6, 2), 14), (RUNS_X, (0, 0), 10),
    # wave 6: rays along z and along x in one wave: it walks max(nx, nz) = 8 planes, the z lanes only the first 4
    (RUNS_Z, (4, 4), 20), (RUNS_X_BACK, (2, 0), 26), (RUNS_Z, (4, 4), 18),
    # wave 7: 17 lanes, the other 47 have no ray
    (RUNS_Z, (6, 6), 17),
)
RUNS_DEAD = (3 * 64 + 9, 3 * 64 + 30)                       # rays whose y is 0: the device takes them for dead lanes
RUNS_N = 465


class RunsCase(Case):
    """A Case with the whole-number ray vector y of the exact family, and which of its rays the device's adjoint walks."""

    def __init__(self, *args, y):
        super().__init__(*args)
        self.y = np.ascontiguousarray(y, np.float64)
        self.live = self.y != 0.0


def whole_numbers(rng, size, top: int = 8) -> np.ndarray:
    """Whole numbers in [-top, top] without 0, as f64."""
    v = rng.integers(1, top + 1, size).astype(np.float64)
    return np.where(rng.random(size) < 0.5, -v, v)


@functools.lru_cache(maxsize=None)
def runs_case() -> RunsCase:
    dims, spacing, origin = RUNS_GRID
    quarter = (0.0, 0.25, 0.5, 0.75)
    o, d = [], []
    for direction, cell, lanes in RUNS_LAYOUT:
        a = int(np.flatnonzero(direction)[0])
        b, c = [k for k in range(3) if k != a]
        for _ in range(lanes):
            r = len(o)                                          # the fractions turn with the ray: the lanes of a run differ
            p = [0.0, 0.0, 0.0]
            p[a] = origin[a] - 4.0 * spacing[a] if direction[a] > 0 else origin[a] + (dims[a] + 3.0) * spacing[a]
            p[b] = origin[b] + (cell[0] + quarter[r % 4]) * spacing[b]
            p[c] = origin[c] + (cell[1] + quarter[(r // 4 + r // 16) % 4]) * spacing[c]
            o.append(p)
            d.append(direction)
    y = whole_numbers(np.random.default_rng(41), len(o))
    y[list(RUNS_DEAD)] = 0.0
    return RunsCase(dims, spacing, origin, o, d, y=y)


def exact_adjoint(taps, ys):
    """sum over the taps of weight * y per voxel in rational arithmetic (one Fraction per voxel), and whether every sum of
    the model is safe from rounding in any order: all products are multiples of one power of two 2^-q, and the sum of their
    magnitudes per voxel stays below 2^(53 - q).  Returns (list of Fraction, bool)."""
    from fractions import Fraction
    total = [Fraction(0)] * taps.n_voxels
    size = [Fraction(0)] * taps.n_voxels
    q = 0
    for i in range(taps.ray.size):
        parts = [Fraction(float(w[i])) * Fraction(float(y[taps.ray[i]])) for w, y in zip(taps.weights, ys)]     # a float is dyadic
        q = max([q] + [p.denominator.bit_length() - 1 for p in parts])
        total[taps.voxel[i]] += sum(parts)
        size[taps.voxel[i]] += sum(abs(p) for p in parts)
    return total, max(size) * 2 ** q < 2 ** 53


def lane_runs(case, live=None, wave: int = 64):
    """Every run of adjacent lanes that add to one voxel in one step of the device's adjoint, as (wave, first lane, length),
    three arrays: ray r is lane r % wave of wave r // wave, and a step is one tap (0 .. 3) of one plane kappa.  A lane whose
    plane does not count breaks a run, and so does a ray that is not `live` (a mask over the rays: the device skips a ray
    whose y are all 0)."""
    t = case.taps
    with np.errstate(invalid="ignore"):
        e = case.dirs / np.linalg.norm(case.dirs, axis=1, keepdims=True)
        axis = np.argmax(np.abs(np.nan_to_num(e)), axis=1)        # the first axis to attain the maximum
    stride = np.array([1, case.dims[0], case.dims[0] * case.dims[1]])
    extent = np.array(case.dims)
    a = axis[t.ray]
    kappa = (t.voxel // stride[a]) % extent[a]
    tap = np.arange(t.ray.size) % 4
    keep = np.ones(t.ray.size, bool) if live is None else np.asarray(live, bool)[t.ray]
    ray, kappa, tap, voxel = t.ray[keep], kappa[keep], tap[keep], t.voxel[keep]
    if ray.size == 0:
        return (np.zeros(0, np.int64),) * 3
    order = np.lexsort((ray % wave, tap, kappa, ray // wave))
    key = np.stack([ray // wave, kappa, tap, voxel], axis=1)[order]
    lane = (ray % wave)[order]
    joined = (key[1:] == key[:-1]).all(axis=1) & (lane[1:] == lane[:-1] + 1)
    first = np.concatenate([[True], ~joined])
    return key[first, 0], lane[first], np.bincount(np.cumsum(first) - 1)


def lane_run_histogram(case, live=None, wave: int = 64) -> np.ndarray:
    """np.bincount of the lengths of lane_runs: entry n counts the runs of exactly n lanes."""
    return np.bincount(lane_runs(case, live, wave)[2])


def longest_lane_run(case, wave: int = 64) -> int:
    """The longest run of adjacent lanes that add to one voxel in one step of the device's adjoint (lane_runs)."""
    return max(len(lane_run_histogram(case, wave=wave)) - 1, 1)


def blob_field(case: Case, centre=None) -> np.ndarray:
    x, y, z = case.nodes()
    c = BLOB["centre"] if centre is None else centre
    return BLOB["amplitude"] * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * BLOB["sigma"] ** 2))


def blob_projection(case: Case, centre=None) -> np.ndarray:
    """The analytic line integrals of the blob along the case's rays."""
    c = BLOB["centre"] if centre is None else centre
    return bd.gaussian_projection(tm.line_distance_sq(case.origins, case.dirs, c), BLOB["amplitude"], BLOB["sigma"])


def sphere_support(case: Case, radius: float = 11000.0) -> np.ndarray:
    x, y, z = case.nodes()
    return ((x * x + y * y + z * z) <= radius * radius).astype(np.uint8)


def ray_weights(n_rays: int) -> np.ndarray:
    """Random weights in [0.2, 2) with 10 % of them 0, for the solver tests on the views of a blob."""
    rng = np.random.default_rng(9)
    w = rng.uniform(0.2, 2.0, n_rays)
    w[rng.random(n_rays) < 0.1] = 0.0
    return w


def rel_l2(a, b) -> float:
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))
