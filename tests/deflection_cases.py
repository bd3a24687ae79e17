"""Shared cases of the deflection-tomography tests (test_tomo_deflection.py, test_tomo_deflection_gpu.py): the ray sets of
tomography_cases.py with two transverse vectors per ray, and the analytic deflections of the Gaussian blob.  Every case is
built once and shared: nobody writes into what these functions return."""
import functools

import numpy as np

import tomography_cases as tc
from photon_amd import tomography as tm

# the hand-set vectors of "random", on its first rays
ZERO_T1, PARALLEL_T1, NAN_T2 = 0, 1, 2
DELTA = 1.0                     # the shift of the shift-derivative identity, microns


class DeflectionCase:
    """A tomography case with its vectors t1, t2 [n_rays, 3]."""

    def __init__(self, case: tc.Case, t1, t2):
        self.case = case
        self.t1 = np.ascontiguousarray(t1, np.float64)
        self.t2 = np.ascontiguousarray(t2, np.float64)
        for k in ("dims", "spacing", "origin", "origins", "dirs", "n_rays", "shape", "grid"):
            setattr(self, k, getattr(case, k))
        self.rays = (self.origins, self.dirs, self.t1, self.t2)

    @functools.cached_property
    def taps(self) -> tm.Taps:
        return tm.deflection_taps(*self.grid, *self.rays)


@functools.lru_cache(maxsize=None)
def random_case() -> DeflectionCase:
    c = tc.random_case()
    rng = np.random.default_rng(21)
    t1, t2 = rng.normal(size=(c.n_rays, 3)), rng.normal(size=(c.n_rays, 3))
    t1[ZERO_T1] = 0.0
    t1[PARALLEL_T1] = 1.7 * c.dirs[PARALLEL_T1] / np.linalg.norm(c.dirs[PARALLEL_T1])
    t2[NAN_T2, 1] = np.nan
    return DeflectionCase(c, t1, t2)


def view_frames_of(case: tc.Case, k_views: int = tc.K_VIEWS) -> DeflectionCase:
    """t1 = the view's rotated x axis made perpendicular to the ray and normalised, t2 = e x t1."""
    per_view = case.n_rays // k_views
    e = case.dirs / np.linalg.norm(case.dirs, axis=1, keepdims=True)
    x = np.concatenate([np.broadcast_to(tc.rot_y(np.pi * k / k_views) @ np.array([1.0, 0.0, 0.0]), (per_view, 3)) for k in range(k_views)])
    t1 = x - (x * e).sum(axis=1, keepdims=True) * e
    t1 = t1 / np.linalg.norm(t1, axis=1, keepdims=True)
    return DeflectionCase(case, t1, np.cross(e, t1))


@functools.lru_cache(maxsize=None)
def views_case(n: int = 24) -> DeflectionCase:
    return view_frames_of(tc.views_case(n))


@functools.lru_cache(maxsize=None)
def large_case() -> DeflectionCase:
    return view_frames_of(tc.large_case())


@functools.lru_cache(maxsize=None)
def dense_case() -> DeflectionCase:
    return view_frames_of(tc.dense_case())


@functools.lru_cache(maxsize=None)
def coarse_case(n: int) -> DeflectionCase:
    return view_frames_of(tc.coarse_case(n))


# "coarse2" .. "coarse4": runs of up to 64, 52 and 34 adjacent lanes in one voxel (test_tomography.py holds the lengths)
CASES = {"random": random_case, "views": views_case, "large": large_case, "dense": dense_case,
         "coarse2": functools.partial(coarse_case, 2), "coarse3": functools.partial(coarse_case, 3),
         "coarse4": functools.partial(coarse_case, 4)}


@functools.lru_cache(maxsize=None)
def runs_case() -> DeflectionCase:
    """The exact family of tomography_cases.runs_case for section 10: its rays with vectors whose entries are multiples of
    1/4 in [-2, 2], and two whole-number ray vectors y1, y2 that are 0 together in the rays of tc.RUNS_DEAD.  Every weight is
    a multiple of 2^-7, so D^T y is exact in f64 in any order of addition."""
    base = tc.runs_case()
    rng = np.random.default_rng(43)
    t1, t2 = (rng.integers(-8, 9, (base.n_rays, 3)) / 4.0 for _ in range(2))
    c = DeflectionCase(base, t1, t2)
    c.y1, c.y2 = tc.whole_numbers(rng, base.n_rays), tc.whole_numbers(rng, base.n_rays)
    c.y1[list(tc.RUNS_DEAD)] = c.y2[list(tc.RUNS_DEAD)] = 0.0
    c.live = (c.y1 != 0.0) | (c.y2 != 0.0)
    return c


def random_problem(c: DeflectionCase):
    """Random deflections, weights (some 0, one NaN) and an 80 % support for the solver parity tests."""
    rng = np.random.default_rng(9)
    g1, g2 = tm.deflect_model(rng.normal(size=c.shape), c.spacing, c.origin, *c.rays, taps=c.taps)
    scale = max(np.abs(g1).max(), np.abs(g2).max())
    g1 = g1 + 0.05 * rng.normal(size=g1.shape) * scale
    g2 = g2 + 0.05 * rng.normal(size=g2.shape) * scale
    w = rng.uniform(0.2, 2.0, g1.shape)
    w[rng.random(g1.shape) < 0.1] = 0.0
    w[7], g1[11], g2[13] = np.nan, np.inf, np.nan
    support = (rng.random(c.shape) < 0.8).astype(np.uint8)
    return g1, g2, w, support


def blob_deflections(c: DeflectionCase, centre=None):
    """The analytic deflections of the blob along the case's rays: along tau, g = -P (rel_perp . tau) / sigma^2 with rel_perp
    the vector from the blob's centre to the nearest point of the ray."""
    ctr = tc.BLOB["centre"] if centre is None else centre
    e = c.dirs / np.linalg.norm(c.dirs, axis=1, keepdims=True)
    rel = c.origins - ctr
    perp = rel - (rel * e).sum(axis=1, keepdims=True) * e
    P = tc.blob_projection(c.case, centre)
    return tuple(-P * (perp * t).sum(axis=1) / tc.BLOB["sigma"] ** 2 for t in (c.t1, c.t2))


def shifted_origins(c: DeflectionCase, tau, sign: float, delta: float = DELTA) -> np.ndarray:
    return c.origins + (sign * delta) * tau


def same_cells(c: DeflectionCase, tau, delta: float = DELTA) -> np.ndarray:
    """The rays of the shift-derivative identity: those that cross the grid, are no miss of section 10, and whose copies at
    origins +- delta tau count as many planes and tap the same voxels as the ray itself.  Returns (keep, crossing), two
    masks over the rays."""
    base = c.case.taps
    crossing = c.taps.planes > 0
    keep = crossing.copy()
    for sign in (1.0, -1.0):
        with np.errstate(invalid="ignore"):
            t = tm.ray_taps(*c.grid, shifted_origins(c, tau, sign, delta), c.dirs)
        same = keep & (t.planes == base.planes)
        a, b = same[base.ray], same[t.ray]                      # the taps of the rays still in: as many on both sides
        oa, ob = np.lexsort((base.voxel[a], base.ray[a])), np.lexsort((t.voxel[b], t.ray[b]))
        differ = base.voxel[a][oa] != t.voxel[b][ob]
        keep = same & (np.bincount(base.ray[a][oa], differ, minlength=c.n_rays) == 0)
    return keep, crossing
