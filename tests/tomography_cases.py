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


def longest_lane_run(case: Case, wave: int = 64) -> int:
    """The longest run of adjacent lanes that add to one voxel in one step of the device's adjoint: ray r is lane r % wave of
    wave r // wave, and a step is one tap (0 .. 3) of one plane kappa.  A lane whose plane does not count breaks a run."""
    t = case.taps
    with np.errstate(invalid="ignore"):
        e = case.dirs / np.linalg.norm(case.dirs, axis=1, keepdims=True)
        axis = np.argmax(np.abs(np.nan_to_num(e)), axis=1)        # the first axis to attain the maximum
    stride = np.array([1, case.dims[0], case.dims[0] * case.dims[1]])
    extent = np.array(case.dims)
    a = axis[t.ray]
    kappa = (t.voxel // stride[a]) % extent[a]
    tap = np.arange(t.ray.size) % 4
    order = np.lexsort((t.ray % wave, tap, kappa, t.ray // wave))
    key = np.stack([t.ray // wave, kappa, tap, t.voxel], axis=1)[order]
    lane = (t.ray % wave)[order]
    joined = (key[1:] == key[:-1]).all(axis=1) & (lane[1:] == lane[:-1] + 1)
    # lengths of the stretches of True in `joined`, plus one
    edges = np.flatnonzero(np.diff(np.concatenate([[0], joined.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max()) + 1 if edges.size else 1


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


def rel_l2(a, b) -> float:
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))
