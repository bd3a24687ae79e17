"""What the self-calibration tests share (tests/test_piv_stereo_selfcal.py on the CPU, tests/test_piv_stereo_selfcal_gpu.py and
tests/test_zz_piv_stereo_selfcal_perf_gpu.py on the device): piv_stereo.SELFCAL_CASE's frames, the model's self-calibration of
them and the model chain's figures before and after (each computed once), and the disparity fields the triangulation runs on.
Everything is cached and read-only."""
import functools

import numpy as np

import piv_stereo_cases as base
from photon_amd import piv_stereo as ps

CASE = ps.SELFCAL_CASE
PLANE, SHEET = CASE["plane"], CASE["sheet"]
DISPARITY, EVALUATION = CASE["disparity"], CASE["evaluation"]
frozen = base.frozen


@functools.lru_cache(maxsize=None)
def inputs():
    """(views, frames, pair, aligned) of piv_stereo.selfcal_inputs, the stacks read-only."""
    views, frames, pair, aligned = ps.selfcal_inputs()
    return views, tuple(frozen(f) for f in frames), tuple(frozen(f) for f in pair), tuple(frozen(f) for f in aligned)


def cameras():
    return tuple(v[1] for v in inputs()[0])


def pinholes():
    return tuple(v[0] for v in inputs()[0])


@functools.lru_cache(maxsize=None)
def true_frame():
    return ps.sheet_frame(SHEET, PLANE)


@functools.lru_cache(maxsize=None)
def model_result():
    """(cameras, report) of self_calibrate_model on the case's frames."""
    frames = inputs()[1]
    return ps.self_calibrate_model(frames[0], frames[1], cameras(), PLANE, **DISPARITY)


def camera_errors(cams):
    """Per camera, the largest distance in pixels on calibration_target(plane, 9, (-0.5, 0, 0.5)) between `cams` and the true
    pinholes seen through the true sheet frame."""
    target = ps.calibration_target(PLANE, 9, (-0.5, 0.0, 0.5))
    world = ps.to_world(true_frame(), target)
    return [float(np.linalg.norm(ps.map_points(cam, target) - view.project(world), axis=-1).max()) for cam, view in zip(cams, pinholes())]


def report_frame(report):
    return report["R"], report["O"], report["C"]


@functools.lru_cache(maxsize=None)
def model_evaluation():
    """The model chain's (rms dX dY dZ, median residual) on the case's pair with the original cameras, with the model's
    corrected cameras, and on the same flow rendered on the aligned sheet with the original cameras."""
    _, _, pair, aligned = inputs()
    corrected, report = model_result()
    run = lambda f, cams: ps.correlate_stereo_model(f[0], f[1], cams, PLANE, **EVALUATION)[0]     # noqa: E731
    return (ps.selfcal_figures(run(pair, cameras())), ps.selfcal_figures(run(pair, corrected), report_frame(report)),
            ps.selfcal_figures(run(aligned, cameras())))


# ---- the triangulation ---------------------------------------------------------------------------------------------------------
WIN, STEP = base.WIN, base.STEP
GRIDS = {"1x1": (32, 32), "5x7": (96, 128), "9x29": (160, 480)}        # plane (height, width) at win 32, step 16; 261 nodes: two blocks


def grid_plane(grid):
    h, w = GRIDS[grid]
    return ps.centred_plane(w, h, 0.2)


def disparity_inputs(grid, seed=17):
    """A random disparity field f32 [r, c, 4] within +- 6 px and flags on the grid `grid` of GRIDS, with a NaN dx, an infinite
    dy and section 5's flag bits sprinkled in (not on the 1 x 1 grid's only node): (plane, field, flags)."""
    pl = grid_plane(grid)
    h, w = GRIDS[grid]
    r, c = (h - WIN) // STEP + 1, (w - WIN) // STEP + 1
    rng = np.random.default_rng(seed)
    field = rng.uniform(-6.0, 6.0, (r, c, 4)).astype(np.float32)
    flags = rng.choice([0, 0, 0, 1, 4, 8], (r, c)).astype(np.int32)
    if r * c > 1:
        field[0, 1, 0], flags[0, 1] = np.nan, 2
        field[r - 1, c - 1, 1] = np.inf
    return pl, frozen(field), frozen(flags)


def plane_image(cam, W, z):
    """The points of the plane Z = z that the camera sees where it sees the world points W [..., 3] (Newton on X, Y)."""
    want = ps.map_points(cam, W)
    p = np.array(W, np.float64)
    p[..., 2] = z
    for _ in range(12):
        J = ps.jacobian(cam, p)[..., :, :2]
        p[..., :2] += np.linalg.solve(J, (want - ps.map_points(cam, p))[..., None])[..., 0]
    return p


def surface_disparity(cams, pl, surface, win=WIN, step=STEP):
    """Per node of the plane's grid, the world point of Z = surface(X, Y) whose two images on the plane have the node's centre
    as their midpoint, and the disparity in dewarped pixels (f64) between those images: (points [r, c, 3], disparity [r, c, 2])."""
    P = ps.window_centres(pl, win, step)
    W = P.copy()
    for _ in range(40):
        W[..., 2] = surface(W[..., 0], W[..., 1])
        p1, p2 = (plane_image(cam, W, pl["z"]) for cam in cams)
        W[..., :2] += P[..., :2] - 0.5 * (p1[..., :2] + p2[..., :2])
    W[..., 2] = surface(W[..., 0], W[..., 1])
    p1, p2 = (plane_image(cam, W, pl["z"]) for cam in cams)
    assert np.abs(0.5 * (p1 + p2) - P)[..., :2].max() < 1e-12
    return W, (p2 - p1)[..., :2] / pl["pitch"]
