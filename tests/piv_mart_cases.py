"""Shared cases of the MART tests (test_piv_mart.py, test_piv_mart_gpu.py and the two test_zz_piv_mart_* modules): the small
geometry with voxels inside and outside one camera, its volumes, frames and f32 models (computed once, read-only), the
camera whose image of the whole volume is a 3 x 3 pixel patch, and the accuracy chain on piv_mart.CASES."""
import functools

import numpy as np

from photon_amd import piv_mart as pm
from photon_amd import piv_stereo as ps
from photon_amd import piv_tomo as pt

# ---- the small geometry ------------------------------------------------------------------------------------------------------------
VOLUME = pt.centred_volume(70, 9, 5, 1.0)                 # nx no multiple of 64, ny no multiple of 4: two blocks in x, three in y
SENSORS = ((31, 40), (37, 33), (29, 48))                   # (height, width): every camera its own
ANGLES = ((25.0, 0.0), (-25.0, 10.0), (0.0, -20.0))
OFF_CAMERA = 1                                             # the camera whose image of the volume leaves its sensor
FRAME_COUNTS = (1, 2, 5)                                   # five frames cross the kernel's four-frame chunk
# (n_frames, mu_roots, threshold, iterations): every value of each at least once with two values of the others
PARITY = ((1, 0, 0.0, 1), (2, 1, 0.05, 3), (5, 2, 0.0, 3), (5, 3, 0.05, 1), (2, 3, 0.0, 1), (1, 2, 0.05, 3), (2, 0, 0.05, 1), (5, 1, 0.0, 1),
          (1, 1, 0.05, 1), (2, 2, 0.0, 3))


def readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cameras():
    """Three fitted cameras on VOLUME at half a pixel per voxel; camera OFF_CAMERA images the volume's centre 9 px off its
    sensor's centre, so that part of the volume falls off the sensor."""
    mid = pt.slice_plane(VOLUME, 2)
    target = ps.calibration_target(mid, 7, np.linspace(-3.0, 3.0, 5), margin=0.2)
    out = []
    for c, (theta, phi) in enumerate(ANGLES):
        view = ps.pinhole(np.deg2rad(theta), np.deg2rad(phi), 400.0, 0.5, SENSORS[c], offset=(9.0, -2.0) if c == OFF_CAMERA else (0.0, 0.0))
        out.append(ps.fit_camera(target, view.project(target))[0])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def geometry():
    """(poly f64 [3, nz, 2, 10], grids f64 [3, 4], seen bool [3, nz, ny, nx])."""
    poly, grids = pt.los_coefficients(cameras(), VOLUME)
    seen = np.stack([pm.volume_footprint(poly[c], grids[c], pt.shape_of(VOLUME), SENSORS[c])[0] for c in range(3)])
    return readonly(poly), readonly(grids), readonly(seen)


@functools.lru_cache(maxsize=None)
def volumes(n_frames: int):
    """Sparse volumes f32 [n_frames, nz, ny, nx]: 45 % of the voxels above 0, a few negative and a few NaN (they add nothing
    and stay as they are)."""
    rng = np.random.default_rng(70 + n_frames)
    shape = (n_frames,) + pt.shape_of(VOLUME)
    v = np.where(rng.random(shape) < 0.45, rng.random(shape) + 0.01, 0.0).astype(np.float32)
    v[rng.random(shape) < 0.01] = -0.5
    v[rng.random(shape) < 0.01] = np.nan
    return readonly(v)


@functools.lru_cache(maxsize=None)
def frames(n_frames: int):
    """Per camera frames f32 [n_frames, height, width] that change sign (the clamp at 0 has work) with a few exact zeros."""
    rng = np.random.default_rng(80 + n_frames)
    out = []
    for s in SENSORS:
        f = (rng.random((n_frames,) + s) * 1.25 - 0.25).astype(np.float32)
        f[rng.random(f.shape) < 0.02] = 0.0
        out.append(readonly(f))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mask():
    """u8 [nz, ny, nx]: 1 where a camera does not see the voxel (what section 20a writes) and on a few voxels more."""
    m = (~geometry()[2].all(axis=0)).astype(np.uint8)
    m[np.random.default_rng(9).random(m.shape) < 0.03] = 1
    return readonly(m)


def scale(n_frames: int) -> int:
    return pm.scale_log2_for(list(frames(n_frames)))


@functools.lru_cache(maxsize=None)
def mart_want(n_frames: int, mu_roots: int, threshold: float, iterations: int, with_mask: bool = True):
    poly, grids, _ = geometry()
    return readonly(pm.mart_model_f32(frames(n_frames), volumes(n_frames), poly, grids, iterations, mu_roots, threshold, scale(n_frames),
                                      mask() if with_mask else None))


PROJECT_SCALE = 20


@functools.lru_cache(maxsize=None)
def project_want(n_frames: int):
    """(accumulators int64 [n_frames, height, width] per camera, images f32 likewise)."""
    poly, grids, _ = geometry()
    acc = pm.project_model(volumes(n_frames), poly, grids, SENSORS, PROJECT_SCALE)
    return tuple(readonly(a) for a in acc), tuple(readonly(pm.images_of(a, PROJECT_SCALE)) for a in acc)


# ---- contention: the whole volume on a 3 x 3 pixel patch ---------------------------------------------------------------------------
PATCH_SENSORS = ((3, 3), (3, 3))


@functools.lru_cache(maxsize=None)
def patch_geometry():
    """Two cameras written down as polynomials (grid = voxel indices): x = 1.99 j / (nx - 1), y = 1.99 i / (ny - 1) + 0.002 k,
    the second one mirrored in x: every voxel lands inside a 3 x 3 sensor."""
    nz, ny, nx = pt.shape_of(VOLUME)
    poly, grids = np.zeros((2, nz, 2, 10)), np.tile(np.array([0.0, 1.0, 0.0, 1.0]), (2, 1))
    for k in range(nz):
        poly[0, k, 0, 1], poly[0, k, 1, 2], poly[0, k, 1, 0] = 1.99 / (nx - 1), 1.99 / (ny - 1), 0.002 * k
        poly[1, k, 0, 0], poly[1, k, 0, 1], poly[1, k, 1, 2] = 1.995, -1.99 / (nx - 1), 1.99 / (ny - 1)
    return readonly(poly), readonly(grids)


@functools.lru_cache(maxsize=None)
def capped_volume():
    """One volume f32 whose live voxels are huge (1e30) or infinite: every tap with a weight above 0 adds the cap 2^31, a zero
    weight adds nothing (0 x inf is a NaN: nothing)."""
    v = volumes(1)[0].copy()
    live = v > 0
    v[live] = np.float32(1e30)
    v[live & (np.random.default_rng(3).random(v.shape) < 0.3)] = np.inf
    return readonly(v)


# ---- the accuracy chain ------------------------------------------------------------------------------------------------------------
ITERATIONS, RELAXATION = 5, 0.5


@functools.lru_cache(maxsize=None)
def chain_model(name: str, seed: int = 0):
    """Of piv_mart.CASES[name] at `seed`, in f64: dict(frames, cameras, truth = the true particle field of the first exposure,
    first = the line-of-sight volumes, volumes = after ITERATIONS of MART, mask, q_los and q_mart = (whole volume, interior) of
    the first exposure, result = mart_tomo_model's, rms = its error per component in voxels, nodes)."""
    frames_, cams, vol, (P, brightness, half) = pm.case_inputs(name, seed)
    truth = pt.true_volume(vol, P - half, brightness)
    E, first, unseen = pm.reconstruct_model(frames_, cams, vol, ITERATIONS, RELAXATION)
    result = pm.mart_tomo_model(frames_, cams, vol, **pt.CASE_GRID, volumes=(E, first, unseen))
    rms, nodes = pm.case_figures(name, result[0])
    return dict(frames=frames_, cameras=cams, truth=truth, first=first, volumes=E, mask=unseen, result=result, rms=rms, nodes=nodes,
                q_los=(pt.quality(first[0], truth), pm.interior_quality(first[0], truth)),
                q_mart=(pt.quality(E[0], truth), pm.interior_quality(E[0], truth)))


# rms error of the MART model chain per component over the interior nodes, in voxels: the worst of piv_tomo.CASE_SEEDS x 1.25
# (measured by test_piv_mart.py on the CPU, which prints every seed)
CHAIN_BARS = {"uniform": (0.0797, 0.0785, 0.1258), "shear": (0.0872, 0.0669, 0.1267), "four_cross": (0.0920, 0.0782, 0.1054),
              "three": (0.0845, 0.0837, 0.1990), "uniform_inside": (0.0580, 0.0630, 0.1124)}
# mart_model_f32 against mart_model after 5 iterations from the same first guess, largest difference over max E: the worst
# seed of every case, 4.13e-7 (three, seed 0), x 2
F32_BAR = 8.3e-7
