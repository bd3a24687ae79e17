"""Shared cases of the tomographic-PIV tests (test_piv_tomo.py, test_piv_tomo_gpu.py and the two test_zz_piv_tomo_* modules):
the line-of-sight geometry with voxels inside and outside one camera, the volume pairs of the 3-D correlator with their f64
models (computed once, read-only), the exact tie, and the accuracy chain on piv_tomo.CASES."""
import functools

import numpy as np

from photon_amd import piv_tomo as pt
from photon_amd import piv_stereo as ps

# ---- line of sight ---------------------------------------------------------------------------------------------------------------
LOS_VOLUME = pt.centred_volume(24, 20, 5, 1.0)            # nx, ny, nz
LOS_SENSORS = ((40, 48), (48, 40))                         # (height, width), alternating over the cameras
LOS_ANGLES = ((25.0, 0.0), (-25.0, 10.0), (0.0, -20.0), (35.0, 15.0), (-35.0, -15.0), (10.0, 25.0), (-10.0, -25.0), (20.0, -5.0))
LOS_FRAMES = 2
LOS_OFF_CAMERA = 2                                         # the camera whose image of the volume leaves its sensor


@functools.lru_cache(maxsize=None)
def los_cameras(n: int):
    """n fitted cameras on LOS_VOLUME, one pixel per voxel; camera LOS_OFF_CAMERA (when there is one) images the volume's
    centre 14 px off its sensor's centre, so that part of the volume falls off the sensor."""
    mid = pt.slice_plane(LOS_VOLUME, 2)
    target = ps.calibration_target(mid, 7, np.linspace(-3.0, 3.0, 5), margin=0.2)
    out = []
    for c in range(n):
        theta, phi = LOS_ANGLES[c]
        view = ps.pinhole(np.deg2rad(theta), np.deg2rad(phi), 400.0, 1.0, LOS_SENSORS[c % 2], offset=(14.0, -3.0) if c == LOS_OFF_CAMERA else (0.0, 0.0))
        out.append(ps.fit_camera(target, view.project(target))[0])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def los_coefs(n: int):
    """Per camera 'coefficients' f32 [LOS_FRAMES, height, width]: the kernel takes any f32 array for them; these change sign,
    so that the clamp at 0 has work."""
    rng = np.random.default_rng(40 + n)
    return tuple((rng.random((LOS_FRAMES,) + LOS_SENSORS[c % 2]) * 1.25 - 0.25).astype(np.float32) for c in range(n))


@functools.lru_cache(maxsize=None)
def los_want(n: int, mode: str):
    poly, grids = pt.los_coefficients(los_cameras(n), LOS_VOLUME)
    return pt.los_model_f32(los_coefs(n), poly, grids, pt.shape_of(LOS_VOLUME), mode)


# ---- the 3-D correlator ----------------------------------------------------------------------------------------------------------
# name -> (shape (nz, ny, nx), win, step, R, win_z, step_z, Rz, shift (dz, dy, dx), offsets)
CORRELATOR = {
    "w16_r1_z1": ((12, 36, 40), 16, 8, 1, 1, 1, 0, (0.0, 0.3, -0.4), False),           # K = 1; win_z 1 on many slabs
    "w16_r8_z16": ((20, 36, 40), 16, 8, 8, 16, 4, 8, (2.3, -3.4, 1.7), True),          # K > 1; radius_z = win_z / 2; step_z < win_z
    "w16_r4_z16": ((19, 36, 40), 16, 7, 4, 16, 16, 1, (0.4, 1.6, -2.2), False),        # step_z = win_z, nz no multiple
    "w32_r1_z3": ((12, 36, 40), 32, 4, 1, 3, 3, 1, (-0.3, 0.4, 0.2), False),           # step_z = win_z
    "w32_r16_z3": ((12, 36, 40), 32, 4, 16, 3, 2, 0, (0.2, 5.3, -7.6), True),          # radius_z 0 with win_z > 1
    "w64_r1_z3": ((3, 70, 72), 64, 2, 1, 3, 1, 1, (0.3, -0.2, 0.4), True),
    "w64_r32_z1": ((3, 70, 72), 64, 3, 32, 1, 1, 0, (0.0, 11.4, -9.7), True),
}


def blob_volume(shape, shift, seed, per_voxel=0.01, noise=0.02):
    """Two volumes f32 [nz, ny, nx] of Gaussian blobs (e^-2 diameter 2.5 voxels), the second displaced by shift = (dz, dy,
    dx) voxels, with independent noise."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    n = int(per_voxel * (nz + 8) * (ny + 8) * (nx + 8))
    q = rng.uniform((-4, -4, -4), (nx + 4, ny + 4, nz + 4), (n, 3))                     # (x, y, z)
    amp = rng.uniform(0.5, 1.0, n)
    vol = pt.volume(0.0, 0.0, 0.0, 1.0, nx, ny, nz)
    moved = q + np.array([shift[2], shift[1], shift[0]])
    return ((pt.true_volume(vol, q, amp) + noise * rng.random(shape)).astype(np.float32),
            (pt.true_volume(vol, moved, amp) + noise * rng.random(shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def correlator_case(name: str):
    """(vol1, vol2, offsets int32 [n_slabs, n_rows, n_cols, 3] or None, the f64 model (vectors, flags, planes)).  The offsets
    push windows outside in each axis."""
    shape, win, step, R, win_z, step_z, Rz, shift, with_off = CORRELATOR[name]
    v1, v2 = blob_volume(shape, shift, seed=win * 100 + R + win_z)
    off = None
    if with_off:
        grid = pt.grid_shape(shape, win, step, win_z, step_z)
        off = np.random.default_rng(R + win_z).integers(-3, 4, size=grid + (3,)).astype(np.int32)
        off.reshape(-1, 3)[0] = (0, 0, -(Rz + 1))                                       # outside in z
        off.reshape(-1, 3)[-1] = (win // 2, -4, 0)                                      # half outside in x
    want = pt.correlate_volume_model(v1, v2, win, step, R, win_z, step_z, Rz, offset=off, planes=True)
    return v1, v2, off, want


def clear_windows(want):
    """(live, clear): the windows that are not flat, and of those the ones whose two highest plane values differ by more
    than 1e-3 of the peak."""
    flat = (want[1] & 2) != 0
    planes = want[2][~flat].reshape(int((~flat).sum()), -1)
    srt = np.sort(planes, axis=1)
    return ~flat, srt[:, -1] - srt[:, -2] > 1e-3 * srt[:, -1]


# ---- an exact tie ------------------------------------------------------------------------------------------------------------------
TIE = dict(win=16, step=16, R=3, win_z=4, step_z=4, Rz=2, first=(-1, 1, 0), second=(1, -1, 2))       # (sz, sy, sx)


@functools.lru_cache(maxsize=None)
def tie_pair():
    """A window-periodic volume of -1 / 0 / +1 with mean 0 and vol2 = its copies at two shifts added: every sum is a small
    integer, exact in f32 and f64, and C(first) == C(second) == the energy of the window, the largest value of the plane.
    (nz, ny, nx) = (12, 48, 48): three periods each way; only the centre window needs no outside voxel."""
    rng = np.random.default_rng(5)
    n = TIE["win_z"] * TIE["win"] * TIE["win"]
    tile = np.zeros(n, np.float32)
    tile[:256], tile[256:512] = 1.0, -1.0
    tile = rng.permutation(tile).reshape(TIE["win_z"], TIE["win"], TIE["win"])
    v1 = np.tile(tile, (3, 3, 3))
    v2 = np.roll(v1, TIE["first"], (0, 1, 2)) + np.roll(v1, TIE["second"], (0, 1, 2))
    return v1, v2


# ---- the accuracy chain ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_model(name: str, seed: int = 0):
    """(frames, cameras, the model chain's result) of piv_tomo.CASES[name] at `seed`."""
    frames, cameras, vol, _ = pt.case_inputs(name, seed)
    return frames, cameras, pt.correlate_tomo_model(frames, cameras, vol, **pt.CASE_GRID)


# rms error of the model chain per component over the interior nodes, in voxels: the worst of piv_tomo.CASE_SEEDS x 1.25
# (measured by test_piv_tomo.py on the CPU, which prints every seed)
CHAIN_BARS = {"uniform": (0.1157, 0.0841, 0.1539), "shear": (0.1266, 0.0740, 0.1231), "four_cross": (0.1043, 0.0959, 0.1895),
              "three": (0.0986, 0.0882, 0.1815)}
