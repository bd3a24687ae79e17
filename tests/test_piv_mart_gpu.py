"""MART particle volumes on the device (include/parallel_ray_tracing.h, section 21): photon_piv_volume_mart bit for bit against
piv_mart.mart_model_f32, photon_piv_volume_project integer for integer against piv_mart.project_model, contention on a 3 x 3
pixel patch and the cap, dirty workspaces, gaps and masks, the refusals, and the drivers against the model chains.  The
held-back-stream cases: tests/test_zz_piv_mart_streams_gpu.py; the timing: tests/test_zz_piv_mart_perf_gpu.py."""
import ctypes

import numpy as np
import pytest

import piv_mart_cases as cases
from photon_amd import library
from photon_amd import piv_correlation as pc
from photon_amd import piv_mart as pm
from photon_amd import piv_tomo as pt

pytestmark = pytest.mark.gpu

GAP, FILL = 7, 777.0
SHAPE = pt.shape_of(cases.VOLUME)
NVOX = SHAPE[0] * SHAPE[1] * SHAPE[2]
MAX_PIXELS = max(h * w for h, w in cases.SENSORS)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def padded(stack, gap=GAP):
    """[n, ...] as f32 [n + 1, size + gap] with FILL in the gaps and in the row beyond."""
    n = stack.shape[0]
    flat = stack.reshape(n, -1)
    host = np.full((n + 1, flat.shape[1] + gap), FILL, np.float32)
    host[:n, :flat.shape[1]] = flat
    return host


def run_mart(photon, n_frames, mu_roots, threshold, iterations, with_mask=True, garbage="ff", stream=0):
    """One photon_piv_volume_mart on the case's volumes, every stride GAP above its size and the workspace dirty.  Returns
    the volumes f32 [n_frames, nz, ny, nx] after checking that gaps, the row beyond, the frames, the mask and the words behind
    the workspace are as they were."""
    import torch
    poly, grids, _ = cases.geometry()
    vol_host = padded(cases.volumes(n_frames))
    d_vol = dev(vol_host)
    srcs = [dev(padded(f)) for f in cases.frames(n_frames)]
    d_mask = dev(cases.mask()) if with_mask else None
    words = 2 * n_frames * MAX_PIXELS
    if garbage == "ff":
        d_acc = torch.full((words + GAP,), -1, dtype=torch.int64, device="cuda")        # 0xFF in every byte
    else:
        d_acc = dev(np.random.default_rng(5).integers(-2 ** 62, 2 ** 62, words + GAP))
    tail = d_acc[words:].clone()
    d_poly = dev(poly)
    photon.piv_volume_mart([s.data_ptr() for s in srcs], [h * w + GAP for h, w in cases.SENSORS], n_frames, cases.SENSORS, grids, d_poly.data_ptr(),
                           cases.VOLUME, NVOX + GAP, d_vol.data_ptr(), d_acc.data_ptr(), iterations, mu_roots, threshold, cases.scale(n_frames),
                           d_mask.data_ptr() if with_mask else 0, stream)
    torch.cuda.synchronize()
    got = d_vol.cpu().numpy()
    assert (got[:, NVOX:] == FILL).all() and (got[n_frames] == FILL).all()              # the gaps, the volume beyond
    for s, f in zip(srcs, cases.frames(n_frames)):
        assert s.cpu().numpy().tobytes() == padded(f).tobytes()                         # the frames are not written
    assert torch.equal(d_acc[words:], tail) and (not with_mask or np.array_equal(d_mask.cpu().numpy(), cases.mask()))
    return got[:n_frames, :NVOX].reshape((n_frames,) + SHAPE)


# ---- photon_piv_volume_mart --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames, mu_roots, threshold, iterations", cases.PARITY)
def test_mart_returns_the_f32_models_bits(photon, n_frames, mu_roots, threshold, iterations):
    want = cases.mart_want(n_frames, mu_roots, threshold, iterations)
    got = run_mart(photon, n_frames, mu_roots, threshold, iterations)
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert got.tobytes() == want.tobytes(), f"{differ.sum()} voxels differ, the first at {np.argwhere(differ)[:3].tolist()}"
    start = cases.volumes(n_frames)
    live = start > 0
    assert (got[live] > 0).any() and (got[live] == 0).any() and got[~live].tobytes() == start[~live].tobytes()
    assert (got[:, cases.mask() == 1][live[:, cases.mask() == 1]] == 0).all()           # masked voxels stay 0
    again = run_mart(photon, n_frames, mu_roots, threshold, iterations, garbage="random")
    assert again.tobytes() == got.tobytes()                                             # two calls, another dirt in the workspace: the same bits


def test_the_cases_cover_what_the_kernel_branches_on():
    assert {p[0] for p in cases.PARITY} == {1, 2, 5} and {p[1] for p in cases.PARITY} == {0, 1, 2, 3}
    assert {p[2] > 0 for p in cases.PARITY} == {False, True} and {p[3] for p in cases.PARITY} == {1, 3}
    assert SHAPE[2] % 64 and SHAPE[2] > 64 and SHAPE[1] % 4 and len(set(cases.SENSORS)) == 3
    seen = cases.geometry()[2]
    assert seen[0].all() and seen[2].all() and 0 < seen[cases.OFF_CAMERA].sum() < seen[cases.OFF_CAMERA].size


def test_mart_without_a_mask(photon):
    want = cases.mart_want(2, 1, 0.0, 3, with_mask=False)
    got = run_mart(photon, 2, 1, 0.0, 3, with_mask=False)
    assert got.tobytes() == want.tobytes() and want.tobytes() != cases.mart_want(2, 1, 0.0, 3).tobytes()


# ---- photon_piv_volume_project -----------------------------------------------------------------------------------------------------
def run_project(photon, volumes, poly, grids, sensors, scale_log2, images=True, gap=GAP):
    """One photon_piv_volume_project into dirty accumulators and images, strides `gap` above the sensors' sizes: (accumulators
    int64 [n, height, width] per camera, images f32 likewise or None) after checking the gaps and the volume."""
    import torch
    n = volumes.shape[0]
    vol_host = padded(volumes)
    d_vol, d_poly = dev(vol_host), dev(poly)
    strides = [h * w + gap for h, w in sensors]
    d_acc = [torch.full((n + 1, s), -1, dtype=torch.int64, device="cuda") for s in strides]
    d_img = [torch.full((n + 1, s), FILL, dtype=torch.float32, device="cuda") for s in strides]
    photon.piv_volume_project(d_vol.data_ptr(), volumes[0].size + GAP, n, sensors, grids, d_poly.data_ptr(), cases.VOLUME, [a.data_ptr() for a in d_acc],
                              strides, scale_log2, [i.data_ptr() for i in d_img] if images else None)
    torch.cuda.synchronize()
    assert d_vol.cpu().numpy().tobytes() == vol_host.tobytes()
    accs, imgs = [], []
    for (h, w), a, i in zip(sensors, d_acc, d_img):
        a, i = a.cpu().numpy(), i.cpu().numpy()
        assert (a[n] == -1).all() and (a[:, h * w:] == -1).all() and (i[n] == FILL).all() and (i[:, h * w:] == FILL).all()
        assert images or (i == FILL).all()
        accs.append(a[:n, :h * w].reshape(n, h, w))
        imgs.append(i[:n, :h * w].reshape(n, h, w))
    return accs, (imgs if images else None)


@pytest.mark.parametrize("n_frames", cases.FRAME_COUNTS)
def test_project_returns_the_models_integers_and_images(photon, n_frames):
    poly, grids, _ = cases.geometry()
    want_acc, want_img = cases.project_want(n_frames)
    acc, img = run_project(photon, cases.volumes(n_frames), poly, grids, cases.SENSORS, cases.PROJECT_SCALE)
    for c in range(3):
        assert np.array_equal(acc[c], want_acc[c]) and img[c].tobytes() == want_img[c].tobytes() and want_acc[c].sum() > 0, c
    again, none = run_project(photon, cases.volumes(n_frames), poly, grids, cases.SENSORS, cases.PROJECT_SCALE, images=False, gap=0)
    assert none is None and all(np.array_equal(a, b) for a, b in zip(again, acc))       # two calls; contiguous accumulators: one memset


def test_project_under_contention_and_at_the_cap(photon):
    """Every voxel of the volume on a 3 x 3 pixel patch, two cameras: 3150 voxels x 4 taps on 9 words each, exact; the same
    with voxels of 1e30 and infinity: every tap with a weight adds 2^31, a zero weight under an infinite voxel nothing."""
    poly, grids = cases.patch_geometry()
    for volumes, s in ((np.where(cases.volumes(2) > 0, cases.volumes(2), np.float32(0)), 30), (cases.capped_volume()[None], 20)):
        want = pm.project_model(volumes, poly, grids, cases.PATCH_SENSORS, s)
        acc, img = run_project(photon, volumes, poly, grids, cases.PATCH_SENSORS, s)
        for c in range(2):
            assert np.array_equal(acc[c], want[c]) and img[c].tobytes() == pm.images_of(want[c], s).tobytes() and want[c].min() > 2 ** 30
    assert want[0].max() > 2 ** 38


# ---- the refusals ------------------------------------------------------------------------------------------------------------------
def _fill_cameras(job, grids):
    for c, (h, w) in enumerate(cases.SENSORS):
        job.height[c], job.width[c] = h, w
        for m in range(4):
            job.grid[c][m] = grids[c][m]
    job.volume = library.photon_piv_volume_t(cases.VOLUME["x0"], cases.VOLUME["y0"], cases.VOLUME["z0"], 1.0, SHAPE[2], SHAPE[1], SHAPE[0])


def mart_job(keep):
    """A valid job on the case's three cameras and two frames; `keep` receives the device tensors it points to."""
    import torch
    poly, grids, _ = cases.geometry()
    keep["src"] = [dev(f) for f in cases.frames(2)]
    keep["poly"], keep["vol"], keep["mask"] = dev(poly), dev(cases.volumes(2)), dev(cases.mask())
    keep["acc"] = torch.full((2, 2, MAX_PIXELS), 7, dtype=torch.int64, device="cuda")
    job = library.photon_piv_volume_mart_t(n_cameras=3, n_frames=2, iterations=2, mu_roots=1, scale_log2=cases.scale(2), threshold=0.0,
                                           d_poly=keep["poly"].data_ptr(), vol_stride=NVOX, d_vol=keep["vol"].data_ptr(),
                                           d_mask=keep["mask"].data_ptr(), d_acc=keep["acc"].data_ptr(), stream=None)
    _fill_cameras(job, grids)
    for c, (h, w) in enumerate(cases.SENSORS):
        job.d_frame[c], job.frame_stride[c] = keep["src"][c].data_ptr(), h * w
    return job


def project_job(keep):
    import torch
    poly, grids, _ = cases.geometry()
    keep["poly"], keep["vol"] = dev(poly), dev(cases.volumes(2))
    keep["acc"] = [torch.full((2, h, w), 7, dtype=torch.int64, device="cuda") for h, w in cases.SENSORS]
    keep["img"] = [torch.full((2, h, w), 7.0, dtype=torch.float32, device="cuda") for h, w in cases.SENSORS]
    job = library.photon_piv_volume_project_t(n_cameras=3, n_frames=2, scale_log2=cases.PROJECT_SCALE, d_poly=keep["poly"].data_ptr(),
                                              d_vol=keep["vol"].data_ptr(), vol_stride=NVOX, stream=None)
    _fill_cameras(job, grids)
    for c, (h, w) in enumerate(cases.SENSORS):
        job.d_acc[c], job.acc_stride[c], job.d_image[c] = keep["acc"][c].data_ptr(), h * w, keep["img"][c].data_ptr()
    return job


def _set(name, value, index=None):
    def change(job):
        if index is None:
            setattr(job, name, value)
        else:
            getattr(job, name)[index] = value
    return change


def _volume(name, value):
    return lambda job: setattr(job.volume, name, value)


def _huge(job):
    job.volume.nx, job.volume.ny, job.volume.nz = 1 << 11, 1 << 11, 1 << 10


COMMON_REFUSALS = {
    "null_poly": _set("d_poly", None), "null_vol": _set("d_vol", None), "one_camera": _set("n_cameras", 1), "nine_cameras": _set("n_cameras", 9),
    "no_frames": _set("n_frames", 0), "scale_below": _set("scale_log2", -127), "scale_above": _set("scale_log2", 63), "nx_0": _volume("nx", 0),
    "nz_negative": _volume("nz", -2), "ny_above_the_side_limit": _volume("ny", (1 << 22) + 1), "volume_above_int_max": _huge,
    "width_0": _set("width", 0, 2), "height_above_the_side_limit": _set("height", (1 << 22) + 1, 0), "vol_stride_short": _set("vol_stride", NVOX - 1),
    "grid_not_finite": lambda job: job.grid[1].__setitem__(2, float("inf")),
}
MART_REFUSALS = dict(COMMON_REFUSALS, **{
    "null_acc": _set("d_acc", None), "null_frame": _set("d_frame", None, 1), "frame_stride_short": _set("frame_stride", 31 * 40 - 1, 0),
    "no_iterations": _set("iterations", 0), "roots_negative": _set("mu_roots", -1), "roots_4": _set("mu_roots", 4),
    "threshold_negative": _set("threshold", -1.0), "threshold_nan": _set("threshold", float("nan")), "threshold_inf": _set("threshold", float("inf")),
    "vol_is_a_frame": lambda job: setattr(job, "d_vol", job.d_frame[2]),
    "acc_inside_the_volume": lambda job: setattr(job, "d_acc", job.d_vol + 4 * 100),
    "acc_is_a_frame": lambda job: setattr(job, "d_acc", job.d_frame[0]),
    "mask_inside_the_workspace": lambda job: setattr(job, "d_mask", job.d_acc + 8 * 10),
})
PROJECT_REFUSALS = dict(COMMON_REFUSALS, **{
    "null_acc": _set("d_acc", None, 1), "acc_stride_short": _set("acc_stride", 37 * 33 - 1, 1),
    "two_cameras_one_accumulator": lambda job: job.d_acc.__setitem__(2, job.d_acc[0]),
    "acc_inside_the_volume": lambda job: job.d_acc.__setitem__(0, job.d_vol + 4 * 64),
    "image_inside_an_accumulator": lambda job: job.d_image.__setitem__(1, job.d_acc[2] + 8),
})


def _snapshot(keep):
    out = []
    for v in keep.values():
        out += [t.clone() for t in (v if isinstance(v, list) else [v])]
    return out


def _refused(photon, capfd, symbol, job, keep, what):
    import torch
    before = _snapshot(keep)
    capfd.readouterr()
    rc = getattr(photon.lib, symbol)(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and len(err.strip().splitlines()) == 1 and symbol in err, (what, err)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, _snapshot(keep))), what


@pytest.mark.parametrize("what", list(MART_REFUSALS))
def test_mart_refusals_print_one_line_and_write_nothing(photon, capfd, what):
    keep = {}
    job = mart_job(keep)
    MART_REFUSALS[what](job)
    _refused(photon, capfd, "photon_piv_volume_mart", job, keep, what)


@pytest.mark.parametrize("what", list(PROJECT_REFUSALS))
def test_project_refusals_print_one_line_and_write_nothing(photon, capfd, what):
    keep = {}
    job = project_job(keep)
    PROJECT_REFUSALS[what](job)
    _refused(photon, capfd, "photon_piv_volume_project", job, keep, what)


def test_null_jobs_are_refused_and_the_valid_jobs_run(photon, capfd):
    import torch
    capfd.readouterr()
    for symbol in ("photon_piv_volume_mart", "photon_piv_volume_project"):
        assert getattr(photon.lib, symbol)(None) == 1 and len(capfd.readouterr().err.strip().splitlines()) == 1
    keep = {}
    assert photon.lib.photon_piv_volume_mart(ctypes.byref(mart_job(keep))) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == "" and keep["vol"].cpu().numpy().tobytes() == cases.mart_want(2, 1, 0.0, 2).tobytes()
    keep = {}
    assert photon.lib.photon_piv_volume_project(ctypes.byref(project_job(keep))) == 0
    torch.cuda.synchronize()
    want_acc, want_img = cases.project_want(2)
    assert capfd.readouterr().err == ""
    for c in range(3):
        assert np.array_equal(keep["acc"][c].cpu().numpy(), want_acc[c]) and keep["img"][c].cpu().numpy().tobytes() == want_img[c].tobytes()


# ---- the drivers -------------------------------------------------------------------------------------------------------------------
def test_reconstruct_volume_with_mart_against_the_models(photon):
    """The driver's chain: the B-spline coefficients on the device, one line-of-sight launch in mode "min", then MART on the
    frames themselves -- mart_model_f32 of los_model_f32, bit for bit."""
    import test_piv_stereo_gpu as stereo
    rng = np.random.default_rng(8)
    frames = [rng.random((2,) + s).astype(np.float32) for s in cases.SENSORS]
    cams, vol = cases.cameras(), cases.VOLUME
    got, mask = photon.reconstruct_volume(frames, cams, vol, method="mart", iterations=3, relaxation=0.25)
    assert got.is_cuda and tuple(got.shape) == (2,) + SHAPE
    got, mask = got.cpu().numpy(), mask.cpu().numpy()
    poly, grids = pt.los_coefficients(cams, vol)
    coefs = [stereo.device_coefficients(photon, f)[1] for f in frames]
    first, mask32 = pt.los_model_f32(coefs, poly, grids, SHAPE, "min")
    s, thr = pm.scale_log2_for(frames), pm.default_threshold(frames)
    want = pm.mart_model_f32(frames, first, poly, grids, 3, 2, thr, s, mask32)
    assert got.tobytes() == want.tobytes() and np.array_equal(mask, mask32) and 0 < mask.sum() < mask.size
    assert (want > 0).any() and want.tobytes() != first.tobytes()
    los, _ = photon.reconstruct_volume(frames, cams, vol)                              # the defaults: line of sight, as before
    assert los.cpu().numpy().tobytes() == first.tobytes()
    explicit, _ = photon.reconstruct_volume([f[0] for f in frames], cams, vol, method="mart", iterations=3, relaxation=0.25, threshold=thr, scale_log2=s)
    assert tuple(explicit.shape) == SHAPE and explicit.cpu().numpy().tobytes() == got[0].tobytes()
    for bad in (dict(method="smart"), dict(relaxation=0.3), dict(iterations=0), dict(threshold=-1.0), dict(scale_log2=99), dict(mode="product")):
        with pytest.raises(ValueError):
            photon.reconstruct_volume(frames, cams, vol, **{**dict(method="mart"), **bad})


def test_reproject_against_the_model(photon):
    poly, grids, _ = cases.geometry()
    volumes = cases.volumes(2)
    images, acc = photon.reproject(volumes, cases.cameras(), cases.VOLUME, cases.SENSORS, scale_log2=cases.PROJECT_SCALE)
    want_acc, want_img = cases.project_want(2)
    for c in range(3):
        assert np.array_equal(acc[c].cpu().numpy(), want_acc[c]) and images[c].cpu().numpy().tobytes() == want_img[c].tobytes()
    one, _ = photon.reproject(np.where(volumes[0] > 0, volumes[0], 0), cases.cameras(), cases.VOLUME, cases.SENSORS)     # the driver's own scale
    s = pm.scale_log2_for([np.where(volumes[0] > 0, volumes[0], 0)]) + 2
    assert tuple(one[0].shape) == cases.SENSORS[0]
    assert one[0].cpu().numpy().tobytes() == pm.images_of(pm.project_model(volumes[0], poly, grids, cases.SENSORS, s)[0], s).tobytes()
    with pytest.raises(ValueError):
        photon.reproject(volumes[:, :2], cases.cameras(), cases.VOLUME, cases.SENSORS)


@pytest.mark.parametrize("name", list(pm.CASES))
def test_correlate_tomo_with_mart_against_the_model_chain(photon, name):
    """The device chain with reconstruction="mart" on seed 0 of piv_mart.CASES: per component the rms error over the interior
    nodes within the CPU bars and within the f64 model chain's own figure on the same frames x 1.25."""
    m = cases.chain_model(name)
    m_d, m_vec, m_flags, m_partial = m["result"]
    d, vec, flags, partial = photon.correlate_tomo(list(m["frames"]), m["cameras"], pt.CASE_VOLUME, reconstruction="mart", iterations=cases.ITERATIONS,
                                                   relaxation=cases.RELAXATION, **pt.CASE_GRID)
    rms, n = pm.case_figures(name, d)
    print(f"{name}: device rms dX dY dZ {rms.round(4)} voxels (model {m['rms'].round(4)}) over {n} interior nodes")
    assert d.shape == m_d.shape and d.dtype == np.float64 and vec.shape == m_vec.shape and np.array_equal(partial, m_partial)
    assert n >= 12 and not (flags[pt.interior(flags.shape)] & ~pc.FLAG_OUTSIDE).any()
    assert (rms <= 1.25 * m["rms"]).all() and (rms <= np.array(cases.CHAIN_BARS[name])).all()
