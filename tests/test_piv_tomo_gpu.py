"""Tomographic PIV on the device (include/parallel_ray_tracing.h, section 20): photon_piv_volume_los bit for bit against
piv_tomo.los_model_f32 and against photon_piv_dewarp combined by torch, photon_piv_correlate_volume against section 5's bits
on one slice and against the f64 model under section 5's bars, the refusals, and the drivers against the model chain.  The
held-back-stream cases: tests/test_zz_piv_tomo_streams_gpu.py; the timings: tests/test_zz_piv_tomo_perf_gpu.py."""
import ctypes

import numpy as np
import pytest

import piv_tomo_cases as cases
import test_piv_correlation_gpu as base5
from photon_amd import library
from photon_amd import piv_correlation as pc
from photon_amd import piv_tomo as pt

pytestmark = pytest.mark.gpu

POISON, MASK_POISON, GAP = np.float32("nan"), 0xFF, 7


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


# ---- line of sight ---------------------------------------------------------------------------------------------------------------
def run_los(photon, n, mode, n_frames=cases.LOS_FRAMES, with_mask=True, stream=0):
    """One photon_piv_volume_los of the case's first n cameras into NaN-filled volumes and a 0xFF-filled mask, both strides
    GAP floats above the frame size.  Returns (buffer f32 [n_frames + 1, out_stride], mask u8 [nz, ny, nx] or None, the
    sources as uploaded)."""
    import torch
    coefs = cases.los_coefs(n)
    poly, grids = pt.los_coefficients(cases.los_cameras(n), cases.LOS_VOLUME)
    nz, ny, nx = pt.shape_of(cases.LOS_VOLUME)
    srcs, strides = [], []
    for c in coefs:
        f, h, w = c.shape
        host = np.full((f, h * w + GAP), 777.0, np.float32)
        host[:, :h * w] = c.reshape(f, -1)
        srcs.append(dev(host))
        strides.append(h * w + GAP)
    out_stride = nz * ny * nx + GAP
    d_out = torch.full((n_frames + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
    d_mask = torch.full((nz, ny, nx), MASK_POISON, dtype=torch.uint8, device="cuda")
    d_poly = dev(poly)
    photon.piv_volume_los([s.data_ptr() for s in srcs], strides, n_frames, [c.shape[1:] for c in coefs], grids, d_poly.data_ptr(), cases.LOS_VOLUME,
                          out_stride, d_out.data_ptr(), d_mask.data_ptr() if with_mask else 0, pt.MODES[mode], stream)
    torch.cuda.synchronize()
    for s, c in zip(srcs, coefs):
        got = s.cpu().numpy()
        assert np.array_equal(got[:, :-GAP].reshape(c.shape), c) and (got[:, -GAP:] == 777.0).all()      # the sources are not written
    return d_out.cpu().numpy(), (d_mask.cpu().numpy() if with_mask else None)


@pytest.mark.parametrize("mode", ["min", "product"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_los_returns_the_f32_models_bits(photon, n, mode):
    nz, ny, nx = pt.shape_of(cases.LOS_VOLUME)
    want, want_mask = cases.los_want(n, mode)
    buf, mask = run_los(photon, n, mode)
    got = buf[:cases.LOS_FRAMES, :nz * ny * nx].reshape(want.shape)
    assert got.tobytes() == want.tobytes(), f"{(got != want).sum()} voxels differ, largest {np.nanmax(np.abs(got - want)):.3e}"
    assert np.array_equal(mask, want_mask) and (got[:, mask == 1] == 0).all()
    assert np.isnan(buf[cases.LOS_FRAMES:]).all() and np.isnan(buf[:, nz * ny * nx:]).all()      # the frame beyond, the stride gaps
    if n >= 3:
        assert (mask == 1).sum() > 0 and (mask == 0).sum() > 0
    again, mask2 = run_los(photon, n, mode)
    assert again.tobytes() == buf.tobytes() and mask2.tobytes() == mask.tobytes()                # two calls, the same bytes
    no_mask, none = run_los(photon, n, mode, with_mask=False)
    assert none is None and no_mask.tobytes() == buf.tobytes()
    one, _ = run_los(photon, n, mode, n_frames=1)
    assert one[0].tobytes() == buf[0].tobytes() and np.isnan(one[1]).all()


@pytest.mark.parametrize("mode", ["min", "product"])
def test_los_is_the_dewarps_of_every_slice_combined_by_torch(photon, mode):
    """N nz calls of photon_piv_dewarp, clamped at 0 and combined by torch in camera order."""
    import torch
    n = 3
    nz, ny, nx = pt.shape_of(cases.LOS_VOLUME)
    poly, grids = pt.los_coefficients(cases.los_cameras(n), cases.LOS_VOLUME)
    buf, mask = run_los(photon, n, mode)
    got = buf[:cases.LOS_FRAMES, :nz * ny * nx].reshape(cases.LOS_FRAMES, nz, ny, nx)
    srcs = [dev(c) for c in cases.los_coefs(n)]
    for k in range(nz):
        acc, unseen = None, torch.zeros((ny, nx), dtype=torch.bool, device="cuda")
        for c, src in enumerate(srcs):
            f, h, w = src.shape
            d = torch.empty((f, ny, nx), dtype=torch.float32, device="cuda")
            m = torch.empty((ny, nx), dtype=torch.uint8, device="cuda")
            photon.piv_dewarp(src.data_ptr(), h * w, f, w, h, poly[c][k], grids[c], nx, ny, ny * nx, d.data_ptr(), m.data_ptr())
            v = torch.clamp(d, min=0.0)
            acc = v if acc is None else (torch.minimum(acc, v) if mode == "min" else acc * v)
            unseen |= m != 0
        want = torch.where(unseen, torch.zeros((), device="cuda"), acc).cpu().numpy()
        assert got[:, k].tobytes() == want.tobytes() and np.array_equal(mask[k] != 0, unseen.cpu().numpy()), k


def los_job(keep):
    """A valid job on the case's three cameras; `keep` receives the device tensors it points to."""
    import torch
    n = 3
    coefs = cases.los_coefs(n)
    poly, grids = pt.los_coefficients(cases.los_cameras(n), cases.LOS_VOLUME)
    nz, ny, nx = pt.shape_of(cases.LOS_VOLUME)
    keep["src"] = [dev(c) for c in coefs]
    keep["poly"] = dev(poly)
    keep["out"] = torch.full((cases.LOS_FRAMES, nz, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    keep["mask"] = torch.full((nz, ny, nx), 7, dtype=torch.uint8, device="cuda")
    job = library.photon_piv_volume_los_t(n_cameras=n, n_frames=cases.LOS_FRAMES, mode=0, d_poly=keep["poly"].data_ptr(), out_stride=nz * ny * nx,
                                          d_out=keep["out"].data_ptr(), d_mask=keep["mask"].data_ptr(), stream=None)
    job.volume = library.photon_piv_volume_t(-11.5, -9.5, -2.0, 1.0, nx, ny, nz)
    for c in range(n):
        job.d_coef[c], job.frame_stride[c] = keep["src"][c].data_ptr(), coefs[c].shape[1] * coefs[c].shape[2]
        job.height[c], job.width[c] = coefs[c].shape[1:]
        for m in range(4):
            job.grid[c][m] = grids[c][m]
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


def _grid_nan(job):
    job.grid[1][2] = float("inf")


LOS_REFUSALS = {
    "null_poly": _set("d_poly", None), "null_out": _set("d_out", None), "null_coef": _set("d_coef", None, 1),
    "one_camera": _set("n_cameras", 1), "nine_cameras": _set("n_cameras", 9), "mode_2": _set("mode", 2), "mode_negative": _set("mode", -1),
    "no_frames": _set("n_frames", 0), "nx_0": _volume("nx", 0), "nz_negative": _volume("nz", -2), "ny_above_the_side_limit": _volume("ny", (1 << 22) + 1),
    "volume_above_int_max": lambda job: (setattr(job.volume, "nx", 1 << 11), setattr(job.volume, "ny", 1 << 11), setattr(job.volume, "nz", 1 << 10)),
    "width_0": _set("width", 0, 2), "height_above_the_side_limit": _set("height", (1 << 22) + 1, 0),
    "frame_stride_short": _set("frame_stride", 40 * 48 - 1, 0), "out_stride_short": _set("out_stride", 24 * 20 * 5 - 1),
    "out_is_a_source": lambda job: setattr(job, "d_out", job.d_coef[1]),
    "out_inside_a_source": lambda job: setattr(job, "d_out", job.d_coef[2] + 4 * 100),
    "grid_not_finite": _grid_nan,
}


@pytest.mark.parametrize("what", list(LOS_REFUSALS))
def test_los_refusals_print_one_line_and_write_nothing(photon, capfd, what):
    import torch
    keep = {}
    job = los_job(keep)
    LOS_REFUSALS[what](job)
    before = [s.clone() for s in keep["src"]]
    capfd.readouterr()
    rc = photon.lib.photon_piv_volume_los(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and len(err.strip().splitlines()) == 1 and "photon_piv_volume_los" in err, (what, err)
    assert (keep["out"] == 7.0).all().item() and (keep["mask"] == 7).all().item()
    assert all(torch.equal(a, b) for a, b in zip(before, keep["src"]))


def test_los_refuses_a_null_job_and_runs_the_valid_one(photon, capfd):
    import torch
    capfd.readouterr()
    assert photon.lib.photon_piv_volume_los(None) == 1 and len(capfd.readouterr().err.strip().splitlines()) == 1
    keep = {}
    assert photon.lib.photon_piv_volume_los(ctypes.byref(los_job(keep))) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == "" and keep["out"].cpu().numpy().tobytes() == cases.los_want(3, "min")[0].tobytes()


# ---- the 3-D correlator ----------------------------------------------------------------------------------------------------------
def device_correlate_volume(photon, v1, v2, win, step, R, win_z, step_z, Rz, offset=None, stream=0):
    """photon_piv_correlate_volume through the raw job into NaN-filled outputs: (vectors, flags, planes) as numpy."""
    import torch
    a, b = dev(v1), dev(v2)
    off = dev(np.ascontiguousarray(offset, np.int32)) if offset is not None else None
    nz, ny, nx = v1.shape
    slabs, rows, cols = pt.grid_shape(v1.shape, win, step, win_z, step_z)
    nS, nSz = 2 * R + 1, 2 * Rz + 1
    vec = torch.full((slabs, rows, cols, 5), float("nan"), dtype=torch.float32, device="cuda")
    flg = torch.full((slabs, rows, cols), -1, dtype=torch.int32, device="cuda")
    pln = torch.full((slabs, rows, cols, nSz, nS, nS), float("nan"), dtype=torch.float32, device="cuda")
    job = library.photon_piv_correlate_volume_t(d_vol1=a.data_ptr(), d_vol2=b.data_ptr(), nx=nx, ny=ny, nz=nz, win=win, step=step, radius=R,
                                                win_z=win_z, step_z=step_z, radius_z=Rz, d_offset=off.data_ptr() if off is not None else None,
                                                d_vectors=vec.data_ptr(), d_flags=flg.data_ptr(), d_planes=pln.data_ptr(),
                                                stream=int(stream) or None)
    assert photon.lib.photon_piv_correlate_volume(ctypes.byref(job)) == 0
    torch.cuda.synchronize()
    return vec.cpu().numpy(), flg.cpu().numpy(), pln.cpu().numpy()


@pytest.mark.parametrize("case", base5.CASES, ids=[f"w{c[0]}_r{c[1]}_s{c[2]}_{c[3][0]}x{c[3][1]}{'_off' if c[5] else ''}" for c in base5.CASES])
def test_one_slice_returns_section_5s_bits(photon, case):
    """win_z = 1, step_z = 1, radius_z = 0 on a volume of one slice: photon_piv_correlate's dx, dy, peak, ratio, flags and
    plane bit for bit, on section 5's ten shapes; the third component of an offset is not read."""
    win, R, step, shape, shift, with_off = case
    im1, im2 = base5.particle_pair(shape, shift, seed=win * 100 + R + step)
    grid = pc.grid_shape(shape, win, step)
    off = off3 = None
    if with_off:
        off = np.random.default_rng(R).integers(-3, 4, size=grid + (2,)).astype(np.int32)
        off3 = np.concatenate([off, np.full(grid + (1,), 5, np.int32)], axis=-1)
    want_v, want_f, want_p = base5.device_correlate(photon, im1, im2, win, step, R, off)
    vec, flg, pln = device_correlate_volume(photon, im1[None], im2[None], win, step, R, 1, 1, 0, off3)
    assert vec[0][..., [0, 1, 3, 4]].tobytes() == want_v.tobytes() and flg[0].tobytes() == want_f.tobytes()
    assert pln[0][:, :, 0].tobytes() == want_p.tobytes()
    live = (want_f & pc.FLAG_FLAT) == 0
    assert (vec[0][live][:, 2] == 0).all() and np.isnan(vec[0][~live][:, 2]).all()


@pytest.mark.parametrize("name", list(cases.CORRELATOR))
def test_the_volume_correlator_matches_the_host_model(photon, name):
    """Section 5's bars: flags identical, flat windows all NaN, planes within 1e-4 of the plane's peak; where the model's two
    highest values differ by more than 1e-3 of the peak (at most 10 % of the windows may not), the same integer peak, the
    three components within 1e-3, peak and 1 / ratio within 1e-4.  Two calls return the same bytes."""
    shape, win, step, R, win_z, step_z, Rz, shift, with_off = cases.CORRELATOR[name]
    v1, v2, off, want = cases.correlator_case(name)
    got = device_correlate_volume(photon, v1, v2, win, step, R, win_z, step_z, Rz, off)
    (got_v, got_f, got_p), (want_v, want_f, want_p) = got, want
    assert got_v.shape == want_v.shape and got_p.shape == want_p.shape
    assert np.array_equal(got_f, want_f), np.argwhere(got_f != want_f)[:5]
    flat = (want_f & pc.FLAG_FLAT) != 0
    assert np.isnan(got_v[flat]).all() and np.isnan(got_p[flat]).all()
    ok = ~flat
    n = int(ok.sum())
    pw, pg = want_p[ok].reshape(n, -1), got_p[ok].reshape(n, -1)
    peak = pw.max(axis=1)
    worst = (np.abs(pg - pw).max(axis=1) / peak).max()
    live, clear = cases.clear_windows(want)
    print(f"{name}: {n} live windows, planes within {worst:.2e} of the peak, {int((~clear).sum())} without a clear peak")
    assert worst <= 1e-4 and (~clear).sum() <= 0.1 * n
    assert np.array_equal(np.argmax(pg[clear], axis=1), np.argmax(pw[clear], axis=1))
    dv = np.abs(got_v[ok][clear, :3] - want_v[ok][clear, :3])
    assert dv.max() <= 1e-3, dv.max()
    np.testing.assert_allclose(got_v[ok][clear, 3], want_v[ok][clear, 3], rtol=1e-4)
    assert np.abs(1.0 / got_v[ok][clear, 4].astype(np.float64) - 1.0 / want_v[ok][clear, 4]).max() <= 1e-4
    again = device_correlate_volume(photon, v1, v2, win, step, R, win_z, step_z, Rz, off)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


def test_a_tie_goes_to_the_first_shift_on_the_device(photon):
    """Small integers: every sum is exact in f32, the two shifts tie exactly, and the peak is the first in (sz, sy, sx) order."""
    t = cases.TIE
    v1, v2 = cases.tie_pair()
    args = (t["win"], t["step"], t["R"], t["win_z"], t["step_z"], t["Rz"])
    want = pt.correlate_volume_model(v1, v2, *args, planes=True)
    vec, flg, pln = device_correlate_volume(photon, v1, v2, *args)
    assert np.array_equal(flg, want[1]) and flg[1, 1, 1] == 0
    plane = pln[1, 1, 1]
    assert (plane == plane.max()).sum() == 2 and np.array_equal(np.argwhere(plane == plane.max()), np.argwhere(want[2][1, 1, 1] == want[2][1, 1, 1].max()))
    assert tuple(np.rint(vec[1, 1, 1, [2, 1, 0]]).astype(int)) == t["first"]
    assert np.abs(vec[1, 1, 1] - want[0][1, 1, 1]).max() <= 1e-6


def test_flat_windows_and_the_energy_below_f32(photon):
    """A constant window of vol1, a constant zero-shift window of vol2, and a contrast too small for the f32 energies: flag
    2, every output of the window NaN, the other windows untouched by it."""
    v1, v2 = cases.blob_volume((6, 32, 48), (0.2, 0.4, -0.3), seed=9)
    v1[:, :16, :16] = 0.3
    v2[:, 16:, 32:] = 0.1
    v1[:, :16, 32:] = 1.0
    v1[2, 5, 40] = np.float32(1.0) + np.float32(2.0 ** -23)               # energy 2^-46 (1 - 1/n): its f32 square underflows no float, but
    v1[:, :16, 32:] *= np.float32(1e-20)                                  # ... scaled by 1e-20 the square is below the smallest f32
    want = pt.correlate_volume_model(v1, v2, 16, 16, 2, 6, 6, 1, planes=True)
    vec, flg, pln = device_correlate_volume(photon, v1, v2, 16, 16, 2, 6, 6, 1)
    flat = np.zeros((1, 2, 3), bool)
    flat[0, 0, 0] = flat[0, 1, 2] = flat[0, 0, 2] = True
    assert ((flg & pc.FLAG_FLAT) != 0).tolist() == flat.tolist() and ((want[1] & pc.FLAG_FLAT) != 0)[0, 0, 0] and ((want[1] & pc.FLAG_FLAT) != 0)[0, 1, 2]
    assert np.isnan(vec[flat]).all() and np.isnan(pln[flat]).all() and np.isfinite(vec[~flat]).all() and np.isfinite(pln[~flat]).all()
    assert np.array_equal(flg[~flat], want[1][~flat]) and np.abs(vec[~flat][:, :3] - want[0][~flat][:, :3]).max() <= 1e-3


def correlate_job(keep, shape=(6, 40, 48)):
    import torch
    nz, ny, nx = shape
    keep["vol"] = torch.rand(shape, device="cuda")
    keep["vec"] = torch.full((4096, 5), 7.0, device="cuda")
    keep["flg"] = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    keep["pln"] = torch.full((4096, 3 * 81), 7.0, device="cuda")
    keep["sizes"] = [ctypes.c_int(-5) for _ in range(3)]
    return library.photon_piv_correlate_volume_t(d_vol1=keep["vol"].data_ptr(), d_vol2=keep["vol"].data_ptr(), nx=nx, ny=ny, nz=nz, win=16, step=8, radius=4,
                                                 win_z=4, step_z=2, radius_z=1, d_vectors=keep["vec"].data_ptr(), d_flags=keep["flg"].data_ptr(),
                                                 d_planes=keep["pln"].data_ptr(), n_slabs=ctypes.pointer(keep["sizes"][0]),
                                                 n_rows=ctypes.pointer(keep["sizes"][1]), n_cols=ctypes.pointer(keep["sizes"][2]), stream=None)


CORRELATE_REFUSALS = {
    "win_24": _set("win", 24), "win_128": _set("win", 128), "radius_0": _set("radius", 0), "radius_above_half_win": _set("radius", 9),
    "step_0": _set("step", 0), "slice_smaller_than_a_window": _set("ny", 15), "nx_0": _set("nx", 0), "nz_0": _set("nz", 0),
    "win_z_0": _set("win_z", 0), "win_z_65": _set("win_z", 65), "win_z_above_nz": _set("win_z", 7), "step_z_0": _set("step_z", 0),
    "radius_z_negative": _set("radius_z", -1), "radius_z_above_half_win_z": _set("radius_z", 3),
    "radius_z_17": lambda job: (setattr(job, "win_z", 6), setattr(job, "radius_z", 17)),
    "null_vol1": _set("d_vol1", None), "null_vol2": _set("d_vol2", None), "no_flags": _set("d_flags", None), "no_planes": _set("d_planes", None),
}


@pytest.mark.parametrize("what", list(CORRELATE_REFUSALS))
def test_correlate_volume_refusals_print_one_line_and_write_nothing(photon, capfd, what):
    import torch
    keep = {}
    job = correlate_job(keep)
    CORRELATE_REFUSALS[what](job)
    capfd.readouterr()
    rc = photon.lib.photon_piv_correlate_volume(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and len(err.strip().splitlines()) == 1 and "photon_piv_correlate_volume" in err, (what, err)
    assert [s.value for s in keep["sizes"]] == [-5, -5, -5]
    assert (keep["vec"] == 7.0).all().item() and (keep["flg"] == 7).all().item() and (keep["pln"] == 7.0).all().item()


def test_the_size_query_and_a_null_job(photon, capfd):
    capfd.readouterr()
    assert photon.lib.photon_piv_correlate_volume(None) == 1 and len(capfd.readouterr().err.strip().splitlines()) == 1
    keep = {}
    job = correlate_job(keep)
    job.d_vectors = job.d_flags = job.d_planes = None
    assert photon.lib.photon_piv_correlate_volume(ctypes.byref(job)) == 0 and capfd.readouterr().err == ""
    assert tuple(s.value for s in keep["sizes"]) == pt.grid_shape((6, 40, 48), 16, 8, 4, 2) == (2, 4, 5)
    assert (keep["vec"] == 7.0).all().item()
    vec, flg, pln = photon.piv_correlate_volume(keep["vol"].data_ptr(), keep["vol"].data_ptr(), 48, 40, 6, 16, 8, 4, 4, 2, 1)
    assert tuple(vec.shape) == (2, 4, 5, 5) and tuple(flg.shape) == (2, 4, 5) and tuple(pln.shape) == (2, 4, 5, 3, 9, 9)
    assert (vec[..., :3].abs() < 0.5).all().item() and (vec[..., 3] > 0.999).all().item()     # a volume against itself


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["min", "product"])
def test_reconstruct_volume_against_the_models(photon, mode):
    """The driver computes the coefficients on the device: the f32 model on those coefficients bit for bit, the f64 model
    from the frames within the CPU tier's bound."""
    import test_piv_stereo_gpu as stereo
    n = 3
    rng = np.random.default_rng(8)
    frames = [rng.random((2,) + cases.LOS_SENSORS[c % 2]).astype(np.float32) for c in range(n)]
    cams, vol = cases.los_cameras(n), cases.LOS_VOLUME
    got, mask = photon.reconstruct_volume(frames, cams, vol, mode=mode)
    assert got.is_cuda and tuple(got.shape) == (2,) + pt.shape_of(vol) and mask.dtype.is_floating_point is False
    got, mask = got.cpu().numpy(), mask.cpu().numpy()
    poly, grids = pt.los_coefficients(cams, vol)
    coefs = [stereo.device_coefficients(photon, f)[1] for f in frames]
    want32, mask32 = pt.los_model_f32(coefs, poly, grids, pt.shape_of(vol), mode)
    assert got.tobytes() == want32.tobytes() and np.array_equal(mask, mask32) and 0 < mask.sum() < mask.size
    want64, _ = pt.los_model(frames, poly, grids, pt.shape_of(vol), mode)
    M = np.abs(pt.los_samples(frames, poly, grids, pt.shape_of(vol))[0]).max()
    assert np.abs(got - want64).max() <= (1e-4 if mode == "min" else n * 1e-4 * M ** (n - 1) * 1.01)          # frames in [0, 1]: the CPU tier's bound
    single, mask1 = photon.reconstruct_volume([f[0] for f in frames], cams, vol, mode=mode)
    assert tuple(single.shape) == pt.shape_of(vol) and single.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(mask1.cpu().numpy(), mask)
    for bad in (dict(mode="root"), dict(cameras=cams[:1])):
        with pytest.raises(ValueError):
            photon.reconstruct_volume(frames, **{**dict(cameras=cams, vol=vol, mode=mode), **bad})


@pytest.mark.parametrize("name", list(pt.CASES))
def test_correlate_tomo_against_the_model_chain(photon, name):
    """The device chain on piv_tomo.CASES: per component the rms error over the interior nodes within the model chain's own
    figure on the same frames x 1.25 (section 4.3w's convention: f32 against f64 on a few dozen nodes), the flags of the
    interior nodes clean, `partial` the host's computation from the f64 mask."""
    frames, cameras, (m_d, m_vec, m_flags, m_partial) = cases.chain_model(name)
    d, vec, flags, partial = photon.correlate_tomo(list(frames), cameras, pt.CASE_VOLUME, **pt.CASE_GRID)
    rms, n = pt.case_figures(name, d)
    m_rms, _ = pt.case_figures(name, m_d)
    print(f"{name}: device rms dX dY dZ {rms.round(4)} voxels (model {m_rms.round(4)}) over {n} interior nodes")
    assert d.shape == m_d.shape and d.dtype == np.float64 and vec.shape == m_vec.shape and np.array_equal(partial, m_partial)
    assert np.array_equal(d, pt.CASE_VOLUME["pitch"] * vec[..., :3].astype(np.float64))
    assert n >= 12 and not (flags[pt.interior(flags.shape)] & ~pc.FLAG_OUTSIDE).any()
    assert (rms <= 1.25 * m_rms).all() and (rms <= np.array(cases.CHAIN_BARS[name])).all()


def test_correlate_tomo_partial_windows_and_offsets(photon):
    """A volume that reaches beyond one camera's sensor: `partial` is the host's windows_touching of the mask; offsets reach
    the kernel (dx follows them where the flow is uniform)."""
    frames, cameras, _ = cases.chain_model("three")
    wide = pt.centred_volume(128, 64, 16, 0.1)
    grid = dict(win=16, step=16, radius=3, win_z=8, step_z=8, radius_z=2)
    off = np.zeros(pt.grid_shape(pt.shape_of(wide), 16, 16, 8, 8) + (3,), np.int64)
    off[..., 0] = 1
    d, vec, flags, partial = photon.correlate_tomo(list(frames), cameras, wide, offsets=off, **grid)
    _, mask = pt.los_model(frames, *pt.los_coefficients(cameras, wide), pt.shape_of(wide), "min")
    want = pt.windows_touching(mask, 16, 16, 8, 8)
    assert np.array_equal(partial, want) and want.any() and not want.all()
    m_d, m_vec, m_flags, _ = pt.correlate_tomo_model(frames, cameras, wide, offsets=off, **grid)
    seen = ~want & ((m_flags & (pc.FLAG_FLAT | pc.FLAG_EDGE_PEAK)) == 0)
    assert seen.sum() >= 4 and np.array_equal(flags[seen], m_flags[seen]) and np.median(np.abs(vec[seen][:, :3] - m_vec[seen][:, :3])) <= 1e-3
    assert np.abs(np.median(vec[seen][:, 0]) - 1.6) < 0.2                       # ox + the residual: the offsets were read
    with pytest.raises(ValueError):
        photon.correlate_tomo(list(frames), cameras, wide, offsets=off[..., :2], **grid)
    with pytest.raises(ValueError):
        photon.correlate_tomo([f[:1] for f in frames], cameras, wide, **grid)
