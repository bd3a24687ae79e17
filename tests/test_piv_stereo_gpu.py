"""Stereo PIV on the device (include/parallel_ray_tracing.h, section 19): photon_piv_dewarp bit for bit against
piv_stereo.dewarp_model_f32 on poisoned outputs, photon_piv_stereo_reconstruct against piv_stereo.reconstruct_model to 1e-12,
and the driver PhotonLibrary.correlate_stereo against the same calls made by hand, on the arrays callers hold, and on three
synthetic stereo pairs against the model chain.  The held-back-stream cases: tests/test_zz_piv_stereo_streams_gpu.py."""
import ctypes

import numpy as np
import pytest

import piv_stereo_cases as cases
import test_streams_gpu as ts
from photon_amd import library
from photon_amd import piv_stereo as ps

pytestmark = pytest.mark.gpu

POISON, MASK_POISON = np.float32(-12345.5), 0xAB


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def device_coefficients(photon, im):
    """Section 7a's coefficients of the frames im f32 [n, h, w], computed on the device: (device tensor, numpy copy)."""
    import torch
    n, h, w = im.shape
    src, coef = dev(im), torch.full((n, h, w), float(POISON), dtype=torch.float32, device="cuda")
    for k in range(n):
        photon.bspline_coefficients(src[k].data_ptr(), w, h, coef[k].data_ptr())
    torch.cuda.synchronize()
    return coef, coef.cpu().numpy()


def run_dewarp(photon, coef, poly, grid, out, n_frames, in_stride=None, out_stride=None, with_mask=True, extra=1):
    """One photon_piv_dewarp of the first n_frames frames of coef (numpy f32 [n, h, w]) laid out in_stride apart, into a
    poisoned buffer of n_frames + extra frames out_stride apart and a poisoned mask.  Returns (buffer f32 [n_frames + extra,
    out_stride], mask u8 [oh, ow] or None)."""
    import torch
    n, h, w = coef.shape
    oh, ow = out
    in_stride, out_stride = in_stride or h * w, out_stride or oh * ow
    src = np.full((n, in_stride), 777.0, np.float32)
    src[:, :h * w] = coef.reshape(n, -1)
    d_src = dev(src)
    d_out = torch.full((n_frames + extra, out_stride), float(POISON), dtype=torch.float32, device="cuda")
    d_mask = torch.full((oh, ow), MASK_POISON, dtype=torch.uint8, device="cuda")
    photon.piv_dewarp(d_src.data_ptr(), in_stride, n_frames, w, h, poly, grid, ow, oh, out_stride, d_out.data_ptr(),
                      d_mask.data_ptr() if with_mask else 0)
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), src)                      # the input is not written
    return d_out.cpu().numpy(), (d_mask.cpu().numpy() if with_mask else None)


def assert_dewarp(buf, mask, coef, poly, grid, out, n_frames):
    oh, ow = out
    want, want_mask = ps.dewarp_model_f32(coef[:n_frames], poly, grid, out)
    got = buf[:n_frames, :oh * ow].reshape(n_frames, oh, ow)
    assert got.tobytes() == want.tobytes(), f"{(got != want).sum()} pixels differ, largest {np.abs(got - want).max():.3e}"
    if mask is not None:
        assert np.array_equal(mask, want_mask)
        assert (got[:, mask == 1] == 0).all()
    assert (buf[n_frames:] == POISON).all() and (buf[:, oh * ow:] == POISON).all()       # frames beyond n_frames, the stride gaps


@pytest.fixture(scope="module")
def src_coefficients(photon):
    return device_coefficients(photon, cases.image(cases.SRC, 21, n=3))[1]


# ---- dewarp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["fit", "full", "rotated", "half", "double", "partly_outside", "all_outside", "overflow"])
@pytest.mark.parametrize("out", cases.OUTS, ids=lambda o: f"{o[1]}x{o[0]}")
def test_dewarp_returns_the_f32_models_bits(photon, src_coefficients, out, camera):
    poly, grid = cases.dewarp_cameras(cases.SRC, out)[camera]
    buf, mask = run_dewarp(photon, src_coefficients, poly, grid, out, 2)
    assert_dewarp(buf, mask, src_coefficients, poly, grid, out, 2)
    again, mask2 = run_dewarp(photon, src_coefficients, poly, grid, out, 2)
    assert again.tobytes() == buf.tobytes() and mask2.tobytes() == mask.tobytes()        # two calls, the same bytes
    if camera == "partly_outside":
        assert set(np.unique(mask)) == {0, 1}
    if camera == "all_outside":
        assert mask.all() and (buf[:2] == 0).all()
    no_mask, none = run_dewarp(photon, src_coefficients, poly, grid, out, 2, with_mask=False)
    assert none is None and no_mask.tobytes() == buf.tobytes()                           # a NULL mask changes no image


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "stride_plus_5"])
@pytest.mark.parametrize("n_frames", [1, 2, 3])
def test_dewarp_frames_and_strides(photon, src_coefficients, n_frames, padded):
    out = cases.OUTS[0]
    poly, grid = cases.dewarp_cameras(cases.SRC, out)["full"]
    h, w = cases.SRC
    strides = dict(in_stride=h * w + 5, out_stride=out[0] * out[1] + 5) if padded else {}
    buf, mask = run_dewarp(photon, src_coefficients, poly, grid, out, n_frames, **strides)
    assert_dewarp(buf, mask, src_coefficients, poly, grid, out, n_frames)


@pytest.mark.parametrize("src", [(1, 1), (4, 3)], ids=["1x1", "3x4"])
def test_dewarp_of_sources_smaller_than_the_taps(photon, src):
    """Every tap of a 1 x 1 source and the outer taps of a 3 x 4 one lie more than one reflection away (piv_warp::mirror_far)."""
    _, coef = device_coefficients(photon, cases.image(src, 4, n=2))
    out = cases.OUTS[0]
    for poly, grid in (cases.fit_to(src, out), cases.affine(0.0, 0.1, 0.0, 0.0, 0.0, 0.05), cases.affine(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)):
        buf, mask = run_dewarp(photon, coef, poly, grid, out, 2)
        assert_dewarp(buf, mask, coef, poly, grid, out, 2)
        assert not mask.all()


def test_the_identity_camera_returns_the_warp_at_zero_shift(photon):
    import torch
    d_coef, coef = device_coefficients(photon, cases.image((64, 64), 9, n=1))
    poly, grid = ps.plane_coefficients(ps.identity_camera(), ps.plane(0.0, 0.0, 1.0, 0.0, 64, 64))
    buf, mask = run_dewarp(photon, coef, poly, grid, (64, 64), 1)
    field = torch.full((4, 4, 2), 3.25, dtype=torch.float32, device="cuda")
    warped = torch.full((64, 64), float(POISON), dtype=torch.float32, device="cuda")
    photon.piv_deform(d_coef.data_ptr(), 64, 64, field.data_ptr(), 2, 4, 4, 16, 16, 0.0, warped.data_ptr())
    torch.cuda.synchronize()
    assert not mask.any() and buf[0].tobytes() == warped.cpu().numpy().tobytes()


def dewarp_job(d_src, d_out, d_mask, src, out, n_frames=2):
    poly, grid = cases.dewarp_cameras(src, out)["full"]
    job = library.photon_piv_dewarp_t(d_coef=d_src.data_ptr(), frame_stride=src[0] * src[1], n_frames=n_frames, width=src[1], height=src[0],
                                      out_width=out[1], out_height=out[0], out_stride=out[0] * out[1], d_out=d_out.data_ptr(),
                                      d_mask=d_mask.data_ptr(), stream=None)
    for k in range(10):
        job.poly[0][k], job.poly[1][k] = poly[0, k], poly[1, k]
    for k in range(4):
        job.grid[k] = grid[k]
    return job


DEWARP_REFUSALS = {
    "null_coef": lambda j: setattr(j, "d_coef", None),
    "null_out": lambda j: setattr(j, "d_out", None),
    "out_is_coef": lambda j: setattr(j, "d_out", j.d_coef),
    "width_0": lambda j: setattr(j, "width", 0),
    "height_negative": lambda j: setattr(j, "height", -3),
    "out_width_0": lambda j: setattr(j, "out_width", 0),
    "out_height_0": lambda j: setattr(j, "out_height", 0),
    "side_above_2_22": lambda j: setattr(j, "out_width", (1 << 22) + 1),
    "no_frames": lambda j: setattr(j, "n_frames", 0),
    "frame_stride_short": lambda j: setattr(j, "frame_stride", j.width * j.height - 1),
    "out_stride_short": lambda j: setattr(j, "out_stride", j.out_width * j.out_height - 1),
    "nan_poly": lambda j: j.poly[1].__setitem__(7, float("nan")),
    "inf_grid": lambda j: j.grid.__setitem__(1, float("inf")),
}


@pytest.mark.parametrize("what", [*DEWARP_REFUSALS, "null_job"])
def test_dewarp_refusals_write_nothing(photon, src_coefficients, capfd, what):
    import torch
    out = cases.OUTS[0]
    d_src = dev(src_coefficients)
    d_out = torch.full((3, out[0] * out[1]), float(POISON), dtype=torch.float32, device="cuda")
    d_mask = torch.full(out, MASK_POISON, dtype=torch.uint8, device="cuda")
    job = dewarp_job(d_src, d_out, d_mask, cases.SRC, out)
    assert photon.lib.photon_piv_dewarp(ctypes.byref(job)) == 0          # the job is sound before it is broken
    torch.cuda.synchronize()
    d_out.fill_(float(POISON))
    d_mask.fill_(MASK_POISON)
    torch.cuda.synchronize()
    capfd.readouterr()
    if what == "null_job":
        rc = photon.lib.photon_piv_dewarp(None)
    else:
        DEWARP_REFUSALS[what](job)
        rc = photon.lib.photon_piv_dewarp(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and err.count("\n") == 1 and err.startswith("photon: photon_piv_dewarp: "), err
    assert (d_out.cpu().numpy() == POISON).all() and (d_mask.cpu().numpy() == MASK_POISON).all()
    assert np.array_equal(d_src.cpu().numpy(), src_coefficients)


# ---- reconstruction ----------------------------------------------------------------------------------------------------------
def run_reconstruct(photon, pl, cams, fields, flags, sigmas, stride, stream=0):
    import torch
    f = [dev(np.ascontiguousarray(x[..., :stride])) for x in fields]
    g = [None, None] if flags is None else [dev(x) for x in flags]
    s = [None, None] if sigmas is None else [dev(x) for x in sigmas]
    ptr = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
    out, flg = photon.piv_stereo_reconstruct(f[0].data_ptr(), f[1].data_ptr(), stride, cams, pl, cases.WIN, cases.STEP, ptr(g[0]), ptr(g[1]),
                                             ptr(s[0]), ptr(s[1]), stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), flg.cpu().numpy()


def assert_reconstruction(got, got_flags, want, want_flags, what):
    """Equal flags, equal NaN positions, every finite output within 1e-12 of the model's, relative to itself."""
    assert np.array_equal(got_flags, want_flags), what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isfinite(want)
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    print(f"{what}: {ok.sum()} finite outputs, largest relative difference {rel.max() if rel.size else 0.0:.2e}")
    assert (rel <= 1e-12).all(), what


@pytest.mark.parametrize("with_sigmas", [False, True], ids=["no_sigmas", "sigmas"])
@pytest.mark.parametrize("with_flags", [False, True], ids=["no_flags", "flags"])
@pytest.mark.parametrize("stride", [2, 4])
@pytest.mark.parametrize("grid", list(cases.GRIDS))
def test_reconstruct_against_the_model(photon, grid, stride, with_flags, with_sigmas):
    pl, fields, flags, sigmas = cases.stereo_inputs(grid)
    cams = cases.cameras("asymmetric")
    flags, sigmas = (flags if with_flags else None), (sigmas if with_sigmas else None)
    got, got_flags = run_reconstruct(photon, pl, cams, fields, flags, sigmas, stride)
    want, want_flags = ps.reconstruct_model(fields[0], fields[1], cams, pl, cases.WIN, cases.STEP, *(flags or (None, None)), *(sigmas or (None, None)))
    assert got.shape == want.shape and got.dtype == np.float64 and got_flags.dtype == np.int32
    assert_reconstruction(got, got_flags, want, want_flags, f"{grid} stride {stride}")
    if grid != "1x1":
        assert (want_flags & ps.FLAG_NOT_FINITE).sum() == 2 * ps.FLAG_NOT_FINITE and np.isfinite(want[..., :4]).any()
        assert np.isnan(want[..., 4:7]).all() != with_sigmas
    again, again_flags = run_reconstruct(photon, pl, cams, fields, flags, sigmas, stride)
    assert again.tobytes() == got.tobytes() and again_flags.tobytes() == got_flags.tobytes()


def test_reconstruct_flags_a_degenerate_camera_pair(photon):
    pl, fields, flags, sigmas = cases.stereo_inputs("9x11")
    cam = cases.cameras("symmetric")[0]
    got, got_flags = run_reconstruct(photon, pl, (cam, cam), fields, flags, sigmas, 4)
    want, want_flags = ps.reconstruct_model(fields[0], fields[1], (cam, cam), pl, cases.WIN, cases.STEP, *flags, *sigmas)
    assert np.isnan(got).all() and ((got_flags & ps.FLAG_DEGENERATE) != 0).all()
    assert_reconstruction(got, got_flags, want, want_flags, "degenerate")


def stereo_job(pl, cams, tensors, out, flg, rows, cols):
    job = library._stereo_job(cams, pl, cases.WIN, cases.STEP)
    job.d_field1, job.d_field2, job.field_stride = tensors["f1"].data_ptr(), tensors["f2"].data_ptr(), 4
    job.d_sigma1, job.d_sigma2 = tensors["s1"].data_ptr(), tensors["s2"].data_ptr()
    job.n_rows, job.n_cols, job.d_out, job.d_flags = 9, 11, out.data_ptr(), flg.data_ptr()
    job.rows_out, job.cols_out = ctypes.pointer(rows), ctypes.pointer(cols)
    return job


STEREO_REFUSALS = {
    "win_24": lambda j: setattr(j, "win", 24),
    "step_0": lambda j: setattr(j, "step", 0),
    "plane_smaller_than_a_window": lambda j: setattr(j.plane, "width", 31),
    "not_the_grid": lambda j: setattr(j, "n_cols", 10),
    "null_field": lambda j: setattr(j, "d_field2", None),
    "null_flags_out": lambda j: setattr(j, "d_flags", None),
    "stride_3": lambda j: setattr(j, "field_stride", 3),
    "one_sigma": lambda j: setattr(j, "d_sigma1", None),
    "nan_plane": lambda j: setattr(j.plane, "y0", float("nan")),
    "pitch_0": lambda j: setattr(j.plane, "pitch", 0.0),
    "scale_0": lambda j: j.camera2.scale.__setitem__(2, 0.0),
    "inf_camera": lambda j: j.camera1.cy.__setitem__(18, float("inf")),
}


@pytest.mark.parametrize("what", [*STEREO_REFUSALS, "null_job"])
def test_reconstruct_refusals_write_nothing(photon, capfd, what):
    import torch
    pl, fields, _, sigmas = cases.stereo_inputs("9x11")
    t = {"f1": dev(fields[0]), "f2": dev(fields[1]), "s1": dev(sigmas[0]), "s2": dev(sigmas[1])}
    out = torch.full((9, 11, 8), -4.5, dtype=torch.float64, device="cuda")
    flg = torch.full((9, 11), -9, dtype=torch.int32, device="cuda")
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    job = stereo_job(pl, cases.cameras("symmetric"), t, out, flg, rows, cols)
    torch.cuda.synchronize()
    capfd.readouterr()
    if what == "null_job":
        rc = photon.lib.photon_piv_stereo_reconstruct(None)
    else:
        STEREO_REFUSALS[what](job)
        rc = photon.lib.photon_piv_stereo_reconstruct(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and err.count("\n") == 1 and err.startswith("photon: photon_piv_stereo_reconstruct: "), err
    assert (out.cpu().numpy() == -4.5).all() and (flg.cpu().numpy() == -9).all() and (rows.value, cols.value) == (-1, -1)


def test_reconstruct_size_query(photon):
    job = library._stereo_job(cases.cameras("symmetric"), cases.PLANE, cases.WIN, cases.STEP)
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    job.rows_out, job.cols_out = ctypes.pointer(rows), ctypes.pointer(cols)
    assert photon.lib.photon_piv_stereo_reconstruct(ctypes.byref(job)) == 0 and (rows.value, cols.value) == (9, 11)


# ---- the driver --------------------------------------------------------------------------------------------------------------
SETTINGS = dict(win=cases.WIN, step=cases.STEP, radius=cases.RADIUS, iterations=cases.ITERATIONS)
SHIFTED = ps.plane(cases.PLANE["x0"] + 18.0, cases.PLANE["y0"], 0.2, 0.0, 192, 160)           # its last 38 columns are outside both sensors


def by_hand(photon, f1, f2, cams, pl, evaluate, sigma):
    """correlate_stereo's steps through the raw-pointer methods and the planar drivers, one after the other."""
    import torch
    oh, ow = pl["height"], pl["width"]
    vectors, status, sigmas = [], [], []
    for frames, cam in zip((f1, f2), cams):
        n, h, w = frames.shape
        d_coef, _ = device_coefficients(photon, np.asarray(frames, np.float32))
        poly, grid = ps.plane_coefficients(cam, pl)
        d_out = torch.full((n, oh, ow), float(POISON), dtype=torch.float32, device="cuda")
        d_mask = torch.full((oh, ow), MASK_POISON, dtype=torch.uint8, device="cuda")
        photon.piv_dewarp(d_coef.data_ptr(), h * w, n, w, h, poly, grid, ow, oh, oh * ow, d_out.data_ptr(), d_mask.data_ptr())
        torch.cuda.synchronize()
        mask = d_mask if bool(d_mask.any()) else None
        if evaluate == "correlate":
            v, s = photon.correlate(d_out[0], d_out[1], win=cases.WIN, step=cases.STEP, radius=cases.RADIUS, mask=mask)
            win, step = cases.WIN, cases.STEP
        elif evaluate == "deform":
            v, s = photon.correlate_deform(d_out[0], d_out[1], win=cases.WIN, step=cases.STEP, radius=cases.RADIUS, iterations=cases.ITERATIONS,
                                           mask=mask)
            win, step = cases.WIN, cases.STEP
        else:
            v, s = photon.correlate_multigrid(d_out[0], d_out[1], schedule=((64, 32), (32, 16)), iterations=(1, 1), radius=cases.RADIUS, mask=mask)
            win, step = 32, 16
        vectors.append(v)
        status.append(s)
        if sigma:
            sigmas.append(photon.displacement_uncertainty(d_out[0], d_out[1], v, win=win, step=step)[0])
    t = [dev(x) for x in (*vectors, *status, *sigmas)]
    out, flags = photon.piv_stereo_reconstruct(t[0].data_ptr(), t[1].data_ptr(), 4, cams, pl, win, step, t[2].data_ptr(), t[3].data_ptr(),
                                               *(x.data_ptr() for x in t[4:]))
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), tuple(vectors)


@pytest.mark.parametrize("evaluate,plane,sigma", [("deform", "inside", True), ("deform", "shifted", False), ("correlate", "shifted", True),
                                                  ("multigrid", "inside", False)])
def test_the_driver_returns_what_the_same_calls_made_by_hand_return(photon, evaluate, plane, sigma):
    f1, f2 = cases.accuracy_pair("uniform")
    cams, pl = cases.cameras("symmetric"), (cases.PLANE if plane == "inside" else SHIFTED)
    settings = dict(SETTINGS) if evaluate != "multigrid" else dict(schedule=((64, 32), (32, 16)), iterations=(1, 1), radius=cases.RADIUS)
    if evaluate == "correlate":
        del settings["iterations"]
    got = photon.correlate_stereo(f1, f2, cams, pl, evaluate=evaluate, settings=settings, sigma=sigma)
    want = by_hand(photon, f1, f2, cams, pl, evaluate, sigma)
    assert got[0].shape == (9, 11, 8) and got[1].shape == (9, 11) and got[2][0].shape == (9, 11, 4)
    assert ts.flatten(got) == ts.flatten(want)
    assert np.isfinite(got[0][..., :4]).any() and np.isfinite(got[0][..., 4:7]).any() == sigma
    if plane == "shifted":
        assert (got[1] & 16).any() and (got[1] & ps.FLAG_NOT_FINITE).any() and not (got[1] & ps.FLAG_NOT_FINITE).all()


def test_dewarp_driver_returns_the_raw_calls_bytes(photon):
    import torch
    f1, _ = cases.accuracy_pair("uniform")
    cam = cases.cameras("symmetric")[0]
    frames, mask = photon.dewarp(f1, cam, SHIFTED)
    one, mask1 = photon.dewarp(f1[1], cam, SHIFTED)
    torch.cuda.synchronize()
    _, coef = device_coefficients(photon, np.asarray(f1))
    want, want_mask = ps.dewarp_model_f32(coef, *ps.plane_coefficients(cam, SHIFTED), (160, 192))
    assert frames.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(mask.cpu().numpy(), want_mask)
    assert one.shape == (160, 192) and one.cpu().numpy().tobytes() == want[1].tobytes() and np.array_equal(mask1.cpu().numpy(), want_mask)
    assert set(np.unique(want_mask)) == {0, 1}


def test_the_driver_takes_camera_counts_and_views_and_writes_no_input(photon):
    """uint16 counts in every other column of a wider buffer: the one ingest rule makes the f32 stack of them."""
    f1, f2 = cases.accuracy_pair("uniform")
    cams = cases.cameras("symmetric")
    wide = [np.zeros((2, 224, 512), np.uint16) for _ in range(2)]
    for buf, f in zip(wide, (f1, f2)):
        buf[:, :, ::2] = np.rint(4000.0 * f)
    views = [buf[:, :, ::2] for buf in wide]
    assert not views[0].flags.c_contiguous and views[0].max() > 1000
    before = [buf.copy() for buf in wide]
    settings = dict(SETTINGS, iterations=1)
    got = photon.correlate_stereo(views[0], views[1], cams, cases.PLANE, settings=settings)
    want = photon.correlate_stereo(*(np.ascontiguousarray(v).astype(np.float32) for v in views), cams, cases.PLANE, settings=settings)
    assert ts.flatten(got) == ts.flatten(want) and np.isfinite(got[0][..., :4]).all()
    assert all(np.array_equal(a, b) for a, b in zip(wide, before))
    with pytest.raises(ValueError, match="unknown settings"):
        photon.correlate_stereo(f1, f2, cams, cases.PLANE, settings=dict(window=32))
    with pytest.raises(ValueError, match="cam2_frames"):
        photon.correlate_stereo(f1, f2[0], cams, cases.PLANE)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.ACCURACY))
def test_the_device_chain_measures_three_components(photon, name):
    """The two conditions of the model chain (tests/test_piv_stereo.py) on the device's, and the device's rms errors against
    the model chain's on the same pair: the model's own figure x 1.25, the margin for f32 against f64 correlation on 63 nodes.
    Measured on one MI355X: DESIGN.md section 4.3w."""
    f1, f2 = cases.accuracy_pair(name)
    out, status, (v1, _) = photon.correlate_stereo(f1, f2, cases.cameras(cases.ACCURACY[name][0]), cases.PLANE, settings=SETTINGS)
    rms, alone, median, worst = cases.figures(name, out, v1)
    m_rms, m_alone, m_median, m_worst = cases.model_figures(name)
    print(f"{name}: device rms dX dY dZ {rms.round(4)} px (model {m_rms.round(4)}), camera 1 alone {alone:.3f} px (model {m_alone:.3f}), ratio "
          f"{rms[0] / alone:.3f}, residual median {median:.4f} max {worst:.4f} px (model {m_median:.4f}, {m_worst:.4f})")
    assert not (status & (ps.FLAG_DEGENERATE | ps.FLAG_NOT_FINITE)).any()
    assert rms[0] <= 0.2 * alone and median < 0.1
    assert (rms <= 1.25 * m_rms).all()
