"""Stereo self-calibration on the device (include/parallel_ray_tracing.h, section 19c): photon_piv_stereo_triangulate against
piv_stereo.triangulate_model to 1e-12 of each output, on pre-filled outputs with a guard band behind them, and the driver
PhotonLibrary.self_calibrate_stereo on piv_stereo.SELFCAL_CASE against the model's rounds and against the truth.  The
held-back-stream cases and the timing bound: tests/test_zz_piv_stereo_selfcal_perf_gpu.py."""
import ctypes

import numpy as np
import pytest

import piv_stereo_cases as base
import piv_stereo_selfcal_cases as cases
from photon_amd import library
from photon_amd import piv_stereo as ps

pytestmark = pytest.mark.gpu

OUT_FILL, FLAG_FILL, GUARD = -4.5, -9, 7          # GUARD: nodes' worth of space behind both outputs that no call may touch


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def triangulate_job(pl, cams, field, flags, out, flg, rows, cols, win=cases.WIN, step=cases.STEP, iterations=4, grid=None):
    """Section 19c's job on the device tensors field [r, c, stride] and flags (or None), out and flg as its outputs."""
    job = library._stereo_job(cams, pl, win, step, library.photon_piv_triangulate_t)
    job.d_disparity, job.field_stride, job.d_flags_in = field.data_ptr(), int(field.shape[-1]), (None if flags is None else flags.data_ptr())
    job.n_rows, job.n_cols = grid or tuple(field.shape[:2])
    job.iterations, job.d_out, job.d_flags = iterations, out.data_ptr(), flg.data_ptr()
    job.rows_out, job.cols_out = ctypes.pointer(rows), ctypes.pointer(cols)
    return job


def run_triangulate(photon, pl, cams, field, flags, stride, iterations):
    """One photon_piv_stereo_triangulate into pre-filled outputs with GUARD nodes of space behind them: (out [r, c, 6], flags
    [r, c]); the guard bands and the inputs are checked here."""
    import torch
    r, c = field.shape[:2]
    d_field = dev(np.ascontiguousarray(field[..., :stride]))
    d_flags = None if flags is None else dev(flags)
    out = torch.full((r * c + GUARD, 6), OUT_FILL, dtype=torch.float64, device="cuda")
    flg = torch.full((r * c + GUARD,), FLAG_FILL, dtype=torch.int32, device="cuda")
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    job = triangulate_job(pl, cams, d_field, d_flags, out, flg, rows, cols, iterations=iterations)
    assert photon.lib.photon_piv_stereo_triangulate(ctypes.byref(job)) == 0 and (rows.value, cols.value) == (r, c)
    torch.cuda.synchronize()
    got, got_flags = out.cpu().numpy(), flg.cpu().numpy()
    assert (got[r * c:] == OUT_FILL).all() and (got_flags[r * c:] == FLAG_FILL).all(), "written beyond the grid's nodes"
    assert d_field.cpu().numpy().tobytes() == np.ascontiguousarray(field[..., :stride]).tobytes()
    return got[:r * c].reshape(r, c, 6), got_flags[:r * c].reshape(r, c)


def assert_triangulation(got, got_flags, want, want_flags, what):
    """Equal flags, equal NaN positions, every finite output within 1e-12 of the model's, relative to itself."""
    assert got.shape == want.shape and got.dtype == np.float64 and got_flags.dtype == np.int32
    assert np.array_equal(got_flags, want_flags), what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isfinite(want)
    diff, scale = np.abs(got[ok] - want[ok]), np.abs(want[ok])
    rel = diff[scale > 0] / scale[scale > 0]
    print(f"{what}: {ok.sum()} finite outputs, largest relative difference {rel.max() if rel.size else 0.0:.2e}, {int((diff != 0).sum())} "
          f"outputs differ at all")
    assert (diff <= 1e-12 * scale).all(), what


# ---- the triangulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_flags", [False, True], ids=["no_flags", "flags"])
@pytest.mark.parametrize("stride", [2, 4])
@pytest.mark.parametrize("grid", list(cases.GRIDS))
def test_triangulate_against_the_model(photon, grid, stride, with_flags):
    import torch
    pl, field, flags = cases.disparity_inputs(grid)
    cams = base.cameras("asymmetric")
    flags = flags if with_flags else None
    got, got_flags = run_triangulate(photon, pl, cams, field, flags, stride, 4)
    want, want_flags = ps.triangulate_model(field, cams, pl, cases.WIN, cases.STEP, 4, flags)
    assert_triangulation(got, got_flags, want, want_flags, f"{grid} stride {stride}")
    if grid != "1x1":
        r, c = field.shape[:2]
        assert want_flags[0, 1] & ps.FLAG_NOT_FINITE and want_flags[r - 1, c - 1] & ps.FLAG_NOT_FINITE
        assert (want_flags & ps.FLAG_NOT_FINITE).sum() == 2 * ps.FLAG_NOT_FINITE and not (want_flags & ps.FLAG_DEGENERATE).any()
        assert np.isnan(got[0, 1, :5]).all() and got[0, 1, 5] > 0.01 and np.isfinite(got).sum() == 6 * r * c - 10
    assert (got[..., 4][np.isfinite(got[..., 4])] < 1e-9).all()                        # four iterations have converged
    again, again_flags = run_triangulate(photon, pl, cams, field, flags, stride, 4)
    assert again.tobytes() == got.tobytes() and again_flags.tobytes() == got_flags.tobytes()
    d_field, d_flags = dev(np.ascontiguousarray(field[..., :stride])), (None if flags is None else dev(flags))
    out, flg = photon.piv_stereo_triangulate(d_field.data_ptr(), stride, cams, pl, cases.WIN, cases.STEP, 4, 0 if d_flags is None else d_flags.data_ptr())
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == got.tobytes() and flg.cpu().numpy().tobytes() == got_flags.tobytes()       # the wrapper: the same call


@pytest.mark.parametrize("iterations", [1, 2, 16])
@pytest.mark.parametrize("kind", list(base.ANGLES))
def test_triangulate_iterations_and_cameras(photon, kind, iterations):
    pl, field, flags = cases.disparity_inputs("9x29")
    cams = base.cameras(kind)
    got, got_flags = run_triangulate(photon, pl, cams, field, flags, 4, iterations)
    want, want_flags = ps.triangulate_model(field, cams, pl, cases.WIN, cases.STEP, iterations, flags)
    assert_triangulation(got, got_flags, want, want_flags, f"{kind}, {iterations} iterations")


def test_triangulate_a_known_surface(photon):
    """The disparity of Z = 0.8 + 0.02 X - 0.015 Y, rounded to f32 (2e-7 px: 1e-7 mm of Z): the device returns the surface."""
    cams, pl = base.cameras("symmetric"), cases.grid_plane("5x7")
    W, d = cases.surface_disparity(cams, pl, lambda X, Y: 0.8 + 0.02 * X - 0.015 * Y)
    got, got_flags = run_triangulate(photon, pl, cams, d.astype(np.float32), None, 2, 4)
    print(f"points off by {np.abs(got[..., :3] - W).max():.2e} mm, error {got[..., 3].max():.2e} px, last step {got[..., 4].max():.2e} mm")
    assert not got_flags.any() and np.abs(got[..., :3] - W).max() < 1e-6 and got[..., 3].max() < 1e-5 and got[..., 4].max() < 1e-10


def test_triangulate_flags_two_cameras_on_one_line_of_sight(photon):
    pl, field, flags = cases.disparity_inputs("5x7")
    cam = base.cameras("symmetric")[0]
    got, got_flags = run_triangulate(photon, pl, (cam, cam), field, flags, 4, 3)
    want, want_flags = ps.triangulate_model(field, (cam, cam), pl, cases.WIN, cases.STEP, 3, flags)
    assert np.isnan(got[..., :5]).all() and ((got_flags & ps.FLAG_DEGENERATE) != 0).all() and ((got_flags & ~(64 | 128)) == flags).all()
    assert np.array_equal(got_flags, want_flags) and np.array_equal(np.isnan(got), np.isnan(want))
    assert not (got[..., 5] > ps.MIN_PIVOT_RATIO).any()


TRIANGULATE_REFUSALS = {
    "win_24": lambda j: setattr(j, "win", 24),
    "step_0": lambda j: setattr(j, "step", 0),
    "plane_smaller_than_a_window": lambda j: setattr(j.plane, "width", 31),
    "not_the_grid": lambda j: setattr(j, "n_cols", 6),
    "null_disparity": lambda j: setattr(j, "d_disparity", None),
    "null_flags_out": lambda j: setattr(j, "d_flags", None),
    "stride_3": lambda j: setattr(j, "field_stride", 3),
    "no_iterations": lambda j: setattr(j, "iterations", 0),
    "iterations_17": lambda j: setattr(j, "iterations", 17),
    "nan_plane": lambda j: setattr(j.plane, "x0", float("nan")),
    "pitch_negative": lambda j: setattr(j.plane, "pitch", -0.2),
    "scale_0": lambda j: j.camera1.scale.__setitem__(0, 0.0),
    "inf_camera": lambda j: j.camera2.cx.__setitem__(3, float("inf")),
}


@pytest.mark.parametrize("what", [*TRIANGULATE_REFUSALS, "null_job"])
def test_triangulate_refusals_write_nothing(photon, capfd, what):
    import torch
    pl, field, flags = cases.disparity_inputs("5x7")
    d_field, d_flags = dev(field), dev(flags)
    out = torch.full((35 + GUARD, 6), OUT_FILL, dtype=torch.float64, device="cuda")
    flg = torch.full((35 + GUARD,), FLAG_FILL, dtype=torch.int32, device="cuda")
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    job = triangulate_job(pl, base.cameras("symmetric"), d_field, d_flags, out, flg, rows, cols)
    torch.cuda.synchronize()
    capfd.readouterr()
    if what == "null_job":
        rc = photon.lib.photon_piv_stereo_triangulate(None)
    else:
        TRIANGULATE_REFUSALS[what](job)
        rc = photon.lib.photon_piv_stereo_triangulate(ctypes.byref(job))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert rc == 1 and err.count("\n") == 1 and err.startswith("photon: photon_piv_stereo_triangulate: "), err
    assert (out.cpu().numpy() == OUT_FILL).all() and (flg.cpu().numpy() == FLAG_FILL).all() and (rows.value, cols.value) == (-1, -1)


def test_triangulate_size_query(photon):
    job = library._stereo_job(base.cameras("symmetric"), cases.grid_plane("9x29"), cases.WIN, cases.STEP, library.photon_piv_triangulate_t)
    job.iterations = 4
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    job.rows_out, job.cols_out = ctypes.pointer(rows), ctypes.pointer(cols)
    assert photon.lib.photon_piv_stereo_triangulate(ctypes.byref(job)) == 0 and (rows.value, cols.value) == (9, 29)
    job.rows_out = job.cols_out = None
    assert photon.lib.photon_piv_stereo_triangulate(ctypes.byref(job)) == 0


# ---- the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_result(photon):
    frames = cases.inputs()[1]
    return photon.self_calibrate_stereo(frames[0], frames[1], cases.cameras(), cases.PLANE, **cases.DISPARITY)


def test_the_driver_finds_the_models_sheet_round_by_round(device_result):
    """The f32 device chain against the f64 model: per round the sheet within 1e-3 mm and 1e-4 of slope.  Measured on one
    MI355X: DESIGN.md section 4.3w."""
    _, report = device_result
    _, model = cases.model_result()
    assert len(report["rounds"]) == len(model["rounds"])
    for k, (got, want) in enumerate(zip(report["rounds"], model["rounds"])):
        off = np.abs(np.array(got["sheet"]) - want["sheet"])
        print(f"round {k + 1}: device sheet {np.round(got['sheet'], 6)}, model {np.round(want['sheet'], 6)}, off by {off}; disparity rms "
              f"{got['disparity_rms']:.4f} px (model {want['disparity_rms']:.4f}), {got['nodes']} nodes (model {want['nodes']}), error median "
              f"{got['error_median']:.4f} px (model {want['error_median']:.4f})")
        assert off[0] <= 1e-3 and off[1] <= 1e-4 and off[2] <= 1e-4
        assert max(r[1] for r in got["refit"]) < 1e-6 and got["step_max"] < 1e-10
    assert sorted(report) == sorted(model) and sorted(report["rounds"][0]) == sorted(model["rounds"][0])


def test_the_driver_corrects_the_cameras(device_result):
    """The model's bars (tests/test_piv_stereo_selfcal.py) on the device's result."""
    corrected, report = device_result
    off = np.abs(np.array(report["sheet"]) - cases.SHEET)
    after, before = cases.camera_errors(corrected), cases.camera_errors(cases.cameras())
    print(f"device: sheet {np.round(report['sheet'], 5)} (off by {off.round(5)}), cameras within {max(after):.4f} px (before: {max(before):.2f} px; "
          f"model: {max(cases.camera_errors(cases.model_result()[0])):.4f} px)")
    assert off[0] <= 0.03 and off[1] <= 0.002 and off[2] <= 0.002
    assert report["rounds"][-1]["disparity_rms"] < 0.05 and max(after) <= 0.05 and min(before) > 1.0


def test_the_corrected_cameras_measure_the_third_component_on_the_device(photon, device_result):
    """correlate_stereo with the cameras the driver returned: the model chain's conditions, and the device's rms errors within
    the model chain's own x 1.25, as tests/test_piv_stereo_gpu.py holds the uncorrected chain."""
    corrected, report = device_result
    _, _, pair, aligned = cases.inputs()
    settings = dict(cases.EVALUATION)
    run = lambda f, cams: photon.correlate_stereo(f[0], f[1], cams, cases.PLANE, settings=settings)[0]     # noqa: E731
    before, _ = ps.selfcal_figures(run(pair, cases.cameras()))
    after, res = ps.selfcal_figures(run(pair, corrected), cases.report_frame(report))
    flat, _ = ps.selfcal_figures(run(aligned, cases.cameras()))
    (m_before, _), (m_after, m_res), (m_flat, _) = cases.model_evaluation()
    print(f"device rms dX dY dZ: uncorrected {before.round(4)} px (model {m_before.round(4)}), corrected {after.round(4)} px (model "
          f"{m_after.round(4)}), aligned sheet {flat.round(4)} px (model {m_flat.round(4)}); median residual {res:.4f} px (model {m_res:.4f})")
    assert after[2] <= 0.5 * before[2] and after[2] <= 1.25 * flat[2]
    assert after[0] <= 1.25 * before[0] and after[1] <= 1.25 * before[1]
    assert (after <= 1.25 * m_after).all()


def test_the_driver_takes_what_callers_hold_and_refuses_what_it_cannot_use(photon):
    frames = cases.inputs()[1]
    cams = cases.cameras()
    two = photon.self_calibrate_stereo(frames[0][:2], frames[1][:2], cams, cases.PLANE, rounds=1, **cases.DISPARITY)
    counts = [np.rint(4000.0 * f[:2]).astype(np.uint16) for f in frames]
    same = photon.self_calibrate_stereo(counts[0], counts[1], cams, cases.PLANE, rounds=1, **cases.DISPARITY)
    assert len(two[1]["rounds"]) == 1 and np.allclose(two[1]["sheet"], same[1]["sheet"], rtol=0, atol=1e-4)      # counts: 1 / 8000 of rounding; the model moves by 2e-6
    with pytest.raises(ValueError, match="same N"):
        photon.self_calibrate_stereo(frames[0][:2], frames[1][:3], cams, cases.PLANE)
    with pytest.raises(ValueError, match="two cameras"):
        photon.self_calibrate_stereo(frames[0], frames[1], cams[:1], cases.PLANE)
    with pytest.raises(ValueError, match="iterations"):
        photon.self_calibrate_stereo(frames[0], frames[1], cams, cases.PLANE, iterations=17)
    with pytest.raises(ValueError, match="passes"):
        photon.self_calibrate_stereo(frames[0], frames[1], cams, cases.PLANE, passes=3)


def test_two_passes_reach_a_disparity_beyond_the_radius(photon):
    """Radius 4 against 4.6 px of disparity: one pass reads edge peaks (flag 1, unusable), two passes follow the disparity."""
    frames = cases.inputs()[1]
    settings = dict(cases.DISPARITY, radius=4)
    with pytest.raises(ValueError, match="usable"):
        photon.self_calibrate_stereo(frames[0], frames[1], cases.cameras(), cases.PLANE, rounds=1, **settings)
    _, report = photon.self_calibrate_stereo(frames[0], frames[1], cases.cameras(), cases.PLANE, rounds=1, passes=2, **settings)
    off = np.abs(np.array(report["sheet"]) - cases.SHEET)
    print(f"two passes at radius 4: sheet {np.round(report['sheet'], 5)}, {report['rounds'][0]['nodes']} nodes")
    assert off[0] <= 0.03 and off[1] <= 0.002 and off[2] <= 0.002
