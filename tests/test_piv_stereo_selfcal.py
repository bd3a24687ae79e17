"""Stereo self-calibration on the host (photon_amd/piv_stereo.py, section 19c): the triangulation model on disparities whose
world points are known, the sheet fit and the frame it defines, the moved cameras, and the model's rounds on SELFCAL_CASE --
the sheet found, the cameras corrected, and what that buys the three components.  No GPU."""
import numpy as np
import pytest

import piv_stereo_cases as base
import piv_stereo_selfcal_cases as cases
from photon_amd import piv_stereo as ps


def surface(X, Y):
    return 0.8 + 0.02 * X - 0.015 * Y


# ---- the triangulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(base.ANGLES))
def test_the_triangulation_returns_the_points_of_a_known_surface(kind):
    cams, pl = base.cameras(kind), cases.grid_plane("5x7")
    W, d = cases.surface_disparity(cams, pl, surface)
    out, flags = ps.triangulate_model(d, cams, pl, cases.WIN, cases.STEP, 4)
    assert out.shape == (5, 7, 6) and flags.dtype == np.int32 and not flags.any()
    print(f"{kind}: disparity up to {np.abs(d).max():.2f} px, points off by {np.abs(out[..., :3] - W).max():.2e} mm, error {out[..., 3].max():.2e} px, "
          f"last step {out[..., 4].max():.2e} mm, pivot ratio {out[..., 5].min():.3f}")
    assert np.abs(d[..., 0]).min() > 2.5                                           # the surface is 0.5 to 1.1 mm off: 2.7 to 6.3 px
    assert np.abs(out[..., :3] - W).max() <= 1e-9 and out[..., 3].max() < 1e-9 and out[..., 4].max() < 1e-10
    assert (out[..., 5] > 0.01).all()


def test_no_disparity_is_the_plane_itself():
    cams, pl = base.cameras("asymmetric"), cases.grid_plane("5x7")
    out, flags = ps.triangulate_model(np.zeros((5, 7, 2)), cams, pl, cases.WIN, cases.STEP, 4, flags=np.full((5, 7), 4))
    assert np.array_equal(out[..., :3], ps.window_centres(pl, cases.WIN, cases.STEP)) and (out[..., 3] == 0).all() and (out[..., 4] == 0).all()
    assert (flags == 4).all()


def test_one_iteration_is_the_first_gauss_newton_step():
    cams, pl = base.cameras("symmetric"), cases.grid_plane("5x7")
    W, d = cases.surface_disparity(cams, pl, surface)
    one = ps.triangulate_model(d, cams, pl, cases.WIN, cases.STEP, 1)[0]
    four = ps.triangulate_model(d, cams, pl, cases.WIN, cases.STEP, 4)[0]
    P = ps.window_centres(pl, cases.WIN, cases.STEP)
    assert np.allclose(np.linalg.norm(one[..., :3] - P, axis=-1), one[..., 4], rtol=1e-12)      # the step is W - P
    assert 1e-9 < np.abs(one[..., :3] - W).max() < 1e-2 and (four[..., 4] < 1e-6 * one[..., 4]).all()
    assert (four[..., 5] <= one[..., 5]).all()                                                  # the smallest ratio of the iterations


def test_flags_of_the_triangulation():
    cams, pl = base.cameras("symmetric"), cases.grid_plane("5x7")
    d = np.ones((5, 7, 2))
    d[2, 3, 0] = np.nan
    out, flags = ps.triangulate_model(d, cams, pl, cases.WIN, cases.STEP, 3)
    assert flags[2, 3] == ps.FLAG_NOT_FINITE and flags.sum() == ps.FLAG_NOT_FINITE
    assert np.isnan(out[2, 3, :5]).all() and out[2, 3, 5] > 0.01 and np.isfinite(out).sum() == 6 * 35 - 5
    start = ps.reconstruct_model(d, d, cams, pl, cases.WIN, cases.STEP)[0]
    assert out[2, 3, 5] == start[2, 3, 7]                                          # the ratio of the start point: the reconstruction's
    out, flags = ps.triangulate_model(np.ones((5, 7, 2)), (cams[0], cams[0]), pl, cases.WIN, cases.STEP, 3, flags=np.full((5, 7), 1))
    assert (flags == (1 | ps.FLAG_DEGENERATE)).all() and np.isnan(out[..., :5]).all() and not (out[..., 5] > ps.MIN_PIVOT_RATIO).any()
    for bad in (0, 17):
        with pytest.raises(ValueError, match="iterations"):
            ps.triangulate_model(d, cams, pl, cases.WIN, cases.STEP, bad)
    with pytest.raises(ValueError, match="grid"):
        ps.triangulate_model(d[:4], cams, pl, cases.WIN, cases.STEP, 2)


# ---- the sheet and its frame -------------------------------------------------------------------------------------------------
def _exact_points(pl=cases.PLANE, win=64, step=32):
    P = ps.window_centres(pl, win, step).copy()
    P[..., 2] = surface(P[..., 0], P[..., 1])
    return P


def test_fit_sheet_recovers_a_plane_and_ignores_outliers_and_flagged_nodes():
    P = _exact_points()
    flags = np.zeros(P.shape[:2], np.int32)
    flags[0, 0] = 4                                                                # informational: stays in
    sheet, rms, used = ps.fit_sheet(P, flags)
    assert np.allclose(sheet, (0.8, 0.02, -0.015), rtol=0, atol=1e-13) and rms < 1e-13 and used >= 10
    dirty = P.copy()
    dirty[1, 2, 2] += 0.5                                                          # an outlier the rejection must drop
    for k, bit in enumerate((1, 2, 16, 64, 128)):                                  # flagged nodes with wild values
        dirty[2, k, 2], flags[2, k] = 50.0 + k, bit
    dirty[3, 0, 2], error = 7.0, np.zeros(P.shape[:2])
    error[3, 0] = np.nan                                                           # no triangulation error: left out
    sheet, rms, used = ps.fit_sheet(dirty, flags, error)
    assert np.allclose(sheet, (0.8, 0.02, -0.015), rtol=0, atol=1e-13) and rms < 1e-13 and used <= 20 - 7
    flags[:] = 2
    flags[0, :5] = 0
    with pytest.raises(ValueError, match="at least 6"):
        ps.fit_sheet(P, flags)
    flags[:] = 2
    flags[:, 0] = 0
    flags[:3, 1] = 0
    assert ps.fit_sheet(P, flags)[2] == 7
    flags[:3, 1] = 2
    flags[:, 0] = 0
    column = np.concatenate([P[:, :1]] * 2, axis=0)                                # 8 nodes on one X
    with pytest.raises(ValueError, match="spread"):
        ps.fit_sheet(column, np.zeros(column.shape[:2], np.int32))


def test_sheet_frame_is_a_rotation_onto_the_sheet():
    pl = cases.PLANE
    R, O, C = ps.sheet_frame(cases.SHEET, pl)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    e3 = np.array([-0.02, 0.015, 1.0]) / np.linalg.norm([-0.02, 0.015, 1.0])
    e1 = np.array([1.0, 0.0, 0.0]) - e3[0] * e3
    assert np.allclose(R[:, 2], e3, rtol=0, atol=1e-15) and np.allclose(R[:, 0], e1 / np.linalg.norm(e1), rtol=0, atol=1e-15)
    assert np.allclose(R[:, 1], np.cross(R[:, 2], R[:, 0]), rtol=0, atol=1e-15) and R[0, 0] > 0.99 and R[1, 1] > 0.99
    assert np.allclose(C, [0.0, 0.0, 0.0]) and np.allclose(O, [0.0, 0.0, 0.8])
    W = ps.to_world((R, O, C), ps.plane_points(pl, [0, 80, 159], [0, 100, 191]))   # the plane's own points land on the sheet
    assert np.abs(W[..., 2] - surface(W[..., 0], W[..., 1])).max() < 1e-14
    assert np.allclose(ps.frame_sheet((R, O, C)), cases.SHEET, rtol=0, atol=1e-15)
    I, O0, C0 = ps.identity_frame(pl)
    assert np.array_equal(I, np.eye(3)) and np.array_equal(O0, C0)
    twice = ps.compose_frames((R, O, C), (R, O, C))
    P = np.array([[1.0, -2.0, 0.3]])
    assert np.allclose(ps.to_world(twice, P), ps.to_world((R, O, C), ps.to_world((R, O, C), P)), rtol=0, atol=1e-14)


def test_move_camera_keeps_the_camera_within_the_19_terms():
    pl, cams = cases.PLANE, cases.cameras()
    probe = ps.calibration_target(pl, 7, (-0.7, 0.2, 0.9))
    same, rms, worst = ps.move_camera(cams[0], *ps.identity_frame(pl), pl)
    assert np.abs(ps.map_points(same, probe) - ps.map_points(cams[0], probe)).max() <= 1e-9 and worst <= 1e-9
    frame = cases.true_frame()
    for cam in cams:
        moved, rms, worst = ps.move_camera(cam, *frame, pl)
        print(f"refit of the moved camera: rms {rms:.2e} px, max {worst:.2e} px")
        assert rms <= worst < 1e-6
        assert np.abs(ps.map_points(moved, probe) - ps.map_points(cam, ps.to_world(frame, probe))).max() < 1e-6


# ---- the rounds ----------------------------------------------------------------------------------------------------------------
def test_the_model_finds_the_sheet_and_corrects_the_cameras():
    """Measured: the sheet off by 0.0033 mm, 0.00001 and 0.0002; the corrected cameras within 0.020
    px of the true pinholes in the true sheet frame, the uncorrected ones 3.5 and 4.0 px off."""
    corrected, report = cases.model_result()
    for k, entry in enumerate(report["rounds"]):
        print(f"round {k + 1}: disparity rms {entry['disparity_rms']:.3f} px, sheet {np.round(entry['sheet'], 5)}, sheet rms {entry['sheet_rms']:.4f} mm, "
              f"{entry['nodes']} nodes, error median {entry['error_median']:.4f} px, last step {entry['step_max']:.1e} mm, refit max "
              f"{max(r[1] for r in entry['refit']):.1e} px")
    off = np.abs(np.array(report["sheet"]) - cases.SHEET)
    after, before = cases.camera_errors(corrected), cases.camera_errors(cases.cameras())
    print(f"sheet {np.round(report['sheet'], 5)} (off by {off.round(5)}), cameras within {max(after):.4f} px (before: {max(before):.2f} px)")
    assert off[0] <= 0.03 and off[1] <= 0.002 and off[2] <= 0.002
    assert 1 <= len(report["rounds"]) <= 3 and report["rounds"][-1]["disparity_rms"] < 0.05 < report["rounds"][0]["disparity_rms"]
    assert max(after) <= 0.05 and min(before) > 1.0
    assert all(max(r[1] for r in entry["refit"]) < 1e-6 and entry["step_max"] < 1e-10 for entry in report["rounds"])
    R = report["R"]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.allclose(report["C"], cases.true_frame()[2])


def test_the_corrected_cameras_measure_the_third_component():
    """The point of it all, on the model chain: rms dZ with the corrected cameras at most half of what the original cameras
    give and at most 1.25 x the aligned sheet's; dX and dY not worse by more than 1.25 x.  Measured:
    dZ 0.212 px uncorrected, 0.043 px corrected (ratio 0.21), 0.045 px on the aligned sheet."""
    (before, res0), (after, res1), (aligned, res2) = cases.model_evaluation()
    print(f"rms dX dY dZ: uncorrected {before.round(4)} px, corrected {after.round(4)} px, aligned sheet {aligned.round(4)} px; "
          f"median residual {res0:.4f}, {res1:.4f}, {res2:.4f} px")
    assert after[2] <= 0.5 * before[2] and after[2] <= 1.25 * aligned[2]
    assert after[0] <= 1.25 * before[0] and after[1] <= 1.25 * before[1]
