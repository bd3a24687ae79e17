"""Displacement uncertainty from correlation statistics, CPU tier: the f64 model of photon_piv_uncertainty
(photon_amd/piv_uncertainty.py: its symmetries, its branches on the device's cases, its calibration against pairs with a
known displacement) and the glue that carries sigma into weights and through the integral (photon_amd/bos_density.py)."""
import numpy as np
import pytest

import piv_uncertainty_cases as uc
from photon_amd import bos_density as bd
from photon_amd import piv_correlation as pc
from photon_amd import piv_uncertainty as pu


def test_identical_frames_give_zero_sigma():
    im = uc.matched_pair((97, 130))[0]
    for reach in uc.REACHES:
        sigma, flags, stats, T = pu.uncertainty_model(im, im, 32, 16, reach)
        assert (stats[..., 2:] == 0.0).all()                # d = 0 exactly: IEEE multiplication commutes
        assert (sigma == 0.0).all() and (flags == 0).all()


@pytest.mark.parametrize("case", uc.CASES[5:10] + uc.CASES[20:25], ids=uc.case_id)
def test_swapping_the_frames_returns_identical_bits(case):
    shape, win, step, reach = case
    im1, im2 = uc.matched_pair(shape)
    for got, want in zip(pu.uncertainty_model(im2, im1, win, step, reach), uc.model(case)):
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", uc.CASES[15:25], ids=uc.case_id)
def test_transposing_the_images_swaps_the_axes(case):
    shape, win, step, reach = case
    im1, im2 = uc.matched_pair(shape)
    sigma, flags, stats, _ = uc.model(case)
    st, ft, tt, _ = pu.uncertainty_model(im1.T, im2.T, win, step, reach)
    assert np.array_equal(ft.T, flags)
    np.testing.assert_allclose(np.swapaxes(st, 0, 1)[..., ::-1], sigma, rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.swapaxes(tt, 0, 1)[..., ::-1, :], stats, rtol=1e-12, atol=0)


@pytest.mark.parametrize("which", [0, 1])
def test_a_constant_window_in_either_frame_is_flat(which):
    ims = [im.copy() for im in uc.matched_pair((64, 64))]
    ims[which][8:24, 16:32] = 0.37                          # window (1, 2) of the 16 / 8 grid, and only that one
    sigma, flags, stats, _ = pu.uncertainty_model(*ims, 16, 8, 2)
    assert flags[1, 2] == pu.FLAG_FLAT == pc.FLAG_FLAT
    assert np.isnan(sigma[1, 2]).all() and np.isnan(stats[1, 2]).all()
    rest = np.ones(flags.shape, bool)
    rest[1, 2] = False
    assert np.isfinite(sigma[rest]).all() and not (flags[rest] & pu.FLAG_FLAT).any()


def test_refused_arguments():
    im = uc.matched_pair((64, 64))[0]
    for win, step, reach in ((24, 8, 2), (32, 0, 2), (32, 8, -1), (32, 8, 5)):
        with pytest.raises(ValueError):
            pu.uncertainty_model(im, im, win, step, reach)
    with pytest.raises(ValueError):
        pu.uncertainty_model(im[:20], im[:20], 32, 8, 2)


@pytest.mark.parametrize("case", uc.CASES, ids=uc.case_id)
def test_no_case_sits_on_a_branch(case):
    """|V| >= 1e-8 T and den >= 1e-3 on every window: a branch the device takes differently is a bug, not rounding.  The
    fallback of a negative V is exercised without contrived input."""
    sigma, flags, stats, T = uc.model(case)
    C0, C1, S00, V = (stats[..., k] for k in range(4))
    assert (np.abs(V) >= 1e-8 * T).all()
    s = np.sqrt(np.where(V < 0, S00, V))
    lo, hi = C1 - s / 2, C1 + s / 2
    assert (lo > 0).all() and (C0 > 0).all()
    den = 4 * np.log(C0) - 2 * np.log(lo) - 2 * np.log(hi)
    assert den.min() >= 1e-3
    assert np.array_equal(flags, np.where((V < 0).any(axis=-1), pu.FLAG_NEGATIVE_VARIANCE, 0))
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    s2, f2 = pu.sigma_from_stats(stats)
    assert s2.tobytes() == sigma.tobytes() and np.array_equal(f2, flags)


@pytest.mark.parametrize("case", uc.CASES, ids=uc.case_id)
def test_the_sign_of_V_does_not_hang_on_rounding(case):
    """The device's flags must equal the model's exactly, and bit 32 is the sign of V.  The device's V is held to the model's
    within 1e-11 N T (test_piv_uncertainty_gpu.SUM_RTOL): every |V| lies 10^4 times further from zero, on either axis."""
    _, _, stats, T = uc.model(case)
    margin = np.abs(stats[..., 3]) / (uc.n_terms(case[3]) * T)            # [n_rows, n_cols, axis]
    print(f"{uc.case_id(case)}: smallest |V| / (N T) = {margin.min():.2e}")
    assert margin.min() >= 1e-7


def test_negative_variances_occur_naturally():
    count = {uc.case_id(c): int((uc.model(c)[1] & pu.FLAG_NEGATIVE_VARIANCE).astype(bool).sum()) for c in uc.CASES}
    assert count["130x97-win16-step5-K2"] == 4 and count["130x97-win16-step5-K4"] == 24
    assert count["64x64-win16-step8-K4"] == 4 and count["256x256-win32-step16-K4"] == 1


def test_parabolic_branch_and_missing_peak():
    # lo <= 0: the parabolic fit; den <= 0: no maximum at zero shift
    stats = np.array([[[4.0, 1.0, 16.0, 16.0], [4.0, 5.0, 1.0, 1.0]], [[4.0, 1.0, 1.0, -3.0], [np.nan] * 4]])
    sigma, flags = pu.sigma_from_stats(stats)
    assert sigma[0, 0] == 4.0 / (4 * 3.0) and np.isnan(sigma[0, 1]) and flags[0] == pu.FLAG_NO_PEAK
    assert flags[1] == pu.FLAG_FLAT and np.isnan(sigma[1]).all()
    one = pu.sigma_from_stats(np.array([[4.0, 1.0, 1.0, -3.0], [4.0, 1.0, 1.0, 1.0]]))
    assert one[1] == pu.FLAG_NEGATIVE_VARIANCE and one[0][0] == one[0][1]


# ---- calibration against pairs with a known displacement ---------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.05, 0.10])
def test_sigma_is_calibrated_on_uniform_pairs(noise):
    ratio, cover, rms = uc.model_calibration("uniform", noise)
    print(f"uniform, noise {noise}: rms sigma / std(error) = {ratio[0]:.3f} (x) {ratio[1]:.3f} (y); |error| <= sigma on "
          f"{100 * cover[0]:.0f} % / {100 * cover[1]:.0f} % of the nodes; rms sigma {rms:.4f} px")
    assert (ratio >= uc.CAL_BOUND[0]).all() and (ratio <= uc.CAL_BOUND[1]).all(), ratio


def test_sigma_grows_with_the_image_noise():
    low, high = uc.model_calibration("uniform", 0.02)[2], uc.model_calibration("uniform", 0.10)[2]
    print(f"rms sigma {low:.4f} px at noise 0.02, {high:.4f} px at noise 0.10: {high / low:.1f} x")
    assert high >= 2.0 * low


# ---- weights -------------------------------------------------------------------------------------------------------------
def weight_case():
    rng = np.random.default_rng(21)
    sigma = rng.lognormal(np.log(0.05), 0.8, (12, 15, 2))
    flags = np.zeros((12, 15), np.int32)
    outliers = rng.random((12, 15)) < 0.1
    flags[3, 4] = flags[7, 7] = pc.FLAG_FLAT
    flags[5, 5] = pc.FLAG_EDGE_PEAK                         # no reason for a zero
    sigma[2, 9, 1] = np.nan
    sigma[8, 1, 0] = np.inf
    sigma[0, 0] = 1e-9                                      # far below the floor
    return sigma, flags, outliers


def test_weights_from_uncertainty():
    sigma, flags, outliers = weight_case()
    outliers[0, 0] = False
    for floor in (0.25, 0.5):
        w = bd.weights_from_uncertainty(sigma, flags, outliers, floor=floor)
        zero = outliers | ((flags & pc.FLAG_FLAT) != 0) | ~np.isfinite(sigma).all(axis=-1)
        assert np.array_equal(w == 0, zero) and zero.sum() > 4 and not zero[5, 5]
        assert np.isclose(np.median(w[~zero]), 1.0, rtol=1e-12)
        assert w.max() <= 1 / floor ** 2 * (1 + 1e-12) and w[0, 0] == w.max() and np.isclose(w[0, 0], 1 / floor ** 2, rtol=1e-12)
        s2 = (sigma ** 2).sum(axis=-1)
        free = ~zero & (w < 0.99 / floor ** 2)
        np.testing.assert_allclose(w[free] * s2[free], np.median(s2[~zero]), rtol=1e-12)
    with pytest.raises(ValueError):
        bd.weights_from_uncertainty(sigma, flags, outliers, floor=0.0)


def test_equal_sigma_reproduces_weights_from_correlation():
    sigma, flags, outliers = weight_case()
    vectors = np.where(np.isfinite(sigma), 1.5, np.nan)
    equal = np.where(np.isfinite(sigma), 0.07, sigma)
    assert np.array_equal(bd.weights_from_uncertainty(equal, flags, outliers), bd.weights_from_correlation(vectors, flags, outliers))
    assert (bd.weights_from_uncertainty(np.full((3, 3, 2), np.nan), np.zeros((3, 3), int), np.zeros((3, 3), bool)) == 0).all()


def test_gradient_uncertainty_follows_the_gradients_map():
    sigma = np.random.default_rng(2).uniform(0.01, 0.2, (5, 6, 2))
    for diffraction in (False, True):
        cam = {"implement_diffraction": diffraction}
        sgx, sgy = bd.gradient_uncertainty(sigma, cam, 3.5)
        gx, gy = bd.gradients_from_displacements(sigma, cam, 3.5)
        assert np.array_equal(sgx, np.abs(gx)) and np.array_equal(sgy, np.abs(gy))
        assert np.array_equal(bd.gradient_uncertainty(sigma, cam, -3.5)[0], sgx)


def test_projected_density_uncertainty_equals_the_columns_of_solve_direct():
    """J column by column: solve_direct on unit gradients (fixed values 0, so phi is linear in g)."""
    rng = np.random.default_rng(33)
    ny, nx = 7, 6
    w = rng.uniform(0.2, 3.0, (ny, nx))
    w[3, 2] = 0.0
    sgx, sgy = rng.uniform(0.5, 2.0, (2, ny, nx))
    hx, hy = 0.7, 1.3
    got = bd.projected_density_uncertainty(sgx, sgy, w, None, hx, hy)
    var = np.zeros((ny, nx))
    zero = np.zeros((ny, nx))
    for j in range(ny * nx):
        unit = np.zeros(ny * nx)
        unit[j] = 1.0
        unit = unit.reshape(ny, nx)
        var += np.nan_to_num(bd.solve_direct(unit, zero, w, None, None, hx, hy)) ** 2 * sgx.ravel()[j] ** 2
        var += np.nan_to_num(bd.solve_direct(zero, unit, w, None, None, hx, hy)) ** 2 * sgy.ravel()[j] ** 2
    phi = bd.solve_direct(sgx, sgy, w, None, None, hx, hy)
    assert np.array_equal(np.isnan(got), np.isnan(phi)) and np.isnan(got[3, 2])
    frame = np.ones((ny, nx), bool)
    frame[1:-1, 1:-1] = False
    assert (got[frame] == 0).all()
    inner = ~frame & np.isfinite(got)
    assert inner.sum() == 19 and (got[inner] > 0).all()
    np.testing.assert_allclose(got[inner] ** 2, var[inner], rtol=1e-10, atol=0)


def test_uncertainty_weights_need_sigma():
    from photon_amd import scenes
    call = scenes.bos_scene(n_dots=4, points_per_dot=2, rays_per_source=4, n_pixels=64)
    vec = np.zeros((3, 3, 4))
    vec[..., 0] = 0.5
    flags = np.zeros((3, 3), np.int32)
    args = (vec, flags, (64, 64), call, 300000.0, 66300.0, 32, 16)
    with pytest.raises(ValueError):
        bd.measured_gradients(*args, weights="uncertainty")
    with pytest.raises(ValueError):
        bd.measured_gradients(*args, weights="sigma")
    sigma = np.full((3, 3, 2), 0.05)
    sigma[1, 1] = 0.1
    w = bd.measured_gradients(*args, weights="uncertainty", sigma=sigma)[2]
    assert w[1, 1] == 0.25 and (np.delete(w.ravel(), 4) == 1.0).all()
    assert np.array_equal(bd.measured_gradients(*args, weights="median")[2], np.ones((3, 3)))
