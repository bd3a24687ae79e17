"""Window weighting in the direct correlator on the host models (CPU tier): photon_amd/piv_weighting.py and the weighting=
keyword of the drivers' models (include/parallel_ray_tracing.h, section 18)."""
import numpy as np
import pytest

import piv_weighting_cases as cases
import test_piv_correlation_gpu as base
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_multigrid as pm
from photon_amd import piv_weighting as pw

ONE_PER_WIN = [base.CASES[1], base.CASES[4], base.CASES[8]]         # (16, 4) and (32, 8) and (64, 16), all with offsets


def pair_of(case):
    win, R, step, shape, shift, with_off = case
    im1, im2 = base.particle_pair(shape, shift, seed=win * 100 + R + step)
    off = np.random.default_rng(R).integers(-3, 4, size=pc.grid_shape(shape, win, step) + (2,)).astype(np.int32) if with_off else None
    return im1, im2, off


@pytest.mark.parametrize("case", ONE_PER_WIN, ids=[f"w{c[0]}" for c in ONE_PER_WIN])
def test_uniform_weights_are_the_unweighted_model_exactly(case):
    win, R, step = case[:3]
    im1, im2, off = pair_of(case)
    want = pc.correlate_model(im1, im2, win, step, R, offset=off, planes=True)
    got = pw.correlate_weighted_model(im1, im2, pw.window_weights(win, "uniform"), win, step, R, offset=off, planes=True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("case", ONE_PER_WIN, ids=[f"w{c[0]}" for c in ONE_PER_WIN])
def test_the_scale_of_the_table_does_not_matter(case):
    win, R, step = case[:3]
    im1, im2, off = pair_of(case)
    table = cases.asymmetric(win)
    a = pw.correlate_weighted_model(im1, im2, table, win, step, R, offset=off, planes=True)
    b = pw.correlate_weighted_model(im1, im2, 4.0 * table.astype(np.float64), win, step, R, offset=off, planes=True)
    assert np.array_equal(a[1], b[1])
    live = (a[1] & pc.FLAG_FLAT) == 0
    assert np.abs(a[0][live][:, :3] - b[0][live][:, :3]).max() <= 1e-12
    assert np.abs(a[2][live] - b[2][live]).max() <= 1e-12


@pytest.mark.parametrize("win", pc.WINDOW_SIZES)
def test_window_weights_symmetries(win):
    g = pw.window_weights(win)
    assert g.dtype == np.float32 and g.shape == (win, win)
    assert np.array_equal(g, g.T) and np.array_equal(g, g[::-1]) and np.array_equal(g, g[:, ::-1])
    assert g.max() == g[win // 2, win // 2] == g[win // 2 - 1, win // 2 - 1] < 1.0 and g.min() == g[0, 0] > 0.0
    assert np.array_equal(g, pw.window_weights(win, "gaussian", win / 4.0))
    c = np.arange(win) - (win - 1) / 2.0                       # separable up to the one rounding
    np.testing.assert_allclose(g, np.outer(np.exp(-c * c / (2 * (win / 4.0) ** 2)), np.exp(-c * c / (2 * (win / 4.0) ** 2))), rtol=1e-6)
    wide = pw.window_weights(win, "gaussian", 1e4)
    assert (wide <= 1.0).all() and wide.min() > 0.999
    assert np.array_equal(pw.window_weights(win, "uniform"), np.ones((win, win), np.float32))


def test_check_weights_and_resolve_refusals():
    good = cases.asymmetric(16)
    assert np.array_equal(pw.check_weights(good.astype(np.float64), 16), good) and pw.check_weights(good, 16).dtype == np.float32
    for bad, what in ((good[:-1], "shape"), (good.ravel(), "shape"), (np.where(good == good[3, 3], np.nan, good), "not finite"),
                      (np.where(good == good[3, 3], np.inf, good), "not finite"), (-good, "negative"), (0.0 * good, "above 0")):
        with pytest.raises(ValueError, match=what):
            pw.check_weights(bad, 16)
    with pytest.raises(ValueError, match="win must be"):
        pw.check_weights(np.ones((24, 24)), 24)
    assert pw.resolve(None, 32) is None
    assert np.array_equal(pw.resolve("gaussian", 32), pw.window_weights(32, "gaussian", 8.0))
    assert np.array_equal(pw.resolve(("gaussian", 5.0), 32), pw.window_weights(32, "gaussian", 5.0))
    assert np.array_equal(pw.resolve(good, 16), good)
    with pytest.raises(ValueError, match="shape"):
        pw.resolve(good, 32)
    with pytest.raises(ValueError, match="kind must be"):
        pw.resolve("hann", 32)
    for sigma in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="sigma must be"):
            pw.resolve(("gaussian", sigma), 32)
    with pytest.raises(ValueError, match="win must be"):
        pw.window_weights(48)


def test_weighting_with_phase_or_a_mask_is_refused_by_the_models():
    im1, im2 = cases.driver_pair()
    mask = np.zeros(im1.shape, bool)
    for kw, what in ((dict(method="phase"), "window_sigma"), (dict(mask=mask), "mask")):
        with pytest.raises(ValueError, match=what):
            pd.model_correlator(kw.get("method", "direct"), 32, None, None, 2.5, kw.get("mask"), 0.5, "gaussian")
        with pytest.raises(ValueError, match=what):
            pd.correlate_deform_model(im1, im2, **cases.DEFORM, weighting="gaussian", **kw)
        with pytest.raises(ValueError, match=what):
            pm.correlate_multigrid_model(im1, im2, **cases.MULTIGRID, weighting="gaussian", **kw)
    with pytest.raises(ValueError, match="shape"):               # an array has one win: the second level has another
        pm.correlate_multigrid_model(im1, im2, **cases.MULTIGRID, weighting=cases.asymmetric(32))


def test_a_window_whose_varying_pixels_have_no_weight_is_flat():
    im1, im2, table = cases.flat_by_weight()
    vec, flags, planes = pw.correlate_weighted_model(im1, im2, table, 16, 16, 4, planes=True)
    assert (flags & ~pc.FLAG_EDGE_PEAK).tolist() == [[pc.FLAG_FLAT | pc.FLAG_OUTSIDE, pc.FLAG_OUTSIDE]]      # (noise: the peak may sit on the edge)
    assert np.isnan(vec[0, 0]).all() and np.isnan(planes[0, 0]).all() and np.isfinite(vec[0, 1]).all()
    _, plain = pc.correlate_model(im1, im2, 16, 16, 4)             # without the table the window is alive
    assert (plain & ~pc.FLAG_EDGE_PEAK).tolist() == [[pc.FLAG_OUTSIDE, pc.FLAG_OUTSIDE]]
    vec, flags = pw.correlate_weighted_model(im1, im2, table, 16, 16, 4, offset=np.array([[[0, 0], [40, 0]]]))
    assert flags[0, 1] == pc.FLAG_FLAT | pc.FLAG_OUTSIDE           # no pixel of b at zero shift lies in the image


@pytest.mark.parametrize("where", [(0, 0), (7, 9), (15, 15)])
def test_a_single_positive_weight_is_flat(where):
    im1, im2, _ = cases.flat_by_weight()
    for table in (cases.single(16, *where), np.zeros((16, 16), np.float32), np.full((16, 16), -1.0), np.full((16, 16), np.nan)):
        vec, flags = pw.correlate_weighted_model(im1, im2, table, 16, 16, 4)
        assert ((flags & pc.FLAG_FLAT) != 0).all() and np.isnan(vec).all()


def test_entries_that_are_not_above_zero_read_as_zero():
    im1, im2, off = pair_of(base.CASES[1])
    table = cases.holed(16)
    clean = np.where(table > 0, table, 0.0)
    a = pw.correlate_weighted_model(im1, im2, table, 16, 16, 4, offset=off, planes=True)
    b = pw.correlate_weighted_model(im1, im2, clean, 16, 16, 4, offset=off, planes=True)
    assert np.isfinite(a[0]).all()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_the_response_to_wavelengths_near_the_window_size():
    """Frames 160 x 256, dy = 1 px sin(2 pi x / lambda), win 32, step 8, six iterations without smoothing.  A top hat answers
    lambda = 24 with sinc(32 / 24) = -0.21 and the loop drives it further down; the Gaussian window (sigma = win / 4) stays
    positive.  The models measure -0.23 -> -0.58 against +0.14 -> +0.30 (seed 1) and, at lambda = 40, 0.29 against 0.59 on
    the first pass."""
    for seed in (1, 2):
        uniform = {lam: cases.model_response(lam, seed, None) for lam in cases.WAVELENGTHS}
        gaussian = {lam: cases.model_response(lam, seed, "gaussian") for lam in cases.WAVELENGTHS}
        for lam in cases.WAVELENGTHS:
            print(f"seed {seed}, lambda {lam}: uniform {uniform[lam][0]:+.3f} -> {uniform[lam][-1]:+.3f}, "
                  f"gaussian {gaussian[lam][0]:+.3f} -> {gaussian[lam][-1]:+.3f}")
        cases.assert_response(uniform, gaussian)
