"""Iterative image-deformation correlation, CPU tier: the f64 host models of include/parallel_ray_tracing.h section 7
(photon_amd/piv_deformation.py) against scipy's spline, analytic truth and piv_correlation's median test."""
import numpy as np
import pytest
from scipy import ndimage

import piv_deformation_cases as cs
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd


# ---- 1. coefficients and warp against scipy -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (2, 5), (7, 13), (33, 21), (65, 97)])
def test_coefficients_equal_scipy_mirror_spline_filter(shape):
    im = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape)
    want = ndimage.spline_filter(im, order=3, mode="mirror", output=np.float64)
    got = pd.bspline_coefficients_model(im)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(im).max()


@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.37, -0.81), (-5.25, 3.5), (14.9, -20.2)])
def test_constant_field_equals_scipy_map_coordinates(shift):
    shape, win, step = (67, 90), 16, 8
    im = np.random.default_rng(7).random(shape)
    field = np.zeros(pc.grid_shape(shape, win, step) + (2,)) + shift
    got = pd.deform_model(pd.bspline_coefficients_model(im), field, win, step, 1.0)
    r, q = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    want = ndimage.map_coordinates(im, [r + shift[1], q + shift[0]], order=3, mode="mirror")
    assert np.abs(got - want).max() <= 1e-12 * np.abs(im).max()


def test_scale_zero_returns_the_image():
    shape, win, step = (50, 41), 16, 16
    rng = np.random.default_rng(3)
    im = rng.random(shape)
    field = rng.uniform(-16, 16, pc.grid_shape(shape, win, step) + (2,))
    got = pd.deform_model(pd.bspline_coefficients_model(im), field, win, step, 0.0)
    assert np.abs(got - im).max() <= 1e-12 * np.abs(im).max()


def test_cubic_polynomial_is_shifted_exactly_away_from_the_borders():
    shape, win, step = (96, 96), 32, 16
    r, q = np.meshgrid(np.arange(96.0), np.arange(96.0), indexing="ij")

    def poly(y, x):
        y, x = (y - 48.0) / 48.0, (x - 48.0) / 48.0
        return 1.0 + 0.5 * x - 0.3 * y + x * y - 0.7 * x * x * y + 0.4 * y ** 3 + 0.9 * x ** 3

    dx, dy = 1.7, -2.4
    field = np.zeros(pc.grid_shape(shape, win, step) + (2,)) + (dx, dy)
    got = pd.deform_model(pd.bspline_coefficients_model(poly(r, q)), field, win, step, 1.0)
    inner = (slice(44, 52), slice(44, 52))          # the border's influence decays as 0.268^distance: 1e-25 at 44 pixels
    assert np.abs(got - poly(r + dy, q + dx))[inner].max() <= 1e-12


# ---- 2. the dense field ---------------------------------------------------------------------------------------------------
def test_dense_field_is_exact_at_the_centres_constant_beyond_and_linear_between():
    shape, win, step = (100, 131), 32, 12
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    rng = np.random.default_rng(11)
    field = rng.normal(size=(n_rows, n_cols, 2))
    field[2, 3] = (np.nan, 1.0)                     # reads as (0, 0)
    clean = np.where(np.isnan(field).any(axis=-1, keepdims=True), 0.0, field)
    # win is even, so the centres 7.5 + 8 i lie between pixels: the pixels 8 + 8 i and 9 + 8 i lie in the cell that starts
    # there, and the field is linear inside a cell, so 1.5 d[8 + 8 i] - 0.5 d[9 + 8 i] is its value at the centre
    win2, step2, shape2 = 16, 8, (65, 81)
    f2 = rng.normal(size=pc.grid_shape(shape2, win2, step2) + (2,))
    d2 = pd.dense_field(f2, shape2, win2, step2)
    n2r, n2c = f2.shape[0] - 1, f2.shape[1] - 1
    at_rows = 1.5 * d2[8::8][:n2r] - 0.5 * d2[9::8][:n2r]
    at_nodes = 1.5 * at_rows[:, 8::8][:, :n2c] - 0.5 * at_rows[:, 9::8][:, :n2c]
    np.testing.assert_allclose(at_nodes, f2[:-1, :-1], atol=1e-12)
    np.testing.assert_allclose(d2[-1, -1], f2[-1, -1], atol=1e-15)         # beyond the last centre: the last node itself

    d = pd.dense_field(field, shape, win, step)
    c = (win - 1) // 2                               # the last pixel before the first centre, the first after the last
    last_r, last_c = (n_rows - 1) * step + c + 1, (n_cols - 1) * step + c + 1
    assert (d[:c + 1] == d[c]).all() and (d[:, :c + 1] == d[:, c:c + 1]).all()
    assert (d[last_r:] == d[last_r]).all() and (d[:, last_c:] == d[:, last_c:last_c + 1]).all()
    np.testing.assert_allclose(d[0, 0], clean[0, 0], atol=1e-15)
    np.testing.assert_allclose(d[-1, -1], clean[-1, -1], atol=1e-15)

    rows, cols = pc.window_centres(shape, win, step)
    lin = np.stack([0.3 + 0.01 * cols - 0.02 * rows, -1.0 + 0.03 * rows], axis=-1)
    dl = pd.dense_field(lin, shape, win, step)
    r, q = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    inside = (slice(c + 1, last_r), slice(c + 1, last_c))
    want = np.stack([0.3 + 0.01 * q - 0.02 * r, -1.0 + 0.03 * r], axis=-1)
    np.testing.assert_allclose(dl[inside], want[inside], atol=1e-12)


def test_degenerate_grids():
    one_row = pd.dense_field(np.array([[[1.0, 2.0], [3.0, -2.0], [5.0, 0.0]]]), (16, 48), 16, 16)
    assert one_row.shape == (16, 48, 2) and (one_row == one_row[0]).all()
    np.testing.assert_allclose(one_row[0, 15], (1.9375, 0.125), atol=1e-15)         # (15 - 7.5) / 16 of the way from node 0 to node 1
    one_col = pd.dense_field(np.array([[[1.0, 2.0]], [[3.0, -2.0]]]), (32, 16), 16, 16)
    assert (one_col == one_col[:, :1]).all()
    single = pd.dense_field(np.array([[[4.0, -1.0]]]), (16, 16), 16, 16)
    assert (single == (4.0, -1.0)).all()
    with pytest.raises(ValueError):
        pd.dense_field(np.zeros((2, 2, 2)), (16, 48), 16, 16)


# ---- 3. validate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.validate_cases(), ids=lambda c: f"{c[0]}x{c[1]}{'_pred' if c[3] else ''}")
def test_validate_model_agrees_with_the_median_test_and_the_predictor(case):
    pred, vec, flags = cs.validate_case(*case)
    field, smooth, status, outliers, score = pd.validate_model(pred, vec, flags)
    total = (0.0 if pred is None else pred.astype(np.float64)) + vec[..., :2].astype(np.float64)
    total[(flags & pc.FLAG_FLAT) != 0] = np.nan
    total[~np.isfinite(total).all(axis=-1)] = np.nan
    want = pc.normalized_median_test(total)
    ok = cs.decided(score)
    assert np.array_equal(outliers[ok], want[ok])
    assert (~ok).mean() <= 1e-3
    # replaced values: the predictor's before its rounding
    good = np.where(outliers[..., None], np.nan, total)
    with np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        repl = np.nan_to_num(np.nanmedian(pc._neighbours(good), axis=0), nan=0.0)
    want_field = np.where(outliers[..., None], repl, total).astype(np.float32)
    assert field.dtype == np.float32 and np.array_equal(field, want_field)
    assert np.isfinite(field).all() and np.isfinite(smooth).all()
    assert np.array_equal(np.rint(field).astype(np.int32), pc.predictor(total, flags, outliers))
    assert np.array_equal(status, flags | np.where(outliers, 8, 0))
    assert outliers[(flags & pc.FLAG_FLAT) != 0].all() and outliers[~np.isfinite(vec[..., :2]).all(axis=-1)].all()


def test_near_threshold_exclusion_is_negligible():
    """Check 5's exclusion, shown with the model alone: 35 random grids from 2 x 2 to 127 x 127."""
    rng = np.random.default_rng(2024)
    scored = excluded = 0
    for k in range(35):
        r, c = (int(v) for v in rng.integers(2, 128, 2))
        pred, vec, flags = cs.validate_case(r, c, 500 + k, with_pred=bool(k % 2))
        score = pd.validate_model(pred, vec, flags)[4]
        scored += int(np.isfinite(score).sum())
        excluded += int((~cs.decided(score)).sum())
    assert scored > 50000 and excluded <= 1e-3 * scored, (scored, excluded)


def test_smoothing_preserves_a_constant_field_and_isolated_nodes_read_zero():
    vec = np.zeros((6, 9, 4), np.float32)
    vec[..., 0], vec[..., 1] = 1.3, -0.7
    flags = np.zeros((6, 9), np.int32)
    field, smooth, status, outliers, _ = pd.validate_model(None, vec, flags)
    assert not outliers.any() and (status == 0).all()
    assert np.array_equal(field, vec[..., :2]) and np.array_equal(smooth, vec[..., :2])
    # one surviving node among NaNs: no neighbours, so it is kept; the others have it as their only neighbour
    vec[...] = np.nan
    vec[2, 2, :2] = (4.0, 5.0)
    flags[0, 0] = pc.FLAG_FLAT
    field, _, status, outliers, _ = pd.validate_model(None, vec, flags)
    assert not outliers[2, 2] and outliers.sum() == 53 and status[0, 0] == (pc.FLAG_FLAT | 8)
    assert tuple(field[2, 2]) == (4.0, 5.0) and tuple(field[1, 1]) == (4.0, 5.0) and tuple(field[5, 8]) == (0.0, 0.0)
    with pytest.raises(ValueError):
        pd.validate_model(None, vec, flags, threshold=0.0)
    with pytest.raises(ValueError):
        pd.validate_model(None, vec, flags, eps=-1.0)


def test_an_injected_outlier_is_replaced_by_its_neighbours_median():
    pred = np.full((5, 5, 2), 1.0, np.float32)
    vec = np.zeros((5, 5, 4), np.float32)
    vec[..., 0] = 0.5
    vec[2, 2, :2] = (9.0, -9.0)
    field, smooth, status, outliers, _ = pd.validate_model(pred, vec, np.zeros((5, 5), np.int32))
    assert outliers.sum() == 1 and status[2, 2] == 8
    assert tuple(field[2, 2]) == (1.5, 1.0)
    assert abs(smooth[2, 2, 0] - 1.5) < 1e-6


# ---- 4. the driver's model on the prototype's pairs ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cs.SEEDS)
def test_model_on_a_vortex_pair(seed):
    """Measured with the model alone (seeds 1-5): two-pass RMS 1.126 / 0.903 / 0.551 / 0.472 / 1.837 px, after 3 iterations
    0.081 / 0.124 / 0.072 / 0.099 / 0.077 px (ratios 0.07 / 0.14 / 0.13 / 0.21 / 0.04), median peak 0.994."""
    im1, im2 = cs.pair("vortex", seed)
    base = cs.interior_rms(cs.two_pass(cs.model_correlate, im1, im2)[0], "vortex")
    vec, status = pd.correlate_deform_model(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=3)
    rms, peak = cs.interior_rms(vec, "vortex"), float(np.nanmedian(vec[1:-1, 1:-1, 2]))
    print(f"vortex seed {seed}: two-pass {base:.4f} px, 3 iterations {rms:.4f} px, ratio {rms / base:.3f}, median peak {peak:.3f}")
    assert rms <= 0.3 * base
    assert peak >= 0.95


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_model_on_a_uniform_pair(seed):
    """Measured with the model alone (seeds 1-5): two-pass RMS 0.034 / 0.035 / 0.035 / 0.040 / 0.037 px, after 3 iterations
    0.042 / 0.040 / 0.036 / 0.042 / 0.040 px (ratios 1.25 / 1.12 / 1.05 / 1.07 / 1.08)."""
    im1, im2 = cs.pair("uniform", seed)
    base = cs.interior_rms(cs.two_pass(cs.model_correlate, im1, im2)[0], "uniform")
    vec, _ = pd.correlate_deform_model(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=3)
    rms = cs.interior_rms(vec, "uniform")
    print(f"uniform seed {seed}: two-pass {base:.4f} px, 3 iterations {rms:.4f} px, ratio {rms / base:.3f}")
    assert rms <= 1.5 * base


def test_iterations_zero_is_pass_zero_plus_validation():
    im1, im2 = cs.pair("rotation", 1, shape=(96, 128))
    vec, status = pd.correlate_deform_model(im1, im2, 32, 16, 16, iterations=0)
    v0, f0 = pc.correlate_model(im1, im2, 32, 16, 16)
    field, _, st, _, _ = pd.validate_model(None, v0, f0)
    assert np.array_equal(vec[..., :2], field.astype(np.float64)) and np.array_equal(status, st)
    np.testing.assert_array_equal(vec[..., 2:], v0[..., 2:])
