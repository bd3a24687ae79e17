"""The host model of photon_piv_correlate (photon_amd/piv_correlation.py; definition: include/parallel_ray_tracing.h,
section 5) on constructed cases, the median test and the predictor.  CPU only."""
import numpy as np
import pytest

from photon_amd import piv_correlation as pc


def particles(shape, per_window, win, rng, margin=0.0):
    h, w = shape
    n = int(round(per_window * h * w / (win * win)))
    return rng.uniform(-margin, w + margin, n), rng.uniform(-margin, h + margin, n)


@pytest.mark.parametrize("shift", [(3, 0), (-2, 0), (0, 4), (0, -5), (2, -3), (-4, 1)])
def test_exact_integer_shifts_and_the_sign_convention(shift):
    """im2(p + d) = im1(p): a pattern moved right (columns) and down (rows) gives positive dx, dy."""
    sx, sy = shift
    rng = np.random.default_rng(7)
    x, y = particles((96, 128), 12, 16, rng, margin=8)
    im1 = pc.particle_image((96, 128), x, y)
    im2 = pc.particle_image((96, 128), x + sx, y + sy)
    vec, flags = pc.correlate_model(im1, im2, 16, 8, 6)
    inner = flags == 0
    assert inner.sum() >= 40
    hit = (np.rint(vec[inner, 0]) == sx) & (np.rint(vec[inner, 1]) == sy)
    assert hit.mean() >= 0.95
    assert np.abs(np.median(vec[inner, :2], axis=0) - [sx, sy]).max() < 0.02
    # a rolled copy (the same pixels, moved): the integer shift on the interior windows
    im2 = np.roll(im1, (sy, sx), axis=(0, 1))
    vec, flags = pc.correlate_model(im1, im2, 16, 8, 6)
    inner = (flags & pc.FLAG_OUTSIDE) == 0
    hit = (np.rint(vec[inner, 0]) == sx) & (np.rint(vec[inner, 1]) == sy)
    assert hit.mean() >= 0.98


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("s", [0.0, 0.25, 0.5, 1.3, -3.7, 5.5])
def test_subpixel_shifts_of_ideal_particle_images(s, axis):
    """>= 400 windows of 32 px on erf-integrated Gaussian particles (2.5 px, ~15 per window, uniform shift, no noise):
    mean bias <= 0.03 px, RMS error <= 0.08 px in the shifted axis, and the other axis stays at 0."""
    win, n_win = 32, 22
    shape = (win * n_win, win * n_win)
    rng = np.random.default_rng(11 + abs(int(10 * s)) + 100 * (axis == "y") + 1000 * (s < 0))
    x, y = particles(shape, 15, win, rng, margin=10)
    d = np.array([s, 0.0] if axis == "x" else [0.0, s])
    im1 = pc.particle_image(shape, x, y)
    im2 = pc.particle_image(shape, x + d[0], y + d[1])
    vec, flags = pc.correlate_model(im1, im2, win, win, 8)
    ok = flags == 0
    assert ok.sum() >= 400
    err = vec[ok, :2] - d
    k = 0 if axis == "x" else 1
    bias, rms = err[:, k].mean(), np.sqrt((err[:, k] ** 2).mean())
    assert abs(bias) <= 0.03 and rms <= 0.08, (bias, rms)
    assert np.sqrt((err[:, 1 - k] ** 2).mean()) <= 0.08


def test_grid_formula_and_centres():
    im = np.random.default_rng(1).random((70, 90))
    for win, step in ((16, 12), (16, 16), (32, 5), (64, 7)):
        if win > 70:
            continue
        vec, flags = pc.correlate_model(im, im, win, step, 1)
        n_rows, n_cols = (70 - win) // step + 1, (90 - win) // step + 1
        assert vec.shape == (n_rows, n_cols, 4) and flags.shape == (n_rows, n_cols)
        assert pc.grid_shape(im.shape, win, step) == (n_rows, n_cols)
        r, c = pc.window_centres(im.shape, win, step)
        assert r.shape == c.shape == (n_rows, n_cols) and r[0, 0] == c[0, 0] == (win - 1) / 2
        assert r[-1, 0] == (n_rows - 1) * step + (win - 1) / 2 and c[0, -1] == (n_cols - 1) * step + (win - 1) / 2
    with pytest.raises(ValueError):
        pc.correlate_model(im[:15], im[:15], 16, 8, 4)


def test_border_peak_flag_and_no_fit_in_that_axis():
    """One bright pixel in the middle of window (1, 1) of im1, one in im2 at the shift (4, -1): with R = 4 the peak lies on
    the search square's edge in x -- flag 1, delta_x 0 -- and inside it in y, where its equal neighbours give delta_y 0."""
    im1 = np.zeros((48, 48))
    im2 = np.zeros((48, 48))
    im1[24, 24] = 1.0
    im2[24 - 1, 24 + 4] = 1.0
    vec, flags = pc.correlate_model(im1, im2, 16, 16, 4)
    assert flags[1, 1] == pc.FLAG_EDGE_PEAK
    assert (vec[1, 1, 0], vec[1, 1, 1]) == (4.0, -1.0)
    im2 = np.zeros((48, 48))
    im2[24 - 4, 24 + 2] = 1.0                                   # the edge in y only
    vec, flags = pc.correlate_model(im1, im2, 16, 16, 4)
    assert flags[1, 1] == pc.FLAG_EDGE_PEAK and (vec[1, 1, 0], vec[1, 1, 1]) == (2.0, -4.0)
    im2 = np.zeros((48, 48))
    im2[24 + 3, 24 - 3] = 1.0                                   # inside: no flag
    vec, flags = pc.correlate_model(im1, im2, 16, 16, 4)
    assert flags[1, 1] == 0 and (vec[1, 1, 0], vec[1, 1, 1]) == (-3.0, 3.0)


def test_flat_window_is_flagged_and_nan():
    rng = np.random.default_rng(4)
    im1 = rng.random((48, 48))
    im2 = rng.random((48, 48))
    im1[:16, :16] = 0.5                                         # window (0, 0) of im1: constant
    im2[16:32, 32:48] = 0.0                                     # window (1, 2) at zero shift: constant in im2
    vec, flags, planes = pc.correlate_model(im1, im2, 16, 16, 2, planes=True)
    for i, j in ((0, 0), (1, 2)):
        assert flags[i, j] & pc.FLAG_FLAT
        assert np.isnan(vec[i, j]).all() and np.isnan(planes[i, j]).all()
    assert flags[1, 1] == 0 or flags[1, 1] == pc.FLAG_EDGE_PEAK
    assert np.isfinite(vec[1, 1]).all()
    assert flags[0, 0] == pc.FLAG_FLAT | pc.FLAG_OUTSIDE        # (0, 0) also needs pixels outside the image


def test_outside_flag_follows_the_search_region_and_the_offset():
    im = np.random.default_rng(5).random((64, 64))
    _, flags = pc.correlate_model(im, im, 16, 16, 4)
    want = np.ones((4, 4), bool)
    want[1:3, 1:3] = False                                      # only the middle windows keep [-4, 4] inside
    assert np.array_equal((flags & pc.FLAG_OUTSIDE) != 0, want)
    off = np.zeros((4, 4, 2), np.int32)
    off[1, 1] = (-13, 0)                                        # window (1, 1) moved 13 columns left: out on the left
    _, flags2 = pc.correlate_model(im, im, 16, 16, 4, offset=off)
    assert flags2[1, 1] & pc.FLAG_OUTSIDE and not flags2[1, 2] & pc.FLAG_OUTSIDE
    # a pixel outside reads as the window's mean at zero shift: window (0, 0) of a 32 x 32 pair (it needs rows and columns
    # -3 .. 18) has the plane of the same window inside the pair padded by 3 pixels, im2's padding set to that mean
    rng = np.random.default_rng(6)
    im1, im2 = rng.random((32, 32)), rng.random((32, 32))
    _, flags, planes = pc.correlate_model(im1, im2, 16, 16, 3, planes=True)
    big1 = np.zeros((38, 38))
    big1[3:35, 3:35] = im1
    big2 = np.full((38, 38), im2[:16, :16].mean())
    big2[3:35, 3:35] = im2
    _, flags_big, planes_big = pc.correlate_model(big1, big2, 16, 3, 3, planes=True)      # window (1, 1) starts at (3, 3)
    assert flags[0, 0] & pc.FLAG_OUTSIDE and not flags_big[1, 1] & pc.FLAG_OUTSIDE
    np.testing.assert_allclose(planes[0, 0], planes_big[1, 1], rtol=1e-12, atol=1e-12)


def test_tie_rule_and_ratio():
    """im1: one bright pixel in the middle of a 16 x 16 window; im2: two equal bright pixels at shifts (sx, sy) = (1, -2)
    and (-2, 1) from it.  Every value is a dyadic fraction, so the two correlation values tie exactly: the peak is the
    first in row-major order (sy, then sx), i.e. (1, -2), with delta 0 (equal neighbours), and the ratio is exactly 1."""
    im1 = np.zeros((48, 48))
    im2 = np.zeros((48, 48))
    im1[24, 24] = 1.0
    im2[24 - 2, 24 + 1] = 1.0
    im2[24 + 1, 24 - 2] = 1.0
    vec, flags, planes = pc.correlate_model(im1, im2, 16, 16, 4, planes=True)
    v, p = vec[1, 1], planes[1, 1]
    assert flags[1, 1] == 0
    assert p[4 - 2, 4 + 1] == p[4 + 1, 4 - 2] == p.max()
    assert (v[0], v[1]) == (1.0, -2.0)
    assert v[3] == 1.0
    assert v[2] == p.max()


def test_ratio_is_the_peak_over_the_largest_value_two_shifts_away():
    rng = np.random.default_rng(8)
    x, y = particles((64, 64), 10, 16, rng, margin=6)
    im1 = pc.particle_image((64, 64), x, y)
    im2 = pc.particle_image((64, 64), x + 1.2, y + 0.4) + 0.05 * rng.random((64, 64))
    vec, flags, planes = pc.correlate_model(im1, im2, 16, 8, 5, planes=True)
    for i, j in np.ndindex(flags.shape):
        p = planes[i, j]
        py, px = np.unravel_index(np.argmax(p), p.shape)
        sy, sx = np.meshgrid(np.arange(11), np.arange(11), indexing="ij")
        far = np.maximum(abs(sy - py), abs(sx - px)) >= 2
        m = p[far].max()
        want = p[py, px] / m if m > 0 else np.inf
        assert vec[i, j, 3] == pytest.approx(want, rel=1e-12)
    # R = 1 and a peak in the middle: no shift is two away, the ratio is +inf
    vec, _ = pc.correlate_model(im1, im1, 16, 16, 1)
    assert (vec[1:-1, 1:-1, 3] == np.inf).all()


def test_offsets_add_to_the_vectors():
    rng = np.random.default_rng(9)
    x, y = particles((96, 96), 12, 16, rng, margin=12)
    im1 = pc.particle_image((96, 96), x, y)
    im2 = pc.particle_image((96, 96), x + 7.3, y - 6.6)
    off = np.zeros((5, 5, 2), np.int32)
    off[...] = (7, -7)
    vec, flags = pc.correlate_model(im1, im2, 32, 16, 3, offset=off)
    inner = flags == 0
    assert inner.sum() >= 4
    assert np.abs(vec[inner, :2] - [7.3, -6.6]).max() < 0.1


def test_median_test_finds_a_planted_outlier_and_leaves_a_smooth_field():
    r, c = np.meshgrid(np.arange(12.0), np.arange(15.0), indexing="ij")
    v = np.stack([0.3 * c + 0.1 * r, -0.2 * r + 0.05 * c, np.ones_like(r), np.ones_like(r)], axis=-1)
    assert not pc.normalized_median_test(v).any()
    bad = v.copy()
    bad[5, 7, :2] += (4.0, -3.0)
    out = pc.normalized_median_test(bad)
    assert out[5, 7] and out.sum() == 1
    bad[0, 0, 0] = np.nan                                        # a NaN vector (a flat window) is an outlier, and not a
    out = pc.normalized_median_test(bad)                         # neighbour of the others
    assert out[0, 0] and out[5, 7] and out.sum() == 2
    flags = np.zeros(v.shape[:2], np.int32)
    off = pc.predictor(bad, flags, out)
    assert off.dtype == np.int32 and off.shape == (12, 15, 2)
    assert tuple(off[5, 7]) == tuple(np.rint(v[5, 7, :2]).astype(int))
    assert tuple(off[0, 0]) == tuple(np.rint(np.median(v[[0, 1, 1], [1, 0, 1], :2], axis=0)).astype(int))
    assert np.array_equal(off[2, 3], np.rint(v[2, 3, :2]).astype(np.int32))


def test_model_refuses_what_the_abi_refuses():
    im = np.zeros((64, 64))
    for win, step, R in ((24, 8, 4), (32, 0, 4), (32, 8, 0), (32, 8, 17), (16, 8, 9)):
        with pytest.raises(ValueError):
            pc.correlate_model(im, im, win, step, R)


def test_axis_mapping_helpers():
    v = np.array([[1.5, -2.0, 0.9, 3.0]])
    four = {"implement_diffraction": False, "x_pixel_number": 64}
    erf = {"implement_diffraction": True, "x_pixel_number": 64}
    assert np.array_equal(pc.sensor_displacements(v, four), [[1.5, -2.0]])
    assert np.array_equal(pc.sensor_displacements(v, erf), [[-1.5, -2.0]])
    assert np.array_equal(pc.image_positions(np.array([10.0, 20.0]), four), [9.0, 19.0])
    assert np.array_equal(pc.image_positions(np.array([10.0, 20.0]), erf), [52.0, 20.0])


# ---- the exact-arithmetic families of piv_correlation_cases.py: what the GPU test runs, shown from the model alone -----------
import piv_correlation_cases as cases      # noqa: E402


def _paths(name):
    c = cases.all_cases()[name]
    return c, cases.classify(c, *cases.model(name))


@pytest.mark.parametrize("name", cases.names())
def test_every_case_meets_the_exactness_condition(name):
    """From the images alone -- and the windows that are flat by their pixels are the model's flat windows."""
    c = cases.all_cases()[name]
    cases.assert_exact(c)
    s = cases.window_stats(c)
    _, flags, _ = cases.model(name)
    assert np.array_equal((flags & pc.FLAG_FLAT) != 0, s["flat_a"] | s["flat_b"])
    assert np.array_equal((flags & pc.FLAG_OUTSIDE) != 0, s["outside"])


def test_the_every_plan_family_covers_every_radius_with_a_plain_window():
    """Every (win, R) the ABI accepts, one launch each, with at least one window that is neither flat nor on the edge; steps
    that divide win, steps that do not, and step == win."""
    plan = [cases.all_cases()[n] for n in cases.names("plan")]
    assert sorted((c.win, c.R) for c in plan) == [(w, r) for w in (16, 32, 64) for r in range(1, w // 2 + 1)]
    for c in plan:
        assert _paths(c.name)[1]["inner"].any(), c.name
    for win in (16, 32, 64):
        steps = {c.step for c in plan if c.win == win}
        assert win in steps and any(win % s for s in steps) and any(win % s == 0 and s < win for s in steps)


def test_the_families_take_every_path_of_the_definition():
    """Counted over all cases from the model's outputs.  The zero-denominator branch of the fit is the one path no finite
    input reaches: the peak is the FIRST maximum, so C- (an earlier shift, in either axis) is strictly below C0 and C+ is at
    most C0 -- C- - 2 C0 + C+ < 0, and ln C- - 2 ln C0 + ln C+ < 0 likewise.  It stays a guard."""
    total = {}
    by_win = {}
    for name in cases.names():
        c, p = _paths(name)
        for key, mask in p.items():
            if mask.dtype == bool:
                total[key] = total.get(key, 0) + int(mask.sum())
                by_win[key, c.win] = by_win.get((key, c.win), 0) + int(mask.sum())
    print({k: v for k, v in sorted(total.items())})
    for key in ("gauss_nonzero_x", "gauss_nonzero_y", "parabolic_x", "parabolic_y", "parabolic_nonzero_x", "parabolic_nonzero_y",
                "edge_x_only", "edge_y_only", "edge_both", "tie", "tie_other_tile", "ratio_one", "ratio_inf_no_far_shift",
                "ratio_inf_far_not_positive", "flat_a", "flat_b", "flat_outside", "flat_constant_a", "flat_constant_b"):
        assert total.get(key, 0) > 0, key
    assert total["zero_den_x"] == 0 and total["zero_den_y"] == 0
    assert pc._subpixel(np.array([2.0, 4.0]), np.array([2.0, 4.0]), np.array([2.0, 4.0])).tolist() == [0.0, 0.0]      # the guard
    for win in (16, 32, 64):                                    # every window size: the Gaussian fit, each edge, a tie, flat
        for key in ("gauss_nonzero_x", "gauss_nonzero_y", "edge_x_only", "edge_y_only", "edge_both", "tie_other_tile",
                    "ratio_inf_no_far_shift", "flat_a", "flat_b", "flat_outside"):
            assert by_win.get((key, win), 0) > 0, (key, win)
    for win in (32, 64):
        assert by_win["flat_constant_a", win] > 0 and by_win["flat_constant_b", win] > 0
    # the tie at R = win / 2 goes to the earlier shift, -R
    for win in (16, 32, 64):
        c, p = _paths(f"plan_w{win}_r{win // 2}_s{cases.STEPS[win][(win // 2 - 1) % 8]}")
        assert p["tie"].any() and (p["px"][p["tie"]] == 0).all()


def test_constants_are_chosen_where_an_f32_mean_misses_them():
    """The replay of the kernel's own f32 sums: each constant of the constant family is one whose replayed mean differs from
    it (f32 energies above 0 on a window of equal pixels), and is not an integer."""
    for win, R, which in cases.CONSTANT_CONFIGS:
        c = cases.pick_constant(win, R, seed=win + R)
        assert c.dtype == np.float32 and c != np.rint(c)
        assert cases.replay_mean(c, win, cases.plan_threads(win, R)) != c
        case = cases.all_cases()[f"constant_{which}_w{win}_r{R}"]
        assert ((case.im1 if which == "a" else case.im2) == c).sum() >= 2 * win * win
    assert cases.replay_mean(np.float32(3.0), 64, 512) == np.float32(3.0)          # small integers: every sum is exact
    assert cases.replay_mean(np.float32(0.1), 16, 64) == np.float32(0.1)           # 4 copies a lane, then doublings: exact
