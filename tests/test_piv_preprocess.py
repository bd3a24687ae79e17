"""The host models of section 15 (photon_amd/piv_preprocess.py; CPU tier): the f32 chain against the f64 chain within a
derived bound, the exactness properties of the f32 chain, the mean against numpy's, the refusals, and the case the feature
is for -- a stationary wall that every raw window locks on."""
import numpy as np
import pytest

import piv_preprocess_cases as cs
from photon_amd import piv_correlation as pc
from photon_amd import piv_preprocess as pp

U = 2.0 ** -24          # the unit roundoff of f32


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ---- f32 against f64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 5, 8])
def test_the_f32_chain_is_within_the_derived_bound_of_the_f64_chain(radius):
    """Every term of a box sum is >= 0, so a relative error only grows by (1 + U) per operation it passes through: one
    subtraction (d), 2r additions along the row (the first, 0 + v, is exact), 2r along the column, one division: lo and hi
    are within eps = (4r + 2) U of the f64 values, relatively; (4r + 3) U is asserted to cover the second-order terms.  Far
    below the 289 U of a 289-term running sum: the sum is separable, no term passes through more than 4r additions.
    out = max(d - lo, 0) / max(hi - lo, floor) is continuous, so with den = max(hi - lo, floor) of the f64 chain
        |out32 - out64| <= [U d + eps lo + out64 (eps (hi + lo) + U den)] / den + 2 U out64     (numerator, denominator,
    the subtraction's and the division's own rounding), asserted with a factor 1.01 for the second-order terms.
    Measured on these frames (r = 1 | 5 | 8): hi uses at most 0.50 | 0.31 | 0.28 of its bound, lo 0.36 | 0.00 | 0.00 (with the
    stack's minimum as background mn is 0 nearly everywhere), out 0.39 | 0.25 | 0.26; the largest |out32 - out64| is 3.8e-7."""
    frames = cs.particle_frames((70, 90), 4, seed=3)
    bg = pp.background_model(frames, pp.MODE_MIN)
    floor = 0.05
    out32, lo32, hi32 = pp.preprocess_model_f32(frames, bg, radius, floor, parts=True)
    out64, lo, hi = pp.preprocess_model(frames, bg, radius, floor, parts=True)
    assert out32.dtype == np.float32 and out64.dtype == np.float64
    d = np.maximum(frames.astype(np.float64) - bg, 0.0)
    eps = (4 * radius + 3) * U
    worst = {}
    for name, got, want in (("lo", lo32, lo), ("hi", hi32, hi)):
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[name] = float(np.nanmax(np.where(want > 0, np.abs(got - want) / (eps * want), 0.0)))
        assert (np.abs(got - want) <= eps * want).all(), name
    den = np.maximum(hi - lo, floor)
    bound = 1.01 * ((U * d + eps * lo + out64 * (eps * (hi + lo) + U * den)) / den + 2 * U * out64)
    err = np.abs(out32 - out64)
    worst["out"] = float((err / np.maximum(bound, 1e-300)).max())
    print(f"r {radius}: share of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; largest |out32 - out64| {err.max():.3e}")
    assert (err <= bound).all()
    assert out64.max() > 0.9 and (out64 == 0).any()       # the frames reach full scale and the floor


# ---- exactness of the f32 chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 4, 8])
def test_a_constant_image_gives_exactly_zero(radius):
    """mn = mx = c everywhere, so lo and hi are the same operations on the same values: hi - lo is exactly 0 for every c, and
    the result is max(c - lo, 0) / floor.  Where 289 c is exact in f32 (c with at most 15 significant bits) lo = c and the
    result is exactly 0, with and without a background; a c that is not (0.1) leaves at most the sum's rounding,
    (4r + 1) U c / floor.  With the image as its own background d = 0 and the result is 0 for every c."""
    shape = (20, 37)
    for c in (0.0, 1.0, 0.5, 3.0, 1000.0, 5 * 2.0 ** -10, 0.1):
        im = np.full((2,) + shape, c, np.float32)
        out, lo, hi = pp.preprocess_model_f32(im, None, radius, 0.25, parts=True)
        assert np.array_equal(bits(lo), bits(hi))
        if c != 0.1:
            assert np.array_equal(bits(lo), bits(im)) and not out.any(), c
        else:
            assert (out <= (4 * radius + 1) * U * c / 0.25).all()
        assert not pp.preprocess_model_f32(im, im[0], radius, 0.25).any(), c
        half = pp.preprocess_model_f32(im, (im[0] / 2).astype(np.float32), radius, 0.25, parts=True)
        assert np.array_equal(bits(half[1]), bits(half[2]))
        if c != 0.1:
            assert not half[0].any(), c


@pytest.mark.parametrize("k", [-20, -3, 7, 40])
def test_scaling_by_a_power_of_two_returns_the_same_bits(k):
    frames = cs.particle_frames((40, 50), 3, seed=5)
    bg = pp.background_model(frames, pp.MODE_MEAN)
    s = np.float32(2.0 ** k)
    for radius, floor in ((0, None), (3, 0.05), (8, 0.3)):
        base = pp.preprocess_model_f32(frames, bg, radius, floor)
        scaled = pp.preprocess_model_f32(frames * s, bg * s, radius, None if floor is None else np.float32(floor) * s)
        want = base * s if radius == 0 else base        # the filter's result is a ratio
        assert np.array_equal(bits(scaled), bits(want)), (radius, k)


def test_the_minimum_as_background_leaves_a_zero_in_every_pixel_and_nothing_negative():
    frames = cs.particle_frames((33, 47), 6, seed=7)
    bg = pp.background_model(frames, pp.MODE_MIN)
    assert np.array_equal(bg, frames.min(axis=0))
    out = pp.preprocess_model_f32(frames, bg, 0)
    assert (out >= 0).all() and (out.min(axis=0) == 0).all() and (np.signbit(out) == 0).all()
    assert np.array_equal(out, frames - bg)


@pytest.mark.parametrize("radius", [2, 8])
def test_integer_frames_give_lo_and_hi_of_the_f64_chain_rounded_once(radius):
    """Integers up to 1000: every sum of at most 289 of them is an integer below 2^24, exact in f32 in any order, and the one
    division is correctly rounded on both sides (a quotient rounded to f64 and then to f32 is the quotient rounded to f32:
    53 >= 2 * 24 + 2)."""
    rng = np.random.default_rng(radius)
    frames = rng.integers(0, 1001, size=(2, 45, 38)).astype(np.float32)
    bg = rng.integers(0, 300, size=(45, 38)).astype(np.float32)
    assert 289 * 1000 < 2 ** 24
    for b in (bg, None):
        _, lo32, hi32 = pp.preprocess_model_f32(frames, b, radius, 1.0, parts=True)
        _, lo64, hi64 = pp.preprocess_model(frames, b, radius, 1.0, parts=True)
        assert np.array_equal(bits(lo32), bits(lo64.astype(np.float32))) and np.array_equal(bits(hi32), bits(hi64.astype(np.float32)))


def test_the_filter_against_a_direct_evaluation_of_the_definition():
    """Pixel by pixel, from the header's text: neighbourhood lists, Python loops, f64."""
    frames = cs.particle_frames((9, 12), 1, seed=9).astype(np.float64)
    r, floor = 2, 0.05
    d = frames[0]
    h, w = d.shape

    def over(a, y, x, f):
        return f(a[max(y - r, 0):min(y + r, h - 1) + 1, max(x - r, 0):min(x + r, w - 1) + 1])
    mn = np.array([[over(d, y, x, np.min) for x in range(w)] for y in range(h)])
    mx = np.array([[over(d, y, x, np.max) for x in range(w)] for y in range(h)])
    lo = np.array([[over(mn, y, x, np.mean) for x in range(w)] for y in range(h)])
    hi = np.array([[over(mx, y, x, np.mean) for x in range(w)] for y in range(h)])
    want = np.maximum(d - lo, 0) / np.maximum(hi - lo, floor)
    got = pp.preprocess_model(frames, None, r, floor)[0]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-14)


# ---- the background ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_the_mean_equals_numpy_in_f64_rounded_to_f32(n):
    frames = cs.particle_frames((31, 33), n, seed=n)
    want = np.mean(frames.astype(np.float64), axis=0).astype(np.float32)
    assert np.array_equal(bits(pp.background_model(frames, pp.MODE_MEAN)), bits(want))
    assert np.array_equal(bits(pp.background_model(frames, pp.MODE_MIN)), bits(frames.min(axis=0)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_everything_the_c_side_refuses_is_a_value_error():
    frames = np.zeros((3, 8, 9), np.float32)
    bg = np.zeros((8, 9), np.float32)
    for bad in (dict(shape=(0, 9)), dict(shape=(8, 0)), dict(shape=(8, (1 << 22) + 1)), dict(shape=((1 << 22) + 1, 8)),
                dict(n_frames=0), dict(n_frames=-1), dict(mode=2), dict(mode=-1), dict(radius=-1), dict(radius=9),
                dict(radius=3), dict(radius=3, floor=0.0), dict(radius=3, floor=-1.0), dict(radius=3, floor=float("nan")),
                dict(radius=3, floor=float("inf")), dict(radius=0, background=False), dict(frame_stride=71), dict(out_stride=71),
                dict(frame_stride=0), dict(frame_stride=-72)):
        args = dict(dict(shape=(8, 9), n_frames=3), **bad)
        with pytest.raises(ValueError):
            pp.check_arguments(**args)
    pp.check_arguments((8, 9), 3, radius=3, floor=0.1, frame_stride=72, out_stride=80)
    pp.check_arguments((1, 1 << 22), 1)
    for call in (lambda: pp.background_model(frames, 2), lambda: pp.background_model(frames[:0]), lambda: pp.background_model(frames[0, 0]),
                 lambda: pp.preprocess_model_f32(frames, None, 0), lambda: pp.preprocess_model_f32(frames, bg, 9, 0.1),
                 lambda: pp.preprocess_model_f32(frames, bg, 2), lambda: pp.preprocess_model_f32(frames, bg, 2, 0.0),
                 lambda: pp.preprocess_model_f32(frames, bg[:4], 0), lambda: pp.preprocess_model(frames, bg, 2, float("inf"))):
        with pytest.raises(ValueError):
            call()


# ---- what the feature is for ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_stationary_wall_defeats_the_raw_pair_and_not_the_processed_one(seed):
    """Of 25 windows, within 0.3 px of the true shift: at most 2 on the raw pair, at least 24 with each stack's own minimum
    subtracted, at least 24 with the min-max filter (r = 5, floor 0.05) on top.  Measured: 0, 25 and 25 for every seed."""
    a, b = cs.wall_series(seed)
    assert a.shape == (cs.WALL_PAIRS, 96, 96)
    counts = {"raw": cs.near_truth(pc.correlate_model(a[0], b[0], cs.WALL_WIN, cs.WALL_STEP, cs.WALL_R)[0])}
    for name, radius in (("minimum subtracted", 0), ("and filtered", cs.WALL_RADIUS)):
        pa, pb = cs.wall_processed(seed, radius)
        vec, flags = pc.correlate_model(pa[0], pb[0], cs.WALL_WIN, cs.WALL_STEP, cs.WALL_R)
        assert vec.shape == (5, 5, 4)
        counts[name] = cs.near_truth(vec)
    print(f"seed {seed}: windows within {cs.WALL_WITHIN} px of {cs.WALL_SHIFT}: {counts}")
    assert counts["raw"] <= 2
    assert counts["minimum subtracted"] >= 24
    assert counts["and filtered"] >= 24
