"""FFT correlation of image pairs (include/parallel_ray_tracing.h, section 13) without a GPU: the f32 model against the f64
definition, mode 0 against brute force, the library's tables against the model's, the pair on a stationary background that
amplitude correlation loses, the deformation loop with the phase correlator, and the refusals."""
import ctypes

import numpy as np
import pytest

import piv_deformation_cases as dcs
import piv_phase_cases as cs
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_phase as pp


@pytest.mark.parametrize("win, step, R", [(16, 8, 7), (32, 16, 8), (64, 32, 31)])
@pytest.mark.parametrize("mode, sigma_frac, diameter", [(0, 0.0, 0.0), (0, 0.25, 0.0), (1, 0.0, 0.0), (1, 0.25, 2.5)])
def test_f32_model_against_f64_model(win, step, R, mode, sigma_frac, diameter):
    """Planes within 1e-5 of each plane's peak (f32 eps x 12 butterfly stages, with room), identical integer peaks, and
    |delta d| <= 1e-4 px where the two highest plane values differ by more than 1e-3 of the peak."""
    im1, im2 = cs.background_pair()
    how = dict(mode=mode, window_sigma=sigma_frac * win, diameter=diameter, planes=True)
    v32, f32, p32 = pp.correlate_phase_model_f32(im1, im2, win, step, R, **how)
    v64, f64, p64 = pp.correlate_phase_model(im1, im2, win, step, R, **how)
    assert v32.dtype == np.float32 and p32.dtype == np.float32 and np.array_equal(f32, f64) and not (f64 & pc.FLAG_FLAT).any()
    n = f64.size
    p32, p64 = p32.reshape(n, -1).astype(np.float64), p64.reshape(n, -1)
    peak = p64.max(axis=1)
    err = (np.abs(p32 - p64).max(axis=1) / peak).max()
    print(f"win {win} mode {mode} sigma {sigma_frac * win:g} d {diameter:g}: largest plane difference {err:.3g} of the peak")
    assert err <= 1e-5
    assert np.array_equal(np.argmax(p32, axis=1), np.argmax(p64, axis=1))
    srt = np.sort(p64, axis=1)
    clear = (srt[:, -1] - srt[:, -2] > 1e-3 * peak).reshape(f64.shape)
    assert clear.mean() > 0.5
    assert np.abs(v32[clear][:, :2] - v64[clear][:, :2]).max() <= 1e-4


def test_mode_0_is_the_circular_correlation_of_the_definition():
    """A 16 x 16 window, brute force: Cn(s) = sum_p a'(p) b'(p + s mod win) / sqrt(sum a'^2 sum b'^2)."""
    win, R, sigma = 16, 7, 4.0
    rng = np.random.default_rng(3)
    im1, im2 = rng.random((win, win)), rng.random((win, win))
    g = np.exp(-(np.arange(win) - (win - 1) / 2.0) ** 2 / (2.0 * sigma ** 2))
    a = (im1 - im1.mean()) * g[:, None] * g[None, :]
    b = (im2 - im2.mean()) * g[:, None] * g[None, :]
    want = np.empty((2 * R + 1, 2 * R + 1))
    for sy in range(-R, R + 1):
        for sx in range(-R, R + 1):
            want[sy + R, sx + R] = (a * np.roll(b, (-sy, -sx), axis=(0, 1))).sum()
    want /= np.sqrt((a * a).sum() * (b * b).sum())
    _, _, p64 = pp.correlate_phase_model(im1, im2, win, win, R, mode=0, window_sigma=sigma, planes=True)
    _, _, p32 = pp.correlate_phase_model_f32(im1, im2, win, win, R, mode=0, window_sigma=sigma, planes=True)
    assert np.abs(p64[0, 0] - want).max() <= 1e-13
    assert np.abs(p32[0, 0] - want).max() <= 1e-5 * want.max()


def test_a_pure_circular_shift_has_a_unit_phase_peak():
    win = 32
    rng = np.random.default_rng(5)
    a = rng.random((win, win))
    for diameter in (0.0, 2.5):
        vec, flg, planes = pp.correlate_phase_model(a, np.roll(a, (3, -5), axis=(0, 1)), win, win, 8, mode=1, diameter=diameter, planes=True)
        assert flg[0, 0] == 0 and abs(vec[0, 0, 2] - 1.0) <= 1e-12
        assert np.unravel_index(np.argmax(planes[0, 0]), planes[0, 0].shape) == (8 + 3, 8 - 5)


@pytest.mark.parametrize("win", pc.WINDOW_SIZES)
@pytest.mark.parametrize("sigma_frac, diameter", [(0.0, 0.0), (0.25, 2.5), (0.3, 3.7)])
def test_library_tables_equal_the_models_bit_for_bit(win, sigma_frac, diameter):
    """photon_piv_phase_tables is host code: the library loads and answers without a GPU.  A last-bit difference between
    the library's elementary functions and numpy's shows here, not in the kernel's tests."""
    from photon_amd import build
    from photon_amd.library import apply_signatures
    lib = apply_signatures(ctypes.CDLL(build.build_library()))
    tw, g, w = np.zeros((win // 2, 2), np.float32), np.zeros(win, np.float32), np.zeros(win, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    assert lib.photon_piv_phase_tables(win, sigma_frac * win, diameter, vp(tw), vp(g), vp(w)) == 0
    want = pp.tables(win, sigma_frac * win, diameter)
    for got, ref in zip((tw, g, w), want):
        assert got.tobytes() == ref.tobytes()
    assert tuple(tw[0]) == (1.0, 0.0) and tuple(tw[win // 4]) == (0.0, -1.0)
    assert (g == 1.0).all() if sigma_frac == 0.0 else (g[0] < g[win // 2 - 1] == g[win // 2] < 1.0)
    assert np.array_equal(w[1:], w[1:][::-1])               # w(k) = w(-k)


def test_background_pair_phase_finds_what_direct_loses():
    im1, im2 = cs.background_pair()
    vp_, fp_ = pp.correlate_phase_model(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_RADIUS, mode=1, window_sigma=cs.BG_WIN / 4.0,
                                        diameter=cs.BG_DIAMETER)
    vd, _ = pc.correlate_model(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_RADIUS)
    ok_p, ok_d = cs.valid(vp_), cs.valid(vd)
    e = vp_[ok_p][:, :2] - np.array(cs.BG_SHIFT)
    print(f"background pair: phase {int(ok_p.sum())} of {ok_p.size} within 0.5 px (RMS {np.sqrt((e * e).sum(axis=1).mean()):.3f} px), "
          f"direct {int(ok_d.sum())} of {ok_d.size}")
    assert ok_p.mean() >= 0.95
    assert ok_d.mean() <= 0.50


@pytest.mark.parametrize("kind", ["vortex", "uniform"])
@pytest.mark.parametrize("seed", [1, 2])
def test_deformation_loop_with_the_phase_correlator(kind, seed):
    """Interior RMS of the phase loop <= 1.1 x the direct loop's on the same pair (same validation, same warps, 3 iterations)."""
    im1, im2 = dcs.pair(kind, seed)
    direct = dcs.interior_rms(pd.correlate_deform_model(im1, im2, dcs.WIN, dcs.STEP, dcs.RADIUS, iterations=3)[0], kind)
    phase = dcs.interior_rms(pd.correlate_deform_model(im1, im2, dcs.WIN, dcs.STEP, dcs.RADIUS, iterations=3, method="phase")[0], kind)
    print(f"{kind} seed {seed}: direct loop {direct:.4f} px, phase loop {phase:.4f} px, ratio {phase / direct:.2f}")
    assert phase <= 1.1 * direct


def test_method_direct_is_the_default_and_unchanged():
    im1, im2 = dcs.pair("uniform", 1, shape=(96, 96))
    a = pd.correlate_deform_model(im1, im2, 32, 16, iterations=1)
    b = pd.correlate_deform_model(im1, im2, 32, 16, iterations=1, method="direct")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(ValueError):
        pd.correlate_deform_model(im1, im2, 32, 16, method="fourier")


def test_drivers_radius_for_the_phase_method():
    assert [pp.default_radius(32, r) for r in (None, 16, 15, 4)] == [15, 15, 15, 4]


def test_device_cases_have_no_ill_conditioned_fit():
    """The seeds of the device comparison: no window of the f32 model whose log-curvature lies below 1e-6, so that the
    device's subpixel bound holds for every window."""
    for k in range(len(cs.DEVICE_CASES)):
        _, flags, planes = cs.device_case(k)[3]
        curv = pp.log_curvature(planes)[(flags & pc.FLAG_FLAT) == 0]
        assert (curv >= 1e-6).all(), (cs.case_id(cs.DEVICE_CASES[k]), curv.min())


@pytest.mark.parametrize("kind", ["checkerboard", "stripes"])
@pytest.mark.parametrize("win", pc.WINDOW_SIZES)
def test_periodic_patterns_leave_zero_bins(kind, win):
    im1, im2 = cs.periodic_pair(kind)
    vec, flags, planes, info = pp.correlate_phase_model_f32(im1, im2, win, win, win // 2 - 1, mode=1, planes=True, details=True)
    assert (info["zero_bins"] >= win * win - 5).all() and (info["zero_bins"] < win * win - 1).all()
    assert not (flags & pc.FLAG_FLAT).any() and np.isfinite(planes).all()


def test_refusals():
    shape = (64, 80)
    pp.check_arguments(shape, 16, 8, 7, 1, 4.0, 2.5)
    for kwargs in (dict(win=24), dict(win=128), dict(radius=0), dict(radius=8), dict(step=0), dict(shape=(15, 80)), dict(mode=2),
                   dict(mode=-1), dict(window_sigma=-1.0), dict(window_sigma=float("nan")), dict(window_sigma=float("inf")),
                   dict(diameter=-0.5), dict(diameter=float("nan")), dict(diameter=float("inf"))):
        args = dict(shape=shape, win=16, step=8, radius=7, mode=1, window_sigma=4.0, diameter=2.5)
        args.update(kwargs)
        with pytest.raises(ValueError):
            pp.check_arguments(**args)
    with pytest.raises(ValueError):
        pp.correlate_phase_model(np.zeros((64, 80)), np.zeros((64, 80)), 16, 8, 8)
    with pytest.raises(ValueError):
        pp.correlate_phase_model_f32(np.zeros((64, 80)), np.zeros((64, 81)), 16, 8, 7)
