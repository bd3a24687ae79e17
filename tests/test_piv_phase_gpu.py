"""photon_piv_correlate_phase on the GPU (include/parallel_ray_tracing.h, section 13): planes, peaks, ratios and flags equal
to the f32 host model of photon_amd/piv_phase.py value for value, zero bins, flat windows, repeats, output bounds, the
refusals, the drivers with method="phase", and the kernel's time next to photon_piv_correlate's."""
import ctypes

import numpy as np
import pytest

import piv_deformation_cases as dcs
import piv_phase_cases as cs
import piv_tail_cases
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_phase as pp

pytestmark = pytest.mark.gpu


def device_phase(photon, im1, im2, win, step, R, offset=None, mode=1, window_sigma=0.0, diameter=0.0, planes=True):
    import torch
    a, b = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    off = torch.from_numpy(np.ascontiguousarray(offset, np.int32)).cuda() if offset is not None else None
    h, w = im1.shape
    vec, flg, pl = photon.piv_correlate_phase(a.data_ptr(), b.data_ptr(), w, h, win, step, R, off.data_ptr() if off is not None else 0,
                                              planes=planes, mode=mode, window_sigma=window_sigma, diameter=diameter)
    torch.cuda.synchronize()
    return vec.cpu().numpy(), flg.cpu().numpy(), (pl.cpu().numpy() if planes else None)


def same_values(got, want):
    """== (so that -0 equals +0), NaN equal to NaN."""
    return bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


@pytest.mark.parametrize("index", range(len(cs.DEVICE_CASES)), ids=[cs.case_id(c) for c in cs.DEVICE_CASES])
def test_device_equals_the_f32_model(photon, index):
    win, R, step, shape, _, with_off, mode, sigma, diameter = cs.DEVICE_CASES[index]
    im1, im2, off, want = cs.device_case(index)
    if with_off:
        assert (want[1] & pc.FLAG_OUTSIDE).any()
    assert not (want[1] & pc.FLAG_FLAT).any()
    worst = assert_equals_the_f32_model(device_phase(photon, im1, im2, win, step, R, off, mode, sigma, diameter), want)
    print(f"{cs.case_id(cs.DEVICE_CASES[index])}: {want[1].size} windows, largest |delta d| {worst:.3g} px")


def assert_equals_the_f32_model(got, want):
    """Flags, planes (NaN where the model has NaN), argmax, peak and ratio value for value; the subpixel part within 1e-5 px:
    the f32 ulp at 31 px (1.9e-6) plus the device's f64 log against numpy's.  A window whose log-curvature lies below 1e-6
    would be excluded (at most 1 % of the windows that are not flat) -- the cases have none (tests/test_piv_phase.py).
    Returns the largest subpixel difference."""
    (got_v, got_f, got_p), (want_v, want_f, want_p) = got, want
    assert got_v.shape == want_v.shape and got_p.shape == want_p.shape and got_p.dtype == want_p.dtype
    assert np.array_equal(got_f, want_f), np.argwhere(got_f != want_f)[:5]
    assert same_values(got_p, want_p), float(np.abs(got_p - want_p).max())
    live = (want_f & pc.FLAG_FLAT) == 0
    n = int(live.sum())
    assert np.array_equal(np.argmax(got_p[live].reshape(n, -1), axis=1), np.argmax(want_p[live].reshape(n, -1), axis=1))
    assert np.isnan(got_v[~live]).all()
    assert same_values(got_v[..., 2], want_v[..., 2]) and same_values(got_v[..., 3], want_v[..., 3])
    keep = (pp.log_curvature(want_p[live]) >= 1e-6).all(axis=-1)
    assert keep.mean() >= 0.99
    dv = np.abs(got_v[live][keep][:, :2].astype(np.float64) - want_v[live][keep][:, :2])
    assert dv.max() <= 1e-5
    return float(dv.max())


NINE_FLAGS = {0: [[6, 1, 0], [0, 0, 4], [0, 4, 0]], 1: [[6, 1, 0], [0, 0, 4], [0, 4, 1]]}


def nine_windows(mode):
    """piv_tail_cases.nine_windows with section 13's second frame and offsets: flat + outside, a
    peak on the plane's edge, outside alone and clean windows in one launch.  (im1, im2, offset, the f32 model's outputs)"""
    im1, _, im2, off = piv_tail_cases.nine_windows()
    want = pp.correlate_phase_model_f32(im1, im2, 16, 16, 4, offset=off, mode=mode, window_sigma=4.0, diameter=2.5, planes=True)
    assert want[1].tolist() == NINE_FLAGS[mode]
    return im1, im2, off, want


@pytest.mark.parametrize("mode", [0, 1])
def test_every_branch_of_the_peak_tail_in_nine_windows(photon, mode):
    im1, im2, off, want = nine_windows(mode)
    assert_equals_the_f32_model(device_phase(photon, im1, im2, 16, 16, 4, off, mode, 4.0, 2.5), want)


@pytest.mark.parametrize("index", [1, 4, 8, "nine"])
def test_without_planes_the_vectors_and_flags_are_the_same_bytes(photon, index):
    """d_planes = NULL: the same vector and flag bytes, at win 16, 32 and 64 and on the nine windows with their flat one."""
    if index == "nine":
        im1, im2, off, _ = nine_windows(1)
        args = (16, 16, 4, off, 1, 4.0, 2.5)
    else:
        win, R, step, _, _, _, mode, sigma, diameter = cs.DEVICE_CASES[index]
        im1, im2, off, _ = cs.device_case(index)
        args = (win, step, R, off, mode, sigma, diameter)
    v1, f1, _ = device_phase(photon, im1, im2, *args, planes=True)
    v0, f0, p0 = device_phase(photon, im1, im2, *args, planes=False)
    assert p0 is None and v0.tobytes() == v1.tobytes() and f0.tobytes() == f1.tobytes()


@pytest.mark.parametrize("kind", ["checkerboard", "stripes"])
@pytest.mark.parametrize("win", pc.WINDOW_SIZES)
def test_zero_bins_contribute_zero(photon, kind, win):
    im1, im2 = cs.periodic_pair(kind)
    R = win // 2 - 1
    want_v, want_f, want_p, info = pp.correlate_phase_model_f32(im1, im2, win, win, R, mode=1, planes=True, details=True)
    assert (info["zero_bins"] >= win * win - 5).all()
    got_v, got_f, got_p = device_phase(photon, im1, im2, win, win, R)
    assert np.isfinite(got_p).all() and same_values(got_p, want_p) and np.array_equal(got_f, want_f)
    assert same_values(got_v[..., 2:], want_v[..., 2:])


@pytest.mark.parametrize("mode", [0, 1])
def test_flat_windows_are_flagged_and_nan(photon, mode):
    im1, im2 = (a.copy() for a in cs.particle_pair((96, 128), (1.2, -0.7), seed=9))
    im1[32:64, 64:96] = 0.25                                    # window (1, 2) of the 32 px grid: constant in frame 1
    im2[0:32, 0:32] = -1.0                                      # window (0, 0): constant in frame 2
    vec, flg, pl = device_phase(photon, im1, im2, 32, 32, 8, mode=mode, window_sigma=8.0, diameter=2.5)
    want_v, want_f, want_p = pp.correlate_phase_model_f32(im1, im2, 32, 32, 8, mode=mode, window_sigma=8.0, diameter=2.5, planes=True)
    flat = (flg & pc.FLAG_FLAT) != 0
    assert flat[1, 2] and flat[0, 0] and flat.sum() == 2 and np.array_equal(flg, want_f)
    assert np.isnan(vec[flat]).all() and np.isnan(pl[flat]).all()
    assert np.isfinite(vec[~flat][:, :3]).all() and same_values(pl, want_p)


def test_two_calls_return_identical_bytes(photon):
    im1, im2 = cs.particle_pair((140, 200), (3.3, -2.7), seed=5)
    for win, step, R, mode in ((32, 16, 15, 1), (64, 32, 31, 1), (16, 8, 3, 0)):
        a = device_phase(photon, im1, im2, win, step, R, mode=mode, window_sigma=win / 4.0, diameter=2.5)
        b = device_phase(photon, im1, im2, win, step, R, mode=mode, window_sigma=win / 4.0, diameter=2.5)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_outputs_stay_inside_the_grid(photon):
    import torch
    L = photon.lib
    im1, im2 = (torch.from_numpy(a).cuda() for a in cs.particle_pair((70, 90), (0.5, 0.5), seed=2))
    win, step, R = 16, 8, 5
    n, ns2, tail = 7 * 10, (2 * R + 1) ** 2, 333
    vec = torch.full((4 * n + tail,), 7.0, device="cuda")
    flg = torch.full((n + tail,), 7, dtype=torch.int32, device="cuda")
    pl = torch.full((n * ns2 + tail,), 7.0, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                # noqa: E731
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert L.photon_piv_correlate_phase(vp(im1), vp(im2), 90, 70, win, step, R, None, 1, 4.0, 2.5, vp(vec), vp(flg), vp(pl),
                                        ctypes.byref(r), ctypes.byref(c), None) == 0
    torch.cuda.synchronize()
    assert (r.value, c.value) == (7, 10)
    assert (vec[4 * n:] == 7.0).all().item() and (flg[n:] == 7).all().item() and (pl[n * ns2:] == 7.0).all().item()
    assert not (flg[:n] == 7).any().item() and not (pl[:n * ns2] == 7.0).any().item()
    assert not (vec[:4 * n].reshape(n, 4)[:, 2] == 7.0).any().item()


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.rand((64, 80), device="cuda")
    vec = torch.full((64, 4), 7.0, device="cuda")
    flg = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p, v, f = (ctypes.c_void_p(t.data_ptr()) for t in (im, vec, flg))
    nan, inf = float("nan"), float("inf")
    good = dict(im1=p, im2=p, width=80, height=64, win=16, step=8, radius=4, mode=1, sigma=4.0, diameter=2.5, vec=v, flg=f)
    capfd.readouterr()
    for what, change in (("win 24", dict(win=24)), ("win 128", dict(win=128)), ("R 0", dict(radius=0)), ("R = win/2", dict(radius=8)),
                         ("step 0", dict(step=0)), ("image too small", dict(height=15)), ("null im1", dict(im1=None)),
                         ("null im2", dict(im2=None)), ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)),
                         ("sigma < 0", dict(sigma=-1.0)), ("sigma nan", dict(sigma=nan)), ("sigma inf", dict(sigma=inf)),
                         ("diameter < 0", dict(diameter=-2.5)), ("diameter nan", dict(diameter=nan)), ("diameter inf", dict(diameter=inf)),
                         ("vectors without flags", dict(flg=None))):
        a = dict(good, **change)
        r, c = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_correlate_phase(a["im1"], a["im2"], a["width"], a["height"], a["win"], a["step"], a["radius"], None, a["mode"],
                                          a["sigma"], a["diameter"], a["vec"], a["flg"], None, ctypes.byref(r), ctypes.byref(c), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, what
        assert len(err.strip().splitlines()) == 1 and "photon_piv_correlate_phase" in err, (what, err)
        assert r.value == -5 and c.value == -5, what
        assert (vec == 7.0).all().item() and (flg == 7).all().item(), what
    r, c = ctypes.c_int(0), ctypes.c_int(0)                     # the size query: no launch, nothing written but the grid
    assert L.photon_piv_correlate_phase(p, p, 80, 64, 16, 8, 4, None, 1, 4.0, 2.5, None, None, None, ctypes.byref(r), ctypes.byref(c), None) == 0
    torch.cuda.synchronize()
    assert (r.value, c.value) == ((64 - 16) // 8 + 1, (80 - 16) // 8 + 1)
    assert (vec == 7.0).all().item() and (flg == 7).all().item()
    assert capfd.readouterr().err == ""
    tw = np.zeros(16, np.float32)
    t = tw.ctypes.data_as(ctypes.c_void_p)
    for args in ((24, 4.0, 2.5, t, t, t), (16, -1.0, 2.5, t, t, t), (16, 4.0, nan, t, t, t), (16, 4.0, 2.5, t, None, t)):
        assert L.photon_piv_phase_tables(*args) == 1
        err = capfd.readouterr().err
        assert len(err.strip().splitlines()) == 1 and "photon_piv_phase_tables" in err
    assert (tw == 0).all()


def test_background_pair_end_to_end(photon):
    """The capability: on a pair with a stationary background, correlate(method="phase") returns the model's valid vectors,
    at least 95 % of all; correlate(method="direct") keeps at most half."""
    im1, im2 = cs.background_pair()
    vec, flg = photon.correlate(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_RADIUS, method="phase")
    want_v, want_f = pp.correlate_phase_model_f32(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_RADIUS, mode=1, window_sigma=cs.BG_WIN / 4.0,
                                                  diameter=cs.BG_DIAMETER)
    assert vec.shape == want_v.shape and np.array_equal(flg, want_f)
    ok = cs.valid(vec)
    assert np.array_equal(ok, cs.valid(want_v))
    direct, _ = photon.correlate(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_RADIUS)
    ok_d = cs.valid(direct)
    print(f"background pair on the device: phase {int(ok.sum())} of {ok.size} within 0.5 px, direct {int(ok_d.sum())} of {ok_d.size}")
    assert ok.mean() >= 0.95
    assert ok_d.mean() <= 0.50
    # the default radius of the phase method, and the predictor driver on the same correlator
    v15, _ = photon.correlate(im1, im2, cs.BG_WIN, cs.BG_STEP, method="phase")
    v15b, _ = photon.correlate(im1, im2, cs.BG_WIN, cs.BG_STEP, cs.BG_WIN // 2, method="phase")
    assert v15.tobytes() == v15b.tobytes()
    pred = photon.correlation_predictor(im1, im2, cs.BG_WIN, cs.BG_STEP, method="phase").cpu().numpy()
    assert np.abs(pred - np.array(cs.BG_SHIFT, np.float32)).max() < 0.5
    with pytest.raises(ValueError):
        photon.correlate(im1, im2, cs.BG_WIN, cs.BG_STEP, method="fourier")


@pytest.mark.parametrize("seed", [1, 2])
def test_deformation_driver_with_the_phase_method(photon, seed):
    im1, im2 = (c.astype(np.float32) for c in dcs.pair("vortex", seed))
    vec, status = photon.correlate_deform(im1, im2, dcs.WIN, dcs.STEP, dcs.RADIUS, iterations=3, method="phase")
    rms = dcs.interior_rms(vec, "vortex")
    model = dcs.interior_rms(pd.correlate_deform_model(im1, im2, dcs.WIN, dcs.STEP, dcs.RADIUS, iterations=3, method="phase")[0], "vortex")
    print(f"vortex seed {seed}, phase loop: device {rms:.4f} px, model {model:.4f} px")
    assert abs(rms - model) <= 0.02


def test_iterations_zero_is_one_phase_pass_plus_validation(photon):
    im1, im2 = (c.astype(np.float32) for c in dcs.pair("rotation", 3))
    vec, status = photon.correlate_deform(im1, im2, dcs.WIN, dcs.STEP, iterations=0, method="phase")
    v1, f1 = photon.correlate(im1, im2, dcs.WIN, dcs.STEP, method="phase")
    field, _, st, _, score = pd.validate_model(None, v1, f1)
    assert dcs.decided(score).all()
    assert np.array_equal(vec[..., :2], field) and np.array_equal(status, st)
    assert np.array_equal(vec[..., 2:], v1[..., 2:])


def test_phase_kernel_is_no_slower_than_direct_at_full_radius(photon):
    """1024^2, device events, alternating calls after a warm-up, the median of five: the phase kernel at R = win/2 - 1 takes
    no longer than photon_piv_correlate at R = win/2 (by operation count the margin is 17 x at win 32 and 40 x at win 64).
    At R 4 both times are recorded, with no bound."""
    import torch
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    a, b = (torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6)))
    h = w = 1024

    def ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for win, step in ((32, 16), (64, 32)):
        calls = {}
        for R in (4, win // 2):
            calls[f"direct R {R}"] = lambda R=R: photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R)
            Rp = min(R, win // 2 - 1)
            calls[f"phase R {Rp}"] = lambda Rp=Rp: photon.piv_correlate_phase(a.data_ptr(), b.data_ptr(), w, h, win, step, Rp, mode=1,
                                                                              window_sigma=win / 4.0, diameter=2.5)
        times = {k: [] for k in calls}
        for rep in range(7):                                    # two warm-up rounds, then five
            for k, fn in calls.items():
                t = ms(fn)
                if rep >= 2:
                    times[k].append(t)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"1024^2 win {win} step {step}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in med.items()))
        assert med[f"phase R {win // 2 - 1}"] <= med[f"direct R {win // 2}"]
