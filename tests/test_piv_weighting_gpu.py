"""photon_piv_correlate_weighted on the GPU (include/parallel_ray_tracing.h, section 18): section 5's bits with a table of
ones, the f64 host model of photon_amd/piv_weighting.py with three tables, scale and repeat invariance, flatness by weight,
the refusals, the C helper's table, the drivers' weighting= and the response study."""
import ctypes

import numpy as np
import pytest

import piv_tail_cases
import piv_weighting_cases as cases
import test_piv_correlation_gpu as base
from photon_amd import piv_correlation as pc
from photon_amd import piv_weighting as pw

pytestmark = pytest.mark.gpu

IDS = [f"w{c[0]}_r{c[1]}_s{c[2]}_{c[3][0]}x{c[3][1]}{'_off' if c[5] else ''}" for c in base.CASES]


def device_weighted(photon, im1, im2, table, win, step, R, offset=None, planes=True):
    import torch
    a, b = torch.from_numpy(np.array(im1)).cuda(), torch.from_numpy(np.array(im2)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(table, np.float32)).cuda()
    off = torch.from_numpy(np.ascontiguousarray(offset, np.int32)).cuda() if offset is not None else None
    h, w = im1.shape
    vec, flg, pl = photon.piv_correlate_weighted(a.data_ptr(), b.data_ptr(), t.data_ptr(), w, h, win, step, R,
                                                 off.data_ptr() if off is not None else 0, planes=planes)
    torch.cuda.synchronize()
    return vec.cpu().numpy(), flg.cpu().numpy(), (pl.cpu().numpy() if planes else None)


def pair_of(case):
    win, R, step, shape, shift, with_off = case
    im1, im2 = base.particle_pair(shape, shift, seed=win * 100 + R + step)
    off = np.random.default_rng(R).integers(-3, 4, size=pc.grid_shape(shape, win, step) + (2,)).astype(np.int32) if with_off else None
    return im1, im2, off


def assert_same_bits(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()


# ---- 1. a table of ones is section 5 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", base.CASES, ids=IDS)
def test_a_table_of_ones_returns_section_5s_bits(photon, case):
    win, R, step = case[:3]
    im1, im2, off = pair_of(case)
    want = base.device_correlate(photon, im1, im2, win, step, R, off)
    assert (want[1] & pc.FLAG_OUTSIDE).any() and np.isfinite(want[0]).any()
    assert_same_bits(device_weighted(photon, im1, im2, np.ones((win, win), np.float32), win, step, R, off), want)
    assert_same_bits(device_weighted(photon, im1, im2, photon.piv_window_weights(win, "uniform"), win, step, R, off, planes=False)[:2], want[:2])


def test_a_table_of_ones_returns_section_5s_bits_on_the_nine_windows(photon):
    im1, im2, _, _ = piv_tail_cases.nine_windows()
    want = base.device_correlate(photon, im1, im2, 16, 16, 4)
    assert want[1].tolist() == [[6, 4, 5], [4, 0, 6], [5, 4, 4]]
    assert_same_bits(device_weighted(photon, im1, im2, np.ones((16, 16), np.float32), 16, 16, 4), want)


# ---- 2. against the f64 model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(cases.TABLES))
@pytest.mark.parametrize("case", base.CASES, ids=IDS)
def test_device_matches_the_host_model(photon, case, kind):
    win, R, step = case[:3]
    im1, im2, off = pair_of(case)
    table = cases.TABLES[kind](win)
    want = pw.correlate_weighted_model(im1, im2, table, win, step, R, offset=off, planes=True)
    assert (want[1] & pc.FLAG_OUTSIDE).any()
    clear = base.assert_close_to_the_host_model(device_weighted(photon, im1, im2, table, win, step, R, off), want)
    print(f"{kind}: {clear.mean():.3f} of the live windows clear")
    if kind == "gaussian":
        assert clear.mean() > 0.5


# ---- 3. the same bits: a table scaled by 4, a second call -------------------------------------------------------------------------
@pytest.mark.parametrize("case", [base.CASES[1], base.CASES[5], base.CASES[9]], ids=[IDS[1], IDS[5], IDS[9]])
def test_the_scale_of_the_table_and_a_second_call_change_no_bit(photon, case):
    win, R, step = case[:3]
    im1, im2, off = pair_of(case)
    for table in (pw.window_weights(win), cases.asymmetric(win)):
        first = device_weighted(photon, im1, im2, table, win, step, R, off)
        assert_same_bits(device_weighted(photon, im1, im2, table, win, step, R, off), first)
        assert_same_bits(device_weighted(photon, im1, im2, 4.0 * table, win, step, R, off), first)


# ---- 4. flat by weight ----------------------------------------------------------------------------------------------------------
def test_a_window_whose_varying_pixels_have_no_weight_is_flat(photon):
    im1, im2, table = cases.flat_by_weight()
    vec, flags, planes = device_weighted(photon, im1, im2, table, 16, 16, 4)
    assert (flags & ~pc.FLAG_EDGE_PEAK).tolist() == [[pc.FLAG_FLAT | pc.FLAG_OUTSIDE, pc.FLAG_OUTSIDE]]
    assert np.isnan(vec[0, 0]).all() and np.isnan(planes[0, 0]).all()
    assert np.isfinite(vec[0, 1]).all() and np.isfinite(planes[0, 1]).all()
    base.assert_close_to_the_host_model((vec, flags, planes), pw.correlate_weighted_model(im1, im2, table, 16, 16, 4, planes=True))
    assert (base.device_correlate(photon, im1, im2, 16, 16, 4)[1] & pc.FLAG_FLAT == 0).all()         # without the table: alive
    off = np.array([[[0, 0], [40, 0]]], np.int32)                  # no pixel of b at zero shift in the image
    assert device_weighted(photon, im1, im2, table, 16, 16, 4, off)[1][0, 1] == pc.FLAG_FLAT | pc.FLAG_OUTSIDE


@pytest.mark.parametrize("where", [(0, 0), (7, 9), (15, 15)])
def test_a_single_positive_weight_is_flat(photon, where):
    im1, im2, _ = cases.flat_by_weight()
    for table in (cases.single(16, *where), np.zeros((16, 16), np.float32), np.full((16, 16), -1.0), np.full((16, 16), np.nan)):
        vec, flags, planes = device_weighted(photon, im1, im2, table, 16, 16, 4)
        assert (flags == (pc.FLAG_FLAT | pc.FLAG_OUTSIDE)).all() and np.isnan(vec).all() and np.isnan(planes).all()


# ---- 5. refusals, the size query, the helper's table --------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.rand((64, 80), device="cuda")
    tab = torch.ones((16, 16), device="cuda")
    vec = torch.full((64, 4), 7.0, device="cuda")
    flg = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p, t = ctypes.c_void_p(im.data_ptr()), ctypes.c_void_p(tab.data_ptr())
    capfd.readouterr()
    for what, args in (("win 24", (p, p, t, 80, 64, 24, 8, 4)), ("win 128", (p, p, t, 80, 64, 128, 8, 4)),
                       ("R 0", (p, p, t, 80, 64, 16, 8, 0)), ("R > win/2", (p, p, t, 80, 64, 16, 8, 9)),
                       ("step 0", (p, p, t, 80, 64, 16, 0, 4)), ("image too small", (p, p, t, 80, 15, 16, 8, 4)),
                       ("null im1", (None, p, t, 80, 64, 16, 8, 4)), ("null im2", (p, None, t, 80, 64, 16, 8, 4)),
                       ("null weight", (p, p, None, 80, 64, 16, 8, 4))):
        r, c = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_correlate_weighted(*args, None, ctypes.c_void_p(vec.data_ptr()), ctypes.c_void_p(flg.data_ptr()), None,
                                             ctypes.byref(r), ctypes.byref(c), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc != 0, what
        assert len(err.strip().splitlines()) == 1 and "photon_piv_correlate_weighted" in err, (what, err)
        assert r.value == -5 and c.value == -5, what
        assert (vec == 7.0).all().item() and (flg == 7).all().item(), what
    r, c = ctypes.c_int(-5), ctypes.c_int(-5)                   # d_vectors without d_flags
    assert L.photon_piv_correlate_weighted(p, p, t, 80, 64, 16, 8, 4, None, ctypes.c_void_p(vec.data_ptr()), None, None, ctypes.byref(r),
                                           ctypes.byref(c), None) != 0
    torch.cuda.synchronize()
    assert len(capfd.readouterr().err.strip().splitlines()) == 1 and r.value == -5 and (vec == 7.0).all().item()
    r, c = ctypes.c_int(0), ctypes.c_int(0)                     # the size query
    assert L.photon_piv_correlate_weighted(p, p, t, 80, 64, 16, 8, 4, None, None, None, None, ctypes.byref(r), ctypes.byref(c), None) == 0
    assert (r.value, c.value) == ((64 - 16) // 8 + 1, (80 - 16) // 8 + 1)
    assert capfd.readouterr().err == ""
    assert (vec == 7.0).all().item() and (flg == 7).all().item()


def test_the_helpers_table_is_window_weights_bit_for_bit(photon, capfd):
    for win in pc.WINDOW_SIZES:
        for sigma in (None, 3.3, 0.7, 100.0):
            got, want = photon.piv_window_weights(win, "gaussian", sigma), pw.window_weights(win, "gaussian", sigma)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (win, sigma)
        assert photon.piv_window_weights(win, "uniform").tobytes() == pw.window_weights(win, "uniform").tobytes()
    out = np.full((16, 16), 7.0, np.float32)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    capfd.readouterr()
    for what, args in (("win", (24, 1, 4.0, ptr)), ("kind", (16, 2, 4.0, ptr)), ("kind", (16, -1, 4.0, ptr)), ("sigma 0", (16, 1, 0.0, ptr)),
                       ("sigma < 0", (16, 1, -2.0, ptr)), ("sigma nan", (16, 1, float("nan"), ptr)), ("sigma inf", (16, 1, float("inf"), ptr)),
                       ("null", (16, 1, 4.0, None))):
        assert photon.lib.photon_piv_window_weights(*args) != 0, what
        err = capfd.readouterr().err
        assert len(err.strip().splitlines()) == 1 and "photon_piv_window_weights" in err, (what, err)
        assert (out == 7.0).all(), what


# ---- 6. the drivers ---------------------------------------------------------------------------------------------------------------
def test_the_drivers_with_a_gaussian_window_hold_their_models(photon):
    """correlate, correlate_deform (3 iterations) and correlate_multigrid ((32, 16) -> (16, 8)) on a 97 x 130 pair: the RMS
    error against the truth within 0.02 px of the model's, test_piv_deformation_gpu's bound."""
    im1, im2 = (np.array(c) for c in cases.driver_pair())
    models = cases.driver_models()
    got = {"correlate": (photon.correlate(im1, im2, 32, 16, weighting="gaussian"), 32, 16),
           "correlate_deform": (photon.correlate_deform(im1, im2, **cases.DEFORM, weighting="gaussian"), 32, 16),
           "correlate_multigrid": (photon.correlate_multigrid(im1, im2, **cases.MULTIGRID, weighting="gaussian"), 16, 8)}
    for name, ((vec, status), win, step) in got.items():
        rms, model = cases.driver_rms(vec, win, step), cases.driver_rms(models[name][0], win, step)
        print(f"{name}: device {rms:.4f} px, model {model:.4f} px")
        assert vec.shape == models[name][0].shape
        assert abs(rms - model) <= 0.02, name
    plain = photon.correlate(im1, im2, 32, 16)                      # the table is in use: other vectors than section 5's
    assert not np.array_equal(got["correlate"][0][0], plain[0], equal_nan=True)
    # the forms of the keyword
    table = pw.window_weights(32)
    assert_same_bits(photon.correlate(im1, im2, 32, 16, weighting=table), got["correlate"][0])
    assert_same_bits(photon.correlate(im1, im2, 32, 16, weighting=("gaussian", 8.0)), got["correlate"][0])
    assert_same_bits(photon.correlate_deform(im1, im2, **cases.DEFORM, weighting=table), got["correlate_deform"][0])
    assert_same_bits(photon.correlate(im1, im2, 32, 16, weighting="uniform"), plain)
    import torch
    smoothed = photon.correlation_predictor(im1, im2, weighting="gaussian")
    torch.cuda.synchronize()
    assert np.isfinite(smoothed.cpu().numpy()).all() and tuple(smoothed.shape) == got["correlate"][0][0].shape[:2] + (2,)


def test_weighting_none_and_the_refusals_of_the_keyword(photon):
    import torch
    im1, im2 = (np.array(c) for c in cases.driver_pair())
    for call, kw in ((photon.correlate, dict(win=32, step=16, passes=2)), (photon.correlate_deform, cases.DEFORM),
                     (photon.correlate_multigrid, cases.MULTIGRID)):
        assert_same_bits(call(im1, im2, **kw, weighting=None), call(im1, im2, **kw))
    a, b = photon.correlation_predictor(im1, im2), photon.correlation_predictor(im1, im2, weighting=None)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    mask = np.zeros(im1.shape, bool)
    for call, kw in ((photon.correlate, dict(win=32, step=16)), (photon.correlate_deform, cases.DEFORM),
                     (photon.correlate_multigrid, cases.MULTIGRID), (photon.correlation_predictor, {})):
        with pytest.raises(ValueError, match="window_sigma"):
            call(im1, im2, **kw, method="phase", weighting="gaussian")
        with pytest.raises(ValueError, match="mask"):
            call(im1, im2, **kw, mask=mask, weighting="gaussian")
        with pytest.raises(ValueError, match="negative"):
            call(im1, im2, **kw, weighting=-np.ones((32, 32)))
    with pytest.raises(ValueError, match="shape"):               # an array has one win: the second level has another
        photon.correlate_multigrid(im1, im2, **cases.MULTIGRID, weighting=pw.window_weights(32))


# ---- 7. the response study on the device --------------------------------------------------------------------------------------------
def test_the_response_to_wavelengths_near_the_window_size(photon):
    """The study of tests/test_piv_weighting.py at seed 1 through PhotonLibrary.correlate_deform: pass 0 and six iterations,
    top hat and Gaussian window, at 24 and 40 px."""
    uniform, gaussian = {}, {}
    for lam in cases.WAVELENGTHS:
        im1, im2 = (np.array(c) for c in cases.response_pair(lam, 1))
        for out, weighting in ((uniform, None), (gaussian, "gaussian")):
            amps = tuple(cases.amplitude(photon.correlate_deform(im1, im2, **cases.R_ARGS, iterations=n, weighting=weighting)[0], lam)
                         for n in range(cases.R_ITERATIONS + 1))
            model = cases.model_response(lam, 1, weighting)
            print(f"lambda {lam}, {weighting or 'uniform'}: device {amps[0]:+.4f} -> {amps[-1]:+.4f}, device - model "
                  f"{amps[0] - model[0]:+.1e} -> {amps[-1] - model[-1]:+.1e}")
            out[lam] = amps
    cases.assert_response(uniform, gaussian)
