"""Multigrid window refinement on the device (include/parallel_ray_tracing.h, section 16): photon_piv_regrid against its f32
model bit for bit, its size query, repeat bits and refusals; PhotonLibrary.correlate_multigrid against the same chain
issued by hand, against correlate_deform, against its model and analytic truth, and into its downstream consumers."""
import ctypes

import numpy as np
import pytest

import piv_multigrid_cases as mc
from photon_amd import piv_correlation as pc
from photon_amd import piv_multigrid as pm

pytestmark = pytest.mark.gpu

POISON = -77.0


def raw_regrid(photon, field, shape, src, dst, out=None):
    """photon_piv_regrid through the C ABI into a poisoned buffer: (rc, out as numpy)."""
    import torch
    h, w = shape
    f = torch.from_numpy(np.ascontiguousarray(field)).cuda()
    if out is None:
        out = torch.full((*pc.grid_shape(shape, *dst), 2), POISON, dtype=torch.float32, device="cuda")
    rc = photon.lib.photon_piv_regrid(ctypes.c_void_p(f.data_ptr()), field.shape[2], field.shape[0], field.shape[1], *src, w, h, *dst,
                                      ctypes.c_void_p(out.data_ptr()), None, None, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


# ---- 1. the device against regrid_model, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.REGRID_CASES + mc.THIN_CASES, ids=mc.case_id)
def test_regrid_is_bit_equal_to_the_model(photon, case):
    shape, src, dst = case
    for stride in (2, 4):
        for bad in (0.0, 0.15):
            field = mc.random_field(shape, src, seed=shape[1] + src[1] + dst[1] + stride, stride=stride, bad=bad)
            want = pm.regrid_model(field, shape, src, dst)
            rc, got = raw_regrid(photon, field, shape, src, dst)
            assert rc == 0 and got.shape == want.shape
            assert got.tobytes() == want.tobytes(), (stride, bad, np.argwhere((got != want).any(axis=-1))[:5])


def test_regrid_of_one_node_and_of_the_same_grid(photon):
    one = np.array([[[3.25, -1.5, np.nan, 3.0e38]]], np.float32)
    rc, got = raw_regrid(photon, one, (64, 64), (64, 32), (16, 8))
    assert rc == 0 and got.shape == (7, 7, 2) and (got == one[0, 0, :2]).all()
    field = mc.random_field((200, 136), (16, 5), seed=5, stride=4)
    rc, got = raw_regrid(photon, field, (200, 136), (16, 5), (16, 5))
    assert rc == 0 and np.array_equal(got, field[..., :2])


def test_piv_regrid_returns_the_grid_s_tensor(photon):
    import torch
    shape, src, dst = (200, 136), (64, 32), (16, 8)
    field = mc.random_field(shape, src, seed=9)
    f = torch.from_numpy(field).cuda()
    out = photon.piv_regrid(f.data_ptr(), 2, field.shape[0], field.shape[1], *src, shape[1], shape[0], *dst)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (*pc.grid_shape(shape, *dst), 2) and out.dtype == torch.float32
    assert out.cpu().numpy().tobytes() == pm.regrid_model(field, shape, src, dst).tobytes()


# ---- 2. the size query -----------------------------------------------------------------------------------------------------
def test_size_query_fills_the_size_and_launches_nothing(photon):
    import torch
    shape, src, dst = (97, 130), (32, 16), (16, 5)
    h, w = shape
    field = torch.from_numpy(mc.random_field(shape, src, seed=1)).cuda()
    out = torch.full((*pc.grid_shape(shape, *dst), 2), POISON, dtype=torch.float32, device="cuda")
    args = (ctypes.c_void_p(field.data_ptr()), 2, field.shape[0], field.shape[1], *src, w, h, *dst, None)
    rows, cols = ctypes.c_int(-77), ctypes.c_int(-77)
    assert photon.lib.photon_piv_regrid(*args, ctypes.byref(rows), ctypes.byref(cols), None) == 0
    assert (rows.value, cols.value) == pc.grid_shape(shape, *dst) == tuple(out.shape[:2])
    rows, cols = ctypes.c_int(-77), ctypes.c_int(-77)
    assert photon.lib.photon_piv_regrid(*args, ctypes.byref(rows), None, None) == 0 and rows.value == out.shape[0]
    assert photon.lib.photon_piv_regrid(*args, None, ctypes.byref(cols), None) == 0 and cols.value == out.shape[1]
    assert photon.lib.photon_piv_regrid(*args, None, None, None) == 0
    torch.cuda.synchronize()
    assert (out == POISON).all().item()


# ---- 3. repeat bits --------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bits(photon):
    shape, src, dst = (200, 136), (32, 16), (16, 8)
    field = mc.random_field(shape, src, seed=2, stride=4, bad=0.15)
    (rc1, a), (rc2, b) = (raw_regrid(photon, field, shape, src, dst) for _ in range(2))
    assert rc1 == rc2 == 0 and (a != POISON).all() and a.tobytes() == b.tobytes()
    x, y = (photon.correlate_multigrid(*mc.pair(2), radius=24) for _ in range(2))
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    h, w, src, dst = 97, 130, (32, 16), (16, 8)
    r, c = pc.grid_shape((h, w), *src)
    fld = torch.zeros((r, c, 4), device="cuda")
    out = torch.full((*pc.grid_shape((h, w), *dst), 2), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    ok = (p(fld), 4, r, c, *src, w, h, *dst, p(out))
    big = (1 << 22) + 64                                            # win 64, step 2^22: a 1 x 2 grid of an image 2^22 + 64 wide
    cases = (("bad source win", {4: 24}, "win must be"), ("bad destination win", {8: 48}, "win must be"),
             ("source step 0", {5: 0}, "step must be"), ("destination step 0", {9: 0}, "step must be"),
             ("grid rows", {2: r + 1}, "not the window grid"), ("grid columns", {3: c - 1}, "not the window grid"),
             ("stride 3", {1: 3}, "src_stride"), ("image smaller than the source window", {7: 31}, "smaller than one window"),
             ("image smaller than the destination window", {8: 64, 6: 63, 3: 2}, "smaller than one window"),
             ("side above 2^22", {2: 1, 3: 2, 4: 64, 5: 1 << 22, 6: big, 7: 64, 8: 64, 9: 1 << 22}, "2^22"),
             ("null source", {0: None}, "null d_src"), ("in place", {0: p(out)}, "d_dst must not be d_src"))
    capfd.readouterr()
    for what, change, phrase in cases:
        rows, cols = ctypes.c_int(-77), ctypes.c_int(-77)
        rc = L.photon_piv_regrid(*[change.get(k, v) for k, v in enumerate(ok)], ctypes.byref(rows), ctypes.byref(cols), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, (what, rc)
        assert len(err.strip().splitlines()) == 1 and "photon_piv_regrid" in err and phrase in err, (what, err)
        assert (out == 7.0).all().item() and (rows.value, cols.value) == (-77, -77), what
    assert L.photon_piv_regrid(*ok, None, None, None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == "" and not (out == 7.0).any().item()


def test_the_driver_refuses_before_anything_is_queued(photon):
    im1, im2 = mc.pair(1)
    for change in (dict(schedule=()), dict(iterations=(1, 1)), dict(iterations=(1, 0, 2)), dict(radius=33), dict(residual_radius=9),
                   dict(method="phase", radius=None, residual_radius=8), dict(schedule=((64, 32), (24, 12), (16, 8)))):
        with pytest.raises(ValueError):
            photon.correlate_multigrid(im1, im2, **{**dict(radius=24), **change})
    with pytest.raises(ValueError):
        photon.correlate_multigrid(im1[:, :60], im2[:, :60], radius=24)


# ---- 5. the driver against its parts ---------------------------------------------------------------------------------------
def by_hand(photon, im1, im2, schedule, iterations, radius, residual_radius, method, smooth=True, eps=0.1, threshold=2.0):
    """correlate_multigrid's chain issued entry point by entry point on raw device pointers."""
    import torch
    a, b = torch.from_numpy(np.ascontiguousarray(im1)).cuda(), torch.from_numpy(np.ascontiguousarray(im2)).cuda()
    h, w = a.shape

    def correlate(x, y, win, step, rad):
        if method == "direct":
            return photon.piv_correlate(x.data_ptr(), y.data_ptr(), w, h, win, step, rad)[:2]
        return photon.piv_correlate_phase(x.data_ptr(), y.data_ptr(), w, h, win, step, rad, mode=1, window_sigma=win / 4.0, diameter=2.5)[:2]

    def validate(pred, vec, flg):
        r, c = flg.shape
        field, smoothed = (torch.full((r, c, 2), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
        status = torch.full((r, c), -77, dtype=torch.int32, device="cuda")
        photon.piv_validate(pred.data_ptr() if pred is not None else 0, vec.data_ptr(), flg.data_ptr(), r, c, field.data_ptr(),
                            smoothed.data_ptr(), status.data_ptr(), eps, threshold)
        return field, smoothed, status

    coef, warped = torch.empty((2, h, w), device="cuda"), torch.empty((2, h, w), device="cuda")
    photon.bspline_coefficients(a.data_ptr(), w, h, coef[0].data_ptr())
    photon.bspline_coefficients(b.data_ptr(), w, h, coef[1].data_ptr())
    for level, ((win, step), n) in enumerate(zip(schedule, iterations)):
        if level == 0:
            vec, flg = correlate(a, b, win, step, radius)
            field, smoothed, status = validate(None, vec, flg)
            pred = smoothed if smooth else field
        else:
            pw, ps = schedule[level - 1]
            pred = photon.piv_regrid(pred.data_ptr(), 2, pred.shape[0], pred.shape[1], pw, ps, w, h, win, step)
        r, c = pc.grid_shape((h, w), win, step)
        for _ in range(n):
            photon.piv_deform(coef[0].data_ptr(), w, h, pred.data_ptr(), 2, r, c, win, step, -0.5, warped[0].data_ptr())
            photon.piv_deform(coef[1].data_ptr(), w, h, pred.data_ptr(), 2, r, c, win, step, 0.5, warped[1].data_ptr())
            vec, flg = correlate(warped[0], warped[1], win, step, residual_radius)
            field, smoothed, status = validate(pred, vec, flg)
            pred = smoothed if smooth else field
    torch.cuda.synchronize()
    return torch.cat([field, vec[..., 2:4]], dim=-1).cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("method", mc.METHODS)
def test_the_driver_is_the_chain_of_its_parts(photon, method):
    im1, im2 = mc.pair(1)
    radius = {"direct": 24, "phase": 31}[method]
    want = by_hand(photon, im1, im2, mc.SCHEDULE, mc.ITERATIONS, radius, 4, method)
    got = photon.correlate_multigrid(im1, im2, radius=mc.RADIUS[method], method=method)
    assert got[0].shape == (*pc.grid_shape(mc.SHAPE, *mc.FINAL), 4) and got[1].shape == got[0].shape[:2]
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # levels that do not halve, a change of step alone, no iteration on level 0, the unsmoothed predictor
    schedule, iterations = ((32, 16), (32, 8), (16, 5)), (0, 1, 2)
    want = by_hand(photon, im1, im2, schedule, iterations, {"direct": 16, "phase": 15}[method], 3, method, smooth=False)
    got = photon.correlate_multigrid(im1, im2, schedule, iterations, residual_radius=3, smooth=False, method=method)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("method", mc.METHODS)
def test_a_one_level_schedule_is_correlate_deform(photon, method):
    im1, im2 = mc.pair(3)
    for win, step, iterations, smooth in ((64, 32, 2, True), (32, 16, 0, True), (16, 5, 1, False)):
        want = photon.correlate_deform(im1, im2, win, step, None, iterations=iterations, smooth=smooth, method=method)
        got = photon.correlate_multigrid(im1, im2, ((win, step),), (iterations,), smooth=smooth, method=method)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (win, step, iterations)


# ---- 6. the driver against its model and truth -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("seed", mc.SEEDS)
def test_multigrid_on_the_device_against_model_and_truth(photon, seed, method):
    """|RMS(device) - RMS(model)| <= 0.02 px (the bar correlate_deform is held to), the device's interior RMS on the final
    16 / 8 grid at most half of the device's correlate_deform(32, 16, iterations=3), at most 5 % of the nodes replaced."""
    im1, im2 = mc.pair(seed)
    vectors, status = photon.correlate_multigrid(im1, im2, mc.SCHEDULE, mc.ITERATIONS, radius=mc.RADIUS[method], method=method)
    base, _ = photon.correlate_deform(im1, im2, 32, 16, mc.BASE_RADIUS[method], iterations=3, method=method)
    rms, model = mc.interior_rms(vectors, mc.FINAL), mc.interior_rms(mc.model_multigrid(seed, method)[0], mc.FINAL)
    base_rms, share = mc.interior_rms(base, (32, 16)), mc.replaced_share(status)
    print(f"{method} seed {seed}: device multigrid {rms:.4f} px (model {model:.4f} px), {100 * share:.1f} % replaced; "
          f"device correlate_deform(32, 16, iterations=3) {base_rms:.4f} px; ratio {rms / base_rms:.3f}")
    assert abs(rms - model) <= 0.02
    assert rms <= 0.5 * base_rms
    assert share <= 0.05


# ---- 7. downstream consumers -----------------------------------------------------------------------------------------------
def test_the_result_feeds_uncertainty_and_optical_flow(photon):
    im1, im2 = mc.pair(1)
    win, step = mc.FINAL
    vectors, status = photon.correlate_multigrid(im1, im2, radius=24)
    sigma, flags = photon.displacement_uncertainty(im1, im2, vectors, win, step)
    assert sigma.shape == (*status.shape, 2) and flags.shape == status.shape
    print(f"sigma: median {np.median(sigma):.4f} px, flags set on {int((flags != 0).sum())} of {flags.size} nodes")
    assert np.isfinite(sigma).all()
    dense, grid = photon.optical_flow(im1, im2, predictor=vectors, win=win, step=step, return_grid=True)
    assert dense.shape == (*mc.SHAPE, 2) and grid.shape == (*status.shape, 2)
    assert np.isfinite(dense).all() and np.isfinite(grid).all()
