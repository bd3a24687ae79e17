"""Iterative image-deformation correlation on the device (include/parallel_ray_tracing.h, section 7): every entry point
against its f64 model (photon_amd/piv_deformation.py), repeat bits, refusals, and PhotonLibrary.correlate_deform against
analytic truth, against correlate(passes=2) and against the clock."""
import ctypes
import time

import numpy as np
import pytest

import piv_deformation_cases as cs
import test_piv_correlation_gpu as base
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_pairs as pp
from photon_amd import scenes

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # of max |im|: the bar section 5 uses for its planes


def image(shape, seed):
    """Particles on a noise floor: sharp peaks and a gradient at every pixel."""
    rng = np.random.default_rng(seed)
    h, w = shape
    n = int(0.03 * h * w)
    im = pc.particle_image(shape, rng.uniform(0, w, n), rng.uniform(0, h, n), 2.5, rng.uniform(0.5, 1.0, n)) + 0.3 * rng.random(shape)
    return im.astype(np.float32)


def device_coefficients(photon, im):
    import torch
    a = torch.from_numpy(im).cuda()
    c = torch.empty_like(a)
    photon.bspline_coefficients(a.data_ptr(), im.shape[1], im.shape[0], c.data_ptr())
    torch.cuda.synchronize()
    return c.cpu().numpy()


def device_deform(photon, coef, field, win, step, scale):
    import torch
    c = torch.from_numpy(coef).cuda()
    f = torch.from_numpy(np.ascontiguousarray(field, np.float32)).cuda()
    out = torch.empty_like(c)
    photon.piv_deform(c.data_ptr(), coef.shape[1], coef.shape[0], f.data_ptr(), field.shape[-1], field.shape[0], field.shape[1], win, step,
                      scale, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_validate(photon, pred, vec, flags, smooth=True, eps=0.1, threshold=2.0):
    import torch
    r, c = flags.shape
    p = torch.from_numpy(pred).cuda() if pred is not None else None
    v, f = torch.from_numpy(vec).cuda(), torch.from_numpy(flags).cuda()
    field = torch.full((r, c, 2), -77.0, dtype=torch.float32, device="cuda")
    sm = torch.full((r, c, 2), -77.0, dtype=torch.float32, device="cuda")
    status = torch.full((r, c), -77, dtype=torch.int32, device="cuda")
    photon.piv_validate(p.data_ptr() if p is not None else 0, v.data_ptr(), f.data_ptr(), r, c, field.data_ptr(),
                        sm.data_ptr() if smooth else 0, status.data_ptr(), eps, threshold)
    torch.cuda.synchronize()
    return field.cpu().numpy(), sm.cpu().numpy(), status.cpu().numpy()


# ---- 5a. coefficients ----------------------------------------------------------------------------------------------------
SHAPES = [(64, 64), (97, 130), (130, 97), (256, 256), (1024, 1024)]


@pytest.mark.parametrize("shape", SHAPES + [(16, 16), (17, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_match_the_model(photon, shape):
    im = image(shape, shape[0] + shape[1])
    want = pd.bspline_coefficients_model(im)
    got = device_coefficients(photon, im)
    err = np.abs(got - want).max() / np.abs(im).max()
    print(f"coefficients {shape[0]} x {shape[1]}: max |device - model| = {err:.2e} of max |im|")
    assert err <= TOL


# sides below the 14-pixel halo of the filter: a halo index is reflected more than once (mirror_far), a side of 1 has no period
SMALL_SHAPES = [(1, 1), (1, 9), (9, 1), (3, 4), (14, 15), (15, 14), (2, 70)]
# The first tap that needs a second reflection lies n pixels from the nearest pixel and weighs |z|^n = 0.268^n: only on sides
# of 5 or less does a wrong second reflection move a coefficient by more than TOL.  The coefficient test adds these.
TINY_SHAPES = [(4, 3), (5, 2), (2, 5)]


def random_image(shape, seed):
    """Plain random f32 in [0, 1): image() places no particle on the smallest shapes."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


@pytest.mark.parametrize("shape", SMALL_SHAPES + TINY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_of_small_images_match_the_model(photon, shape):
    import torch
    im = random_image(shape, 100 * shape[0] + shape[1])
    want = pd.bspline_coefficients_model(im)
    assert np.isfinite(want).all()
    a = torch.from_numpy(im).cuda()
    c = torch.full(shape, -77.0, dtype=torch.float32, device="cuda")
    photon.bspline_coefficients(a.data_ptr(), shape[1], shape[0], c.data_ptr())
    torch.cuda.synchronize()
    got = c.cpu().numpy()
    err = np.abs(got - want).max() / np.abs(im).max()
    print(f"coefficients {shape[0]} x {shape[1]}: max |device - model| = {err:.2e} of max |im|")
    assert (got != -77.0).all() and err <= TOL
    if shape == (1, 1):
        assert abs(float(got[0, 0]) - float(im[0, 0])) <= TOL * float(im[0, 0])       # every tap is the one pixel: the filter's gain, 1


# ---- 5b. warp ------------------------------------------------------------------------------------------------------------
def field_of(kind, n_rows, n_cols, stride, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-3.0, 3.0, (n_rows, n_cols, stride)).astype(np.float32)     # (stride 4: peak and ratio are not read)
    if kind == "zero":
        f[..., :2] = 0.0
    elif kind == "constant":
        f[..., :2] = (7.3, -4.6)
    else:
        d = rng.uniform(-16.0, 16.0, (n_rows, n_cols, 2))
        f[..., :2] = d * np.minimum(1.0, 16.0 / np.maximum(np.hypot(d[..., 0], d[..., 1]), 1e-9))[..., None]      # |D| <= 16 px
        if kind == "nan":
            bad = rng.random((n_rows, n_cols)) < 0.15
            bad.flat[0] = True
            f[bad, rng.integers(0, 2, int(bad.sum()))] = np.nan
            f[rng.random((n_rows, n_cols)) < 0.05, 1] = np.inf
    return f


WARPS = [  # (shape, win, step, field, stride, scale)
    ((64, 64), 16, 8, "random", 2, -0.5), ((64, 64), 64, 64, "constant", 4, 0.5), ((64, 64), 32, 16, "zero", 2, 0.5),
    ((97, 130), 32, 16, "nan", 4, 0.5), ((97, 130), 16, 16, "zero", 4, -0.5), ((97, 130), 64, 20, "random", 2, 0.0),
    ((130, 97), 32, 32, "random", 2, 0.5), ((130, 97), 64, 24, "nan", 4, -0.5), ((130, 97), 16, 5, "constant", 2, 0.0),
    ((256, 256), 32, 16, "random", 4, -0.5), ((256, 256), 64, 32, "nan", 2, 0.5), ((256, 256), 16, 16, "random", 2, 1.0),
    ((1024, 1024), 32, 16, "random", 2, 0.5), ((1024, 1024), 16, 16, "constant", 4, -0.5), ((1024, 1024), 64, 64, "nan", 2, -0.5),
    ((64, 200), 64, 32, "random", 2, 0.5),          # a 1 x n grid
]


@pytest.mark.parametrize("case", WARPS, ids=[f"{c[0][0]}x{c[0][1]}_w{c[1]}_s{c[2]}_{c[3]}_stride{c[4]}_scale{c[5]}" for c in WARPS])
def test_warp_matches_the_model(photon, case):
    shape, win, step, kind, stride, scale = case
    im = image(shape, win + step)
    coef = pd.bspline_coefficients_model(im).astype(np.float32)             # both sides read the same f32 coefficients
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    field = field_of(kind, n_rows, n_cols, stride, seed=step)
    want = pd.deform_model(coef, field, win, step, scale)
    got = device_deform(photon, coef, field, win, step, scale)
    err = np.abs(got - want).max() / np.abs(im).max()
    print(f"warp {case}: max |device - model| = {err:.2e} of max |im|")
    assert err <= TOL
    if scale == 0.0 or kind == "zero":
        assert np.abs(got - im).max() <= TOL * np.abs(im).max()


def test_device_coefficients_and_zero_scale_return_the_image(photon):
    im = image((130, 97), 5)
    field = field_of("random", *pc.grid_shape(im.shape, 32, 16), 2, seed=1)
    got = device_deform(photon, device_coefficients(photon, im), field, 32, 16, 0.0)
    assert np.abs(got - im).max() <= TOL * np.abs(im).max()


# ---- 5b, far from the image: the clamp of scale D to 2^24 pixels and tap indices that one reflection does not bring back ----
FAR_SCALES = (1.0, -0.5)        # scale D is exact in f32 for every f32 D; 0.5 would be too, the existing WARPS hold it
BEYOND = (3.0e7, -5.0e7)        # past the clamp at scale 1.0; at -0.5 the second one still is


def exact_shift(d32, scale):
    """scale D as the device forms it (f32) and as the model does (f64): the test's fields must make them the same number."""
    assert d32.dtype == np.float32
    s32, s64 = np.float32(scale) * d32, float(scale) * d32.astype(np.float64)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)
    return s64


def far_taps(shift, shape):
    """(clamped, far) of shifts [h, w, 2] = (x, y) per pixel: whether any shift meets the clamp's far side, and whether any of
    the four tap indices per axis lies further than one reflection from the image (|i| > 2 (n - 1): piv_warp.hpp, mirror)."""
    s = np.clip(shift, -pd.MAX_SHIFT, pd.MAX_SHIFT)
    h, w = shape
    far = False
    for axis, n, at in ((0, w, np.arange(w)[None, :]), (1, h, np.arange(h)[:, None])):
        first = at + np.floor(s[..., axis]).astype(np.int64) - 1
        far = far or bool((np.abs(np.stack([first, first + 3])) > 2 * (n - 1)).any())
    return bool((np.abs(shift) > pd.MAX_SHIFT).any()), far


def far_dense_fields(shape, seed):
    """Per-pixel fields f32 [k, h, w, 2] in multiples of 1/8 pixel, magnitudes cycling through a few pixels, a few image
    widths, 1e3, 1e6 and the 64 pixels below 2^24, signs at random, plus the two entries of BEYOND; as many fields as it takes
    to hold each of these at least twice (one, unless the image has fewer than 7 pixels)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    n = 2 * h * w
    k = -(-14 // n)
    top = [4.0, 3.0 * max(h, w), 1.0e3, 1.0e6, 2.0 ** 24]
    low = [0.0, float(max(h, w)), 5.0e2, 5.0e5, 2.0 ** 24 - 64.0]
    cls = np.arange(k * n) % 5
    mag = np.round(8.0 * rng.uniform(np.take(low, cls), np.take(top, cls))) / 8.0
    mag = np.where(cls == 4, np.minimum(np.floor(mag), 2.0 ** 24 - 1.0), mag)    # just under 2^24 an f32 is a whole number
    d = mag * rng.choice([-1.0, 1.0], k * n)
    d[0], d[-1] = BEYOND
    d32 = d.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), d)                             # every value is an f32
    return d32.reshape(k, h, w, 2)


FAR_GRID_CASES = [((64, 64), 16, 8), ((97, 130), 32, 16)]
# constant fields (bilinear interpolation of equal nodes is exact: f32 and f64 agree on D).  2^24 - 0.5 is no f32 -- as one
# it is 2^24, the clamp itself --, so 2^24 - 1 stands beside it: the largest shift with a fraction (at scale -0.5).
FAR_GRID_VALUES = [(1000.25, -777.5), (2.0 ** 24 - 0.5, -(2.0 ** 24 - 0.5)), (2.0 ** 24 - 1.0, -(2.0 ** 24 - 1.0)), BEYOND]


@pytest.mark.parametrize("shape,win,step", FAR_GRID_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grid_warp_far_from_the_image_matches_the_model(photon, shape, win, step):
    import torch
    im = image(shape, win + step)
    coef = pd.bspline_coefficients_model(im).astype(np.float32)
    c = torch.from_numpy(coef).cuda()
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    worst = 0.0
    for value in FAR_GRID_VALUES:
        for stride in (2, 4):
            field = np.full((n_rows, n_cols, stride), 0.25, np.float32)
            field[..., :2] = value
            f = torch.from_numpy(field).cuda()
            for scale in FAR_SCALES:
                shift = np.broadcast_to(exact_shift(field[0, 0, :2], scale), (*shape, 2))
                clamped, far = far_taps(shift, shape)
                assert far and clamped == (value == BEYOND), (value, scale)
                want = pd.deform_model(coef, field, win, step, scale)
                assert np.isfinite(want).all()
                out = torch.full(shape, -77.0, dtype=torch.float32, device="cuda")
                photon.piv_deform(c.data_ptr(), shape[1], shape[0], f.data_ptr(), stride, n_rows, n_cols, win, step, scale, out.data_ptr())
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                err = float(np.abs(got - want).max() / np.abs(im).max())
                worst = max(worst, err)
                assert (got != -77.0).all() and err <= TOL, (value, stride, scale, err)
    print(f"grid warp {shape} win {win} step {step}, shifts up to the clamp: max |device - model| = {worst:.2e} of max |im|")


# ---- 5c. validate -------------------------------------------------------------------------------------------------------
def near_undecided(score):
    """Nodes within two nodes of a score the exclusion rule leaves out (a flipped decision moves its neighbours' medians)."""
    bad = ~cs.decided(score)
    out = np.zeros_like(bad)
    for i, j in np.argwhere(bad):
        out[max(i - 2, 0):i + 3, max(j - 2, 0):j + 3] = True
    return out


@pytest.mark.parametrize("case", cs.validate_cases(), ids=lambda c: f"{c[0]}x{c[1]}{'_pred' if c[3] else ''}")
def test_validate_is_bit_equal_to_the_model(photon, case):
    pred, vec, flags = cs.validate_case(*case)
    w_field, w_smooth, w_status, w_out, score = pd.validate_model(pred, vec, flags)
    keep = ~near_undecided(score)
    assert keep.mean() >= 0.975                                 # 0.1 % of the nodes at most, each with its 5 x 5 neighbourhood
    field, smooth, status = device_validate(photon, pred, vec, flags)
    assert np.array_equal(status[keep], w_status[keep]), np.argwhere(status != w_status)[:5]
    assert np.array_equal((status & 8) != 0, w_out) or not keep.all()
    assert field[keep].tobytes() == w_field[keep].tobytes(), np.argwhere((field != w_field).any(axis=-1))[:5]
    assert smooth[keep].tobytes() == w_smooth[keep].tobytes(), np.argwhere((smooth != w_smooth).any(axis=-1))[:5]
    field2, smooth2, status2 = device_validate(photon, pred, vec, flags, smooth=False)         # d_smooth NULL: the rest unchanged
    assert field2.tobytes() == field.tobytes() and status2.tobytes() == status.tobytes() and (smooth2 == -77.0).all()


def test_validate_with_other_eps_and_threshold(photon):
    pred, vec, flags = cs.validate_case(40, 33, 9)
    for eps, thr in ((0.0, 2.0), (0.3, 1.0), (0.05, 3.5)):
        w_field, w_smooth, w_status, _, score = pd.validate_model(pred, vec, flags, eps, thr)
        assert cs.decided(score, thr).all()
        field, smooth, status = device_validate(photon, pred, vec, flags, eps=eps, threshold=thr)
        assert np.array_equal(status, w_status)
        assert field.tobytes() == w_field.tobytes() and smooth.tobytes() == w_smooth.tobytes()


# ---- 6. repeat bits ------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bits(photon):
    im1, im2 = (c.astype(np.float32) for c in cs.pair("vortex", 2))
    a, b = device_coefficients(photon, im1), device_coefficients(photon, im1)
    assert a.tobytes() == b.tobytes()
    field = field_of("nan", *pc.grid_shape(im1.shape, 32, 16), 4, seed=3)
    a, b = (device_deform(photon, a, field, 32, 16, -0.5) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    pred, vec, flags = cs.validate_case(63, 63, 1)
    for x, y in zip(device_validate(photon, pred, vec, flags), device_validate(photon, pred, vec, flags)):
        assert x.tobytes() == y.tobytes()
    for smooth in (True, False):
        x, y = (photon.correlate_deform(im1, im2, 32, 16, 16, iterations=2, smooth=smooth) for _ in range(2))
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    h, w, win, step = 64, 80, 16, 8
    r, c = pc.grid_shape((h, w), win, step)
    im = torch.rand((h, w), device="cuda")
    out = torch.full((h, w), 7.0, device="cuda")
    fld = torch.zeros((r, c, 4), device="cuda")
    vec = torch.zeros((r, c, 4), device="cuda")
    flg = torch.zeros((r, c), dtype=torch.int32, device="cuda")
    f_out = torch.full((r, c, 2), 7.0, device="cuda")
    s_out = torch.full((r, c, 2), 7.0, device="cuda")
    st = torch.full((r, c), 7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    capfd.readouterr()

    def refused(name, what, rc):
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, (name, what, rc)
        assert len(err.strip().splitlines()) == 1 and name in err, (name, what, err)
        assert (out == 7.0).all().item() and (f_out == 7.0).all().item() and (s_out == 7.0).all().item() and (st == 7).all().item(), what

    for what, args in (("null image", (None, w, h, p(out))), ("null output", (p(im), w, h, None)), ("width 0", (p(im), 0, h, p(out))),
                       ("in place", (p(out), w, h, p(out)))):
        refused("photon_piv_bspline_coefficients", what, L.photon_piv_bspline_coefficients(*args, None))
    ok = (p(im), w, h, p(fld), 4, r, c, win, step, 0.5, p(out))
    for what, change in (("null coefficients", {0: None}), ("null field", {3: None}), ("null output", {10: None}), ("stride 3", {4: 3}),
                         ("grid rows", {5: r + 1}), ("grid columns", {6: c - 1}), ("win 24", {7: 24}), ("step 0", {8: 0}),
                         ("image too small", {2: 15}), ("scale nan", {9: float("nan")}), ("in place", {0: p(out)})):
        args = [change.get(k, v) for k, v in enumerate(ok)]
        refused("photon_piv_deform", what, L.photon_piv_deform(*args, None))
    ok = (None, p(vec), p(flg), r, c, 0.1, 2.0, p(f_out), p(s_out), p(st))
    for what, change in (("null vectors", {1: None}), ("null flags", {2: None}), ("null field", {7: None}), ("null status", {9: None}),
                         ("no rows", {3: 0}), ("eps < 0", {5: -0.1}), ("eps nan", {5: float("nan")}), ("threshold 0", {6: 0.0}),
                         ("threshold nan", {6: float("nan")}), ("pred is the field", {0: p(f_out)}), ("pred is smooth", {0: p(s_out)})):
        args = [change.get(k, v) for k, v in enumerate(ok)]
        refused("photon_piv_validate", what, L.photon_piv_validate(*args, None))
    assert L.photon_piv_validate(*ok, None) == 0 and L.photon_piv_deform(p(im), w, h, p(fld), 4, r, c, win, step, 0.5, p(out), None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == ""
    assert (st == 0).all().item() and not (out == 7.0).all().item()


# ---- 8. the driver against truth -----------------------------------------------------------------------------------------
def device_two_pass_rms(photon, im1, im2, kind):
    vec, _ = photon.correlate(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, passes=2)
    return cs.interior_rms(vec, kind)


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_vortex_pair_on_the_device(photon, seed):
    im1, im2 = (c.astype(np.float32) for c in cs.pair("vortex", seed))
    base_rms = device_two_pass_rms(photon, im1, im2, "vortex")
    vec, status = photon.correlate_deform(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=3)
    rms = cs.interior_rms(vec, "vortex")
    model = cs.interior_rms(pd.correlate_deform_model(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=3)[0], "vortex")
    peak = float(np.nanmedian(vec[1:-1, 1:-1, 2]))
    print(f"vortex seed {seed}: device two-pass {base_rms:.4f} px, 3 iterations {rms:.4f} px (model {model:.4f} px), median peak {peak:.3f}")
    assert rms <= 0.3 * base_rms
    assert abs(rms - model) <= 0.02
    assert peak >= 0.95


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_uniform_pair_on_the_device(photon, seed):
    im1, im2 = (c.astype(np.float32) for c in cs.pair("uniform", seed))
    base_rms = device_two_pass_rms(photon, im1, im2, "uniform")
    vec, _ = photon.correlate_deform(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=3)
    rms = cs.interior_rms(vec, "uniform")
    print(f"uniform seed {seed}: device two-pass {base_rms:.4f} px, 3 iterations {rms:.4f} px, ratio {rms / base_rms:.3f}")
    assert rms <= 1.5 * base_rms


def test_iterations_zero_is_one_pass_plus_validation(photon):
    im1, im2 = (c.astype(np.float32) for c in cs.pair("rotation", 3))
    vec, status = photon.correlate_deform(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, iterations=0)
    v1, f1 = photon.correlate(im1, im2, cs.WIN, cs.STEP, cs.RADIUS, passes=1)
    field, _, st, _, score = pd.validate_model(None, v1, f1)
    assert cs.decided(score).all()
    assert np.array_equal(vec[..., :2], field) and np.array_equal(status, st)
    assert vec[..., 2:].tobytes() == v1[..., 2:].tobytes()


# ---- 9. a rendered pair ----------------------------------------------------------------------------------------------------
def rendered_vortex_pair(photon, diffraction: bool, peak_px=5.0, core_px=30.0):
    """base.rendered_pair's camera and particle field (256^2 sensor, ~8000 particles), frame 2 advected through a Lamb-Oseen
    vortex about the optical axis: the sample pair of tools/piv_pair.py at test size."""
    import torch
    n, rays, pitch, n_pix = 8000, 400, 17.0, base.N_PIX
    geom = base.GEOM
    m0 = geom["image_distance"] / geom["object_distance"]
    half = 0.5 * n_pix * pitch / m0 * 1.05
    lo, hi = (-half, -half, -1.0e3), (half, half, 1.0e3)
    rc = core_px * pitch / m0
    gamma = (peak_px * pitch / m0) / pp.lamb_oseen_peak_speed(1.0, rc)
    grid = pp.lamb_oseen_vortex(gamma, rc, (0.0, 0.0), (-1.2 * half, -1.2 * half, -1.2e3), (1.2 * half, 1.2 * half, 1.2e3), (129, 129, 3))
    call = scenes.piv_scene(n_particles=n, rays_per_source=rays, mie=False, seed=4, n_pixels=n_pix)
    if diffraction:
        call.camera["implement_diffraction"] = True
        call.camera["diffraction_diameter"] = 2.5
    flow = photon.flow_from_grid(*grid)
    try:
        f1, w1 = photon.sources_piv_advected(21, n, lo, hi, geom["z_object"], 730.0, 1.0e4, flow=None, t=0.0, return_world=True)
        f2, w2 = photon.sources_piv_advected(21, n, lo, hi, geom["z_object"], 730.0, 1.0e4, flow=flow, t=1.0, return_world=True)
    finally:
        flow.free()
    images, recs = [], []
    for src in (f1, f2):
        scene = photon.scene_create_from_sources(call, src)
        img = torch.zeros(n_pix * n_pix, dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        try:
            scene.trace_moments(img.data_ptr(), rec.data_ptr())
            torch.cuda.synchronize()
        finally:
            scene.free()
            src.free()
        images.append(img.reshape(n_pix, n_pix))
        recs.append(rec.cpu().numpy())
    m = geom["image_distance"] / (geom["object_distance"] + w1[:, 2])
    return images[0], images[1], call, recs, -m[:, None] * (w2[:, :2] - w1[:, :2]) / pitch


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_rendered_vortex_pair_is_not_worse_than_two_passes(photon, diffraction):
    """Median and 95th percentile of |measured - window_truth| over the same windows of the same images, each method
    against the truth of the quantity its definition returns: section 5's vector is the shift of the pattern that lies in
    the window in FRAME 1 (im2(p + d) ~ im1(p)), so its truth collects the particles by their frame-1 centroid (what
    test_two_passes_are_no_worse_than_one and tools/piv_pair.py do); section 7 warps frame 1 by -F/2 and frame 2 by +F/2
    until they coincide, so F at a node is the shift of the particles that lie there HALF-WAY between the frames, and its
    truth collects them by that position (centroid + d/2).  Measured on the MI355X, median / 95th percentile in pixels:
      4-pixel splat: two passes 0.0607 / 0.5106 (against the half-way truth 0.0704 / 0.5778),
                     3 iterations 0.0542 / 0.4976 (against the frame-1 truth 0.0609 / 0.5662);
      erf splat:     two passes 0.0611 / 0.6831 (half-way truth 0.0666 / 0.7543),
                     3 iterations 0.0603 / 0.5077 (frame-1 truth 0.0705 / 0.5888).
    RMS over the windows 0.34 -> 0.19 px (4-pixel splat).  The gain is smaller than on the analytic pairs because this truth
    is itself a window average: around the core it differs from the local displacement, which deformation converges
    towards, by up to 0.3 px per component."""
    from photon_amd import deflections
    im1, im2, call, recs, predicted = rendered_vortex_pair(photon, diffraction)
    shape = (base.N_PIX, base.N_PIX)
    pos = pc.image_positions(deflections.to_pixels(deflections.dot_means(recs[0], call.lightray_number_per_particle, 1, "arrived")["pos"],
                                                   call.camera), call.camera)
    in_image = predicted * np.array([-1.0 if diffraction else 1.0, 1.0])       # (column, row) shift: the erf splat's columns are x-flipped
    truth_1, _ = pc.window_truth(pos, predicted, shape, base.WIN, base.STEP, 5)
    truth_mid, _ = pc.window_truth(pos + 0.5 * in_image, predicted, shape, base.WIN, base.STEP, 5)
    v2, f2 = photon.correlate(im1, im2, win=base.WIN, step=base.STEP, passes=2)
    vd, fd = photon.correlate_deform(im1, im2, win=base.WIN, step=base.STEP, iterations=3)
    use = np.isfinite(truth_1).all(axis=-1) & np.isfinite(truth_mid).all(axis=-1) & ((f2 & pc.FLAG_FLAT) == 0) & ((fd & pc.FLAG_FLAT) == 0)
    assert use.sum() >= 100

    def errors(vec, truth):
        return np.hypot(*(pc.sensor_displacements(vec, call.camera)[use] - truth[use]).T)

    e2, ed, e2_mid, ed_1 = errors(v2, truth_1), errors(vd, truth_mid), errors(v2, truth_mid), errors(vd, truth_1)
    print(f"{'erf' if diffraction else '4-pixel'} splat, {int(use.sum())} windows, |measured - truth| median / 95th percentile: "
          f"two passes {np.median(e2):.4f} / {np.percentile(e2, 95):.4f} px (half-way truth {np.median(e2_mid):.4f} / "
          f"{np.percentile(e2_mid, 95):.4f}), 3 deformation iterations {np.median(ed):.4f} / {np.percentile(ed, 95):.4f} px "
          f"(frame-1 truth {np.median(ed_1):.4f} / {np.percentile(ed_1, 95):.4f})")
    assert np.median(ed) <= np.median(e2)
    assert np.percentile(ed, 95) <= np.percentile(e2, 95)


# ---- 10. time --------------------------------------------------------------------------------------------------------------
def test_deformation_is_not_slower_than_two_passes_at_1024(photon):
    """A recorded measurement and a loose guard (a hidden synchronisation per iteration, a warp an order of magnitude off
    its byte floor): wall time of correlate_deform(iterations=3) <= 1.5 x correlate(passes=2), 1024^2, win 32 / step 16."""
    import torch
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    a, b = (torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6)))
    calls = {"deform": lambda: photon.correlate_deform(a, b, 32, 16, 16, iterations=3),
             "two_pass": lambda: photon.correlate(a, b, 32, 16, 16, passes=2)}
    times = {k: [] for k in calls}
    for rep in range(3 + 12):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append(1e3 * (time.perf_counter() - t0))
    t_deform, t_two = np.median(times["deform"]), np.median(times["two_pass"])
    print(f"1024^2, win 32 / step 16, medians of 12 alternating calls: correlate_deform(iterations=3) {t_deform:.3f} ms, "
          f"correlate(passes=2) {t_two:.3f} ms, ratio {t_deform / t_two:.3f}")
    assert t_deform <= 1.5 * t_two
