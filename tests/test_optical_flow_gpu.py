"""Dense optical flow on the device (include/parallel_ray_tracing.h, section 12): the per-pixel warp against the grid warp,
the data terms and the fused sweeps against their f32 models bit for bit, repeat bits, refusals, the driver against its
parts and against analytic truth, and the flow in the BOS loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import bos_density_cases as bc
import optical_flow_cases as oc
import piv_deformation_cases as dc
from conftest import ROOT
from photon_amd import bos_density as bd
from photon_amd import optical_flow as of
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from test_bos_density_gpu import BOUND_CORRELATED, blob_pairs, check  # noqa: F401  (blob_pairs: the fixture)
from test_piv_deformation_gpu import (FAR_SCALES, SMALL_SHAPES, TOL, device_coefficients, device_deform, exact_shift, far_dense_fields,
                                      far_taps, image, random_image)

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tile_shape():
    """(kTileY, kTileX) of sweep_kernel, from the source."""
    with open(os.path.join(ROOT, "photon_amd", "csrc", "photon_optflow.hip")) as f:
        text = f.read()
    return tuple(int(re.search(rf"#define PHOTON_OPTFLOW_TILE_{a} (\d+)", text).group(1)) for a in "YX")


def device_dense(photon, field, shape, win, step):
    import torch
    f = cuda(field)
    dense = torch.full((*shape, 2), -77.0, dtype=torch.float32, device="cuda")
    photon.field_to_pixels(f.data_ptr(), field.shape[2], field.shape[0], field.shape[1], win, step, shape[1], shape[0], dense.data_ptr())
    torch.cuda.synchronize()
    return dense.cpu().numpy()


def device_deform_dense(photon, coef, dense, scale):
    import torch
    c, d = cuda(coef), cuda(dense)
    out = torch.full(coef.shape, -77.0, dtype=torch.float32, device="cuda")
    photon.piv_deform_dense(c.data_ptr(), coef.shape[1], coef.shape[0], d.data_ptr(), scale, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_terms(photon, w1, w2, u0, gain, alpha2):
    import torch
    a, b = cuda(w1), cuda(w2)
    u = cuda(u0) if u0 is not None else None
    t = torch.full((*w1.shape, 4), -77.0, dtype=torch.float32, device="cuda")
    photon.optflow_terms(a.data_ptr(), b.data_ptr(), w1.shape[1], w1.shape[0], u.data_ptr() if u is not None else 0, gain, alpha2, t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()


def device_iterate(photon, terms, u, n, with_tmp=True):
    import torch
    t, d_u = cuda(terms), cuda(u)
    out = torch.full(u.shape, -77.0, dtype=torch.float32, device="cuda")
    tmp = torch.full(u.shape, -77.0, dtype=torch.float32, device="cuda") if with_tmp else None
    photon.optflow_iterate(t.data_ptr(), d_u.data_ptr(), u.shape[1], u.shape[0], n, out.data_ptr(), tmp.data_ptr() if with_tmp else 0)
    torch.cuda.synchronize()
    assert d_u.cpu().numpy().tobytes() == u.tobytes() and t.cpu().numpy().tobytes() == terms.tobytes()      # inputs untouched
    return out.cpu().numpy()


# ---- a, b: the per-pixel warp is the grid warp ------------------------------------------------------------------------------
WARP_CASES = [((97, 130), 32, 16), ((64, 64), 16, 8), ((16, 40), 16, 8)]


@pytest.mark.parametrize("shape,win,step", WARP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_dense_warp_equals_the_grid_warp_bit_for_bit(photon, shape, win, step):
    coef = device_coefficients(photon, image(shape, 3))
    for cols in (2, 4):
        field = oc.random_grid_field(shape, win, step, 10 + cols, nan_at=(0, 1), cols=cols)
        assert np.isnan(field).any()
        dense = device_dense(photon, field, shape, win, step)
        assert np.isfinite(dense).all()
        want = pd.dense_field(field, shape, win, step)
        print(f"{shape} win {win}: |device dense - f64 dense_field| = {np.abs(dense - want).max():.3g}")
        assert np.abs(dense - want).max() <= 1e-6
        for scale in (-0.5, 0.5, 0.0):
            assert device_deform_dense(photon, coef, dense, scale).tobytes() == device_deform(photon, coef, field, win, step, scale).tobytes()


@pytest.mark.parametrize("shape", SMALL_SHAPES + [(37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_warp_far_from_the_image_matches_the_model(photon, shape):
    """Sides from 1 pixel, shifts from a few pixels to beyond the clamp at 2^24: deform_kernel's clamp, and mirror_far for the
    taps one reflection does not bring back, against the f64 model at the bar of the grid warp."""
    im = random_image(shape, 7 * shape[0] + shape[1])
    coef = pd.bspline_coefficients_model(im).astype(np.float32)             # both sides read the same f32 coefficients
    zero = device_deform_dense(photon, coef, np.zeros((*shape, 2), np.float32), 1.0)
    assert np.abs(zero - im).max() <= TOL * np.abs(im).max()
    fields = far_dense_fields(shape, 11 * shape[0] + shape[1])
    for scale in FAR_SCALES:
        clamped = far = False
        for dense in fields:
            c, f = far_taps(exact_shift(dense, scale), shape)
            clamped, far = clamped or c, far or f
            want = pd.deform_dense_model(coef, dense, scale)
            assert np.isfinite(want).all()
            got = device_deform_dense(photon, coef, dense, scale)
            err = float(np.abs(got - want).max() / np.abs(im).max())
            print(f"dense warp {shape}, scale {scale}, |D| up to {np.abs(dense).max():.3g}: max |device - model| = {err:.2e} of max |im|")
            assert (got != -77.0).all() and err <= TOL, (shape, scale, err)
        assert clamped and far, (shape, scale)


# ---- c: the data terms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_terms_equal_the_model_bit_for_bit(photon, shape):
    w1, w2, u0 = oc.random_pair(shape, 21)
    gain = float(np.float32(1.0 / max(float(w1.std()), 1.0)))
    for field in (u0, None):
        want = of.terms_model(w1, w2, field, gain, oc.ALPHA2)
        assert np.isfinite(want).all()
        assert device_terms(photon, w1, w2, field, gain, oc.ALPHA2).tobytes() == want.tobytes(), field is None


# ---- d: the sweeps ------------------------------------------------------------------------------------------------------------
def sweep_shapes():
    ty, tx = tile_shape()
    big = (2 * ty + 3, 2 * tx + 9)              # sides of more than two tiles plus one pixel: nine workgroups, the last ones narrow
    assert max(big) <= 300
    # one tile exactly, one tile plus a pixel down and less a pixel across, two tiles by two tiles plus a pixel
    return oc.SHAPES + [big, (ty, tx), (ty + 1, tx - 1), (2 * ty, 2 * tx + 1)]


def model_chain(terms, u, counts):
    """{n: iterate_model(terms, u, n)} for the counts: one chain of model sweeps serves them all."""
    model, done = {0: u}, 0
    for n in sorted(set(counts) - {0}):
        model[n] = of.iterate_model(terms, model[done], n - done)
        done = n
    return model


@pytest.mark.parametrize("shape", sweep_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_sweeps_equal_the_model_bit_for_bit(photon, shape):
    T = photon.optflow_iterations_per_launch()
    assert 1 <= T <= 64
    terms, u = oc.random_terms(shape, 31)
    counts = sorted({0, 1, T - 1, T, T + 1, 2 * T + 3})
    model = model_chain(terms, u, counts)
    for n in counts:
        got = device_iterate(photon, terms, u, n)
        assert got.tobytes() == model[n].tobytes(), (shape, n, float(np.abs(got - model[n]).max()))
        if n <= T:
            assert device_iterate(photon, terms, u, n, with_tmp=False).tobytes() == model[n].tobytes(), (shape, n)
    assert device_iterate(photon, terms, u, 0).tobytes() == u.tobytes()


@pytest.mark.parametrize("shape", sweep_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_sweep_kernel_equals_the_model_bit_for_bit(photon, shape, monkeypatch):
    """n = 0 .. T at the default T: count n is one launch of sweep_kernel<n>, so every instantiation (and with it every
    thread arrangement: K = 3, 4 and 5 rows per thread) runs, with and without d_tmp."""
    monkeypatch.delenv("PHOTON_OPTFLOW_SWEEPS", raising=False)
    T = photon.optflow_iterations_per_launch()
    assert T == 8                               # sweep_kernel<1 .. 8>: a new default changes what this test covers
    terms, u = oc.random_terms(shape, 32)
    model = model_chain(terms, u, range(T + 1))
    for n in range(T + 1):
        for with_tmp in (True, False):
            got = device_iterate(photon, terms, u, n, with_tmp=with_tmp)
            assert got.tobytes() == model[n].tobytes(), (shape, n, with_tmp, float(np.abs(got - model[n]).max()))


@pytest.mark.parametrize("t", range(1, 8))
def test_every_launch_size_equals_the_model_bit_for_bit(photon, monkeypatch, t):
    """PHOTON_OPTFLOW_SWEEPS = t: 1 to 4 launches (both parities of the d_tmp / d_out alternation), with a remainder launch
    of every size from 1 to t."""
    monkeypatch.setenv("PHOTON_OPTFLOW_SWEEPS", str(t))
    assert photon.optflow_iterations_per_launch() == t
    counts = sorted({t, t + 1, 2 * t, 2 * t + 1, 3 * t + 2})
    for shape in (sweep_shapes()[len(oc.SHAPES)], (3, 4)):
        terms, u = oc.random_terms(shape, 33)
        model = model_chain(terms, u, counts)
        for n in counts:
            got = device_iterate(photon, terms, u, n)
            assert got.tobytes() == model[n].tobytes(), (t, shape, n, float(np.abs(got - model[n]).max()))
        assert device_iterate(photon, terms, u, t, with_tmp=False).tobytes() == model[t].tobytes()


@pytest.mark.parametrize("value", ["0", "9", "-1", "x"])
def test_a_sweep_count_out_of_range_gives_the_default(photon, monkeypatch, value):
    monkeypatch.delenv("PHOTON_OPTFLOW_SWEEPS", raising=False)
    default = photon.optflow_iterations_per_launch()
    monkeypatch.setenv("PHOTON_OPTFLOW_SWEEPS", value)
    assert photon.optflow_iterations_per_launch() == default == 8
    terms, u = oc.random_terms((37, 53), 34)    # the call reads the variable as the query does: `default` sweeps need no d_tmp
    assert device_iterate(photon, terms, u, default, with_tmp=False).tobytes() == of.iterate_model(terms, u, default).tobytes()


def test_identical_frames_keep_a_constant_field_on_the_device(photon):
    w1, _, _ = oc.random_pair((37, 53), 5)
    u0 = np.empty((37, 53, 2), np.float32)
    u0[...] = (np.float32(1.2345678), np.float32(-0.7654321))
    terms = device_terms(photon, w1, w1, u0, 1.0 / float(w1.std()), oc.ALPHA2)
    T = photon.optflow_iterations_per_launch()
    assert device_iterate(photon, terms, u0, T + 1).tobytes() == u0.tobytes()


def test_two_calls_return_identical_bits(photon):
    shape = (130, 97)
    w1, w2, u0 = oc.random_pair(shape, 8)
    terms, u = oc.random_terms(shape, 9)
    T = photon.optflow_iterations_per_launch()
    field = oc.random_grid_field(shape, 32, 16, 12)
    coef = device_coefficients(photon, w1)
    for run in (lambda: device_terms(photon, w1, w2, u0, 0.01, oc.ALPHA2), lambda: device_iterate(photon, terms, u, 2 * T + 1),
                lambda: device_dense(photon, field, shape, 32, 16), lambda: device_deform_dense(photon, coef, u0, 0.5)):
        assert run().tobytes() == run().tobytes()
    im1, im2 = oc.pair32("vortex", 1)
    x, y = (photon.optical_flow(im1, im2, win=dc.WIN, step=dc.STEP, warps=2, iterations=T + 2) for _ in range(2))
    assert x.tobytes() == y.tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    T = photon.optflow_iterations_per_launch()
    h, w, win, step = 64, 80, 16, 8
    r, c = pc.grid_shape((h, w), win, step)
    im, im2 = torch.rand((h, w), device="cuda"), torch.rand((h, w), device="cuda")
    fld = torch.zeros((r, c, 4), device="cuda")
    u = torch.zeros((h, w, 2), device="cuda")
    tm = torch.rand((h, w, 4), device="cuda")
    outs = dict(dense=torch.full((h, w, 2), -77.0, device="cuda"), image=torch.full((h, w), -77.0, device="cuda"),
                terms=torch.full((h, w, 4), -77.0, device="cuda"), field=torch.full((h, w, 2), -77.0, device="cuda"),
                tmp=torch.full((h, w, 2), -77.0, device="cuda"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    nan, inf = float("nan"), float("inf")
    capfd.readouterr()

    def refused(name, what, rc):
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, (name, what, rc)
        assert len(err.strip().splitlines()) == 1 and f"photon: {name}:" in err, (name, what, err)
        assert all((t == -77.0).all().item() for t in outs.values()), (name, what)

    def each(name, ok, changes):
        for what, change in changes:
            refused(name, what, getattr(L, name)(*[change.get(k, v) for k, v in enumerate(ok)], None))

    ok_a = (p(fld), 4, r, c, win, step, w, h, p(outs["dense"]))
    each("photon_piv_field_to_pixels", ok_a,
         (("null field", {0: None}), ("null output", {8: None}), ("stride 3", {1: 3}), ("grid rows", {2: r + 1}), ("grid columns", {3: c - 1}),
          ("win 24", {4: 24}), ("step 0", {5: 0}), ("image too small", {7: 15})))
    ok_b = (p(im), w, h, p(u), 0.5, p(outs["image"]))
    each("photon_piv_deform_dense", ok_b,
         (("null coefficients", {0: None}), ("null field", {3: None}), ("null output", {5: None}), ("width 0", {1: 0}), ("height 0", {2: 0}),
          ("side above 2^22", {1: (1 << 22) + 1}), ("scale nan", {4: nan}), ("scale inf", {4: inf}), ("in place", {0: p(outs["image"])})))
    ok_c = (p(im), p(im2), w, h, p(u), 0.7, 5.0, p(outs["terms"]))
    each("photon_optflow_terms", ok_c,
         (("null w1", {0: None}), ("null w2", {1: None}), ("null terms", {7: None}), ("width 0", {2: 0}), ("height -1", {3: -1}),
          ("gain 0", {5: 0.0}), ("gain < 0", {5: -1.0}), ("gain nan", {5: nan}), ("gain inf", {5: inf}), ("alpha2 0", {6: 0.0}),
          ("alpha2 nan", {6: nan}), ("alpha2 inf", {6: inf})))
    ok_d = (p(tm), p(u), w, h, T + 1, p(outs["field"]), p(outs["tmp"]))
    each("photon_optflow_iterate", ok_d,
         (("null terms", {0: None}), ("null u", {1: None}), ("null output", {5: None}), ("width 0", {2: 0}), ("height 0", {3: 0}),
          ("iterations < 0", {4: -1}), ("in place", {1: p(outs["field"])}), ("tmp is u", {6: p(u)}), ("tmp is the output", {6: p(outs["field"])}),
          ("no tmp above T", {6: None}), ("in place, no sweeps", {1: p(outs["field"]), 4: 0})))

    # accepted calls are silent and fill their outputs; d_u0 and (up to T sweeps) d_tmp may be NULL
    assert L.photon_piv_field_to_pixels(*ok_a, None) == 0 and L.photon_piv_deform_dense(*ok_b, None) == 0
    assert L.photon_optflow_terms(*[{4: None}.get(k, v) for k, v in enumerate(ok_c)], None) == 0
    assert L.photon_optflow_iterate(*[{4: T, 6: None}.get(k, v) for k, v in enumerate(ok_d)], None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == ""
    assert all(not (outs[k] == -77.0).any().item() for k in ("dense", "image", "terms", "field")) and (outs["tmp"] == -77.0).all().item()
    assert L.photon_optflow_iterate(*ok_d, None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == "" and not (outs["tmp"] == -77.0).any().item()


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def parts(photon, im1, im2, dense0, alpha2, warps, iterations):
    """The driver's calls one by one on a dense start (a device tensor [h, w, 2])."""
    import torch
    h, w = im1.shape
    a, b = cuda(im1), cuda(im2)
    gain = float(1.0 / torch.std(a, correction=0))
    coef, warped = torch.empty((2, h, w), device="cuda"), torch.empty((2, h, w), device="cuda")
    terms, tmp = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w, 2), device="cuda")
    u = dense0.clone()
    photon.bspline_coefficients(a.data_ptr(), w, h, coef[0].data_ptr())
    photon.bspline_coefficients(b.data_ptr(), w, h, coef[1].data_ptr())
    for _ in range(warps):
        nxt = torch.empty_like(u)
        photon.piv_deform_dense(coef[0].data_ptr(), w, h, u.data_ptr(), -0.5, warped[0].data_ptr())
        photon.piv_deform_dense(coef[1].data_ptr(), w, h, u.data_ptr(), 0.5, warped[1].data_ptr())
        photon.optflow_terms(warped[0].data_ptr(), warped[1].data_ptr(), w, h, u.data_ptr(), gain, alpha2, terms.data_ptr())
        photon.optflow_iterate(terms.data_ptr(), u.data_ptr(), w, h, iterations, nxt.data_ptr(), tmp.data_ptr())
        u = nxt
    torch.cuda.synchronize()
    return u.cpu().numpy()


def test_the_driver_equals_its_parts(photon):
    import torch
    shape, win, step = (97, 130), 32, 16
    im1, im2 = (a.astype(np.float32) for a in dc.pair("rotation", 2, shape))
    T = photon.optflow_iterations_per_launch()
    grid = np.nan_to_num(oc.random_grid_field(shape, win, step, 3, cols=4)) * np.float32(0.3)
    dense0 = cuda(device_dense(photon, grid, shape, win, step))
    want = parts(photon, im1, im2, dense0, 2.0, 2, T + 3)
    for predictor in (grid, cuda(grid), dense0):
        got, at_centres = photon.optical_flow(im1, im2, predictor, win, step, alpha2=2.0, warps=2, iterations=T + 3, return_grid=True)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert np.array_equal(at_centres, of.sample_at_window_centres(want, win, step))
    assert photon.optical_flow(im1, im2, dense0, win, step, warps=0).tobytes() == dense0.cpu().numpy().tobytes()
    r, c = pc.grid_shape(shape, win, step)
    for bad in (np.zeros((r + 1, c, 2), np.float32), np.zeros((r, c), np.float32), np.zeros((r, c, 1), np.float32),
                torch.zeros((shape[0], shape[1] - 1, 2), device="cuda"), np.zeros((shape[0], shape[1], 3), np.float32)):
        with pytest.raises(ValueError):
            photon.optical_flow(im1, im2, bad, win, step)
    with pytest.raises(ValueError):
        photon.optical_flow(im1, im2, grid, win, step, alpha2=0.0)


def test_the_device_meets_the_models_bounds(photon):
    """Every field, seeds 1 - 5, the default driver from its own predictor (one iteration of correlate_deform)."""
    rows = []
    for kind in oc.KINDS:
        for seed in dc.SEEDS:
            im1, im2 = oc.pair32(kind, seed)
            pred, _ = photon.correlate_deform(im1, im2, dc.WIN, dc.STEP, iterations=1)
            dense = pd.dense_field(pred, im1.shape, dc.WIN, dc.STEP)
            flow = photon.optical_flow(im1, im2, win=dc.WIN, step=dc.STEP, alpha2=oc.ALPHA2, warps=oc.WARPS, iterations=oc.ITERATIONS)
            rows.append((kind, seed, oc.flow_rms(dense, kind), oc.flow_rms(flow, kind)))
    oc.print_table("PhotonLibrary.optical_flow from one iteration of correlate_deform", rows)
    for kind, seed, p, f in rows:
        assert f <= oc.DEVICE_BOUND[kind], (kind, seed, f, oc.DEVICE_BOUND[kind])
        assert f <= oc.RATIO_BOUND[kind] * p, (kind, seed, p, f)


def test_the_device_follows_the_model(photon):
    """One pair from the same dense predictor: the device differs from the model by the f32 warp alone."""
    im1, im2 = oc.pair32("vortex", 1)
    grid = pd.correlate_deform_model(im1, im2, dc.WIN, dc.STEP, iterations=1)[0][..., :2].astype(np.float32)
    got = photon.optical_flow(im1, im2, grid, dc.WIN, dc.STEP)
    want = of.optical_flow_model(im1, im2, grid, dc.WIN, dc.STEP)
    diff = float(np.abs(got - want).max())
    print(f"|device flow - model flow| = {diff:.3g} px")
    # The f32 warp sums 16 taps of coefficients up to about 1.5: errors of 16 x 2^-24 x 1.5 = 1.4e-6 in a pixel, 1e-5 in It
    # after the gain (1 / std of a particle image: about 7).  du = -It Ix / (alpha2 + |grad I|^2) is at most It / (2 sqrt(alpha2))
    # = 0.22 It at any gradient, and each warp starts from the images again (nothing accumulates beyond the field handed
    # on): 3 warps x 1e-5 px at the very most.
    assert diff <= 3e-5


# ---- the flow in the BOS loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_flow_of_a_rendered_pair_integrates_to_the_projection(photon, blob_pairs, diffraction):
    call, im1, im2, _, _ = blob_pairs[diffraction]
    phi, mid, st = bd.reconstruct_flow(photon, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    assert st["converged"] == 1
    check(f"optical flow, {'erf' if diffraction else '4-pixel'}", phi, call, BOUND_CORRELATED)
