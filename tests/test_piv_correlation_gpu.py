"""photon_piv_correlate on the GPU (include/parallel_ray_tracing.h, section 5): planes, flags and vectors against the f64
host model of photon_amd/piv_correlation.py, bit-identical repeats, the refusals, and the axis mapping of a rendered PIV
pair through both sensor kernels."""
import ctypes

import numpy as np
import pytest

import piv_tail_cases
from photon_amd import piv_correlation as pc
from photon_amd import piv_pairs as pp
from photon_amd import scenes
from photon_amd.ray_tracing import single_lens_camera

pytestmark = pytest.mark.gpu

GEOM = single_lens_camera(lens_model="general", **scenes.SAMPLE_LENS)          # the camera of scenes.piv_scene


def particle_pair(shape, shift, seed, per_px=0.015, noise=0.02):
    rng = np.random.default_rng(seed)
    h, w = shape
    n = int(per_px * h * w)
    x, y = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n)
    amp = rng.uniform(0.5, 1.0, n)
    im1 = pc.particle_image(shape, x, y, 2.5, amp) + noise * rng.random(shape)
    im2 = pc.particle_image(shape, x + shift[0], y + shift[1], 2.5, amp) + noise * rng.random(shape)
    return im1.astype(np.float32), im2.astype(np.float32)


def device_correlate(photon, im1, im2, win, step, R, offset=None, planes=True):
    import torch
    a, b = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    off = torch.from_numpy(np.ascontiguousarray(offset, np.int32)).cuda() if offset is not None else None
    h, w = im1.shape
    vec, flg, pl = photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R, off.data_ptr() if off is not None else 0,
                                        planes=planes)
    torch.cuda.synchronize()
    return vec.cpu().numpy(), flg.cpu().numpy(), (pl.cpu().numpy() if planes else None)


CASES = [  # (win, R, step, (height, width), shift, with offsets)
    (16, 1, 8, (70, 90), (0.4, -0.3), False),
    (16, 4, 16, (64, 100), (2.3, 1.6), True),
    (16, 8, 5, (53, 61), (-3.2, 4.7), False),
    (32, 1, 32, (96, 130), (0.2, 0.6), False),
    (32, 8, 16, (100, 75), (-4.6, 2.2), True),
    (32, 16, 12, (150, 131), (7.4, -5.9), False),
    (32, 16, 32, (96, 160), (3.0, -2.0), True),
    (64, 1, 40, (150, 190), (-0.6, 0.3), False),
    (64, 16, 24, (130, 170), (5.5, 9.2), True),
    (64, 32, 64, (140, 200), (-12.3, 17.8), False),
]


@pytest.mark.parametrize("case", CASES, ids=[f"w{c[0]}_r{c[1]}_s{c[2]}_{c[3][0]}x{c[3][1]}{'_off' if c[5] else ''}" for c in CASES])
def test_device_matches_the_host_model(photon, case):
    win, R, step, shape, shift, with_off = case
    im1, im2 = particle_pair(shape, shift, seed=win * 100 + R + step)
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    off = None
    if with_off:
        off = np.random.default_rng(R).integers(-3, 4, size=(n_rows, n_cols, 2)).astype(np.int32)
    want = pc.correlate_model(im1, im2, win, step, R, offset=off, planes=True)
    assert (want[1] & pc.FLAG_OUTSIDE).any()                                       # windows that reach the image's edge
    clear = assert_close_to_the_host_model(device_correlate(photon, im1, im2, win, step, R, off), want)
    assert clear.mean() > 0.5


def assert_close_to_the_host_model(got, want):
    """The f32 device against the f64 model: flags equal, flat windows all NaN, planes within 1e-4 of the peak; and where the
    model's peak stands clear of its runner-up by 1e-3 of itself (returned, bool per live window), the same argmax, the
    vector within 1e-3 px, peak and 1 / ratio within 1e-4."""
    (got_v, got_f, got_p), (want_v, want_f, want_p) = got, want
    assert got_v.shape == want_v.shape and got_p.shape == want_p.shape
    assert np.array_equal(got_f, want_f), np.argwhere(got_f != want_f)[:5]
    flat = (want_f & pc.FLAG_FLAT) != 0
    assert np.isnan(got_v[flat]).all() and np.isnan(got_p[flat]).all()
    ok = ~flat
    n = int(ok.sum())
    pw, pg = want_p[ok].reshape(n, -1), got_p[ok].reshape(n, -1)
    peak = pw.max(axis=1)
    assert (np.abs(pg - pw).max(axis=1) <= 1e-4 * peak).all(), (np.abs(pg - pw).max(axis=1) / peak).max()
    srt = np.sort(pw, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-3 * peak
    assert np.array_equal(np.argmax(pg[clear], axis=1), np.argmax(pw[clear], axis=1))
    dv = np.abs(got_v[ok][clear, :2] - want_v[ok][clear, :2])
    assert dv.max() <= 1e-3, dv.max()
    np.testing.assert_allclose(got_v[ok][clear, 2], want_v[ok][clear, 2], rtol=1e-4)
    inv_g, inv_w = 1.0 / got_v[ok][clear, 3].astype(np.float64), 1.0 / want_v[ok][clear, 3]       # ratio: +inf -> 0
    assert np.abs(inv_g - inv_w).max() <= 1e-4
    return clear


def test_every_branch_of_the_peak_tail_in_nine_windows(photon):
    """Flat + outside, outside alone, a peak on the plane's edge + outside, and a clean window, in one launch."""
    im1, im2, _, _ = piv_tail_cases.nine_windows()
    want = pc.correlate_model(im1, im2, 16, 16, 4, planes=True)
    assert want[1].tolist() == [[6, 4, 5], [4, 0, 6], [5, 4, 4]]
    clear = assert_close_to_the_host_model(device_correlate(photon, im1, im2, 16, 16, 4), want)
    assert clear.all()                                          # (of the model: the smallest gap is 4e-3 of its peak)


def test_two_calls_return_identical_bits(photon):
    im1, im2 = particle_pair((1024, 1024), (3.3, -2.7), seed=5)
    for win, step, R in ((32, 16, 16), (64, 32, 32), (16, 8, 3)):
        a = device_correlate(photon, im1, im2, win, step, R)
        b = device_correlate(photon, im1, im2, win, step, R)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.rand((64, 80), device="cuda")
    vec = torch.full((64, 4), 7.0, device="cuda")
    flg = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(im.data_ptr())
    capfd.readouterr()
    for what, args in (("win 24", (p, p, 80, 64, 24, 8, 4)), ("win 128", (p, p, 80, 64, 128, 8, 4)),
                       ("R 0", (p, p, 80, 64, 16, 8, 0)), ("R > win/2", (p, p, 80, 64, 16, 8, 9)),
                       ("step 0", (p, p, 80, 64, 16, 0, 4)), ("image too small", (p, p, 80, 15, 16, 8, 4)),
                       ("null im1", (None, p, 80, 64, 16, 8, 4)), ("null im2", (p, None, 80, 64, 16, 8, 4))):
        r, c = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_correlate(*args, None, ctypes.c_void_p(vec.data_ptr()), ctypes.c_void_p(flg.data_ptr()), None,
                                    ctypes.byref(r), ctypes.byref(c), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc != 0, what
        assert len(err.strip().splitlines()) == 1 and "photon_piv_correlate" in err, (what, err)
        assert r.value == -5 and c.value == -5, what
        assert (vec == 7.0).all().item() and (flg == 7).all().item(), what
    r, c = ctypes.c_int(0), ctypes.c_int(0)                     # the size query
    assert L.photon_piv_correlate(p, p, 80, 64, 16, 8, 4, None, None, None, None, ctypes.byref(r), ctypes.byref(c), None) == 0
    assert (r.value, c.value) == ((64 - 16) // 8 + 1, (80 - 16) // 8 + 1)
    assert capfd.readouterr().err == ""


# ---- the axis mapping on a rendered pair ------------------------------------------------------------------------------
N_PIX, WIN, STEP = 256, 32, 16


def rendered_pair(photon, diffraction: bool, image_shift_px=(3.0, -2.0)):
    """A uniform world shift rendered through a reduced sample camera (256^2 sensor, ~8000 particles filling the field of
    view), with the 4-pixel (diffraction False) or the erf splat.  Returns (im1, im2, call, records, per-particle predicted
    image shift -m(Z) (dX, dY) / pitch in to_pixels axes)."""
    import torch
    n, rays = 8000, 400
    pitch = 17.0
    m0 = GEOM["image_distance"] / GEOM["object_distance"]
    half = 0.5 * N_PIX * pitch / m0 * 1.05
    lo, hi = (-half, -half, -1.0e3), (half, half, 1.0e3)
    delta = np.array([-image_shift_px[0] * pitch / m0, -image_shift_px[1] * pitch / m0, 0.0])
    call = scenes.piv_scene(n_particles=n, rays_per_source=rays, mie=False, seed=4, n_pixels=N_PIX)
    if diffraction:
        call.camera["implement_diffraction"] = True
        call.camera["diffraction_diameter"] = 2.5
    z_obj = GEOM["z_object"]
    flow = photon.flow_from_grid(*pp.uniform_flow(delta, lo, hi, 2))
    try:
        f1, w1 = photon.sources_piv_advected(21, n, lo, hi, z_obj, 730.0, 1.0e4, flow=None, t=0.0, return_world=True)
        f2, w2 = photon.sources_piv_advected(21, n, lo, hi, z_obj, 730.0, 1.0e4, flow=flow, t=1.0, return_world=True)
    finally:
        flow.free()
    images, recs = [], []
    for src in (f1, f2):
        scene = photon.scene_create_from_sources(call, src)
        img = torch.zeros(N_PIX * N_PIX, dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        try:
            scene.trace_moments(img.data_ptr(), rec.data_ptr())
            torch.cuda.synchronize()
        finally:
            scene.free()
            src.free()
        images.append(img.reshape(N_PIX, N_PIX))
        recs.append(rec.cpu().numpy())
    m = GEOM["image_distance"] / (GEOM["object_distance"] + w1[:, 2])
    predicted = -m[:, None] * (w2[:, :2] - w1[:, :2]) / pitch
    return images[0], images[1], call, recs, predicted


def window_errors(photon, im1, im2, call, recs, predicted, passes=1):
    from photon_amd import deflections
    vec, flags = photon.correlate(im1, im2, win=WIN, step=STEP, passes=passes)
    meas = pc.sensor_displacements(vec, call.camera)
    pos = deflections.to_pixels(deflections.dot_means(recs[0], call.lightray_number_per_particle, 1, "arrived")["pos"], call.camera)
    truth, count = pc.window_truth(pc.image_positions(pos, call.camera), predicted, (N_PIX, N_PIX), WIN, STEP, 5)
    use = np.isfinite(truth).all(axis=-1) & ((flags & pc.FLAG_FLAT) == 0)
    return meas[use] - truth[use], int(use.sum())


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_axis_mapping_of_a_rendered_pair(photon, diffraction):
    im1, im2, call, recs, predicted = rendered_pair(photon, diffraction)
    err, n = window_errors(photon, im1, im2, call, recs, predicted)
    assert n >= 100, n
    med = np.median(err, axis=0)
    within = (np.abs(err) <= 0.3).all(axis=1).mean()
    print(f"{'erf' if diffraction else '4-pixel'} splat: {n} windows, median error (x, y) ({med[0]:+.4f}, {med[1]:+.4f}) px, "
          f"{100 * within:.1f} % within 0.3 px")
    assert (np.abs(med) <= 0.1).all(), med
    assert within >= 0.9, within
    # the other kernel's mapping is off by twice the x shift: the test tells the two apart
    assert abs(np.median(-err[:, 0] - 2 * 3.0)) > 1.0


def test_two_passes_are_no_worse_than_one(photon):
    im1, im2, call, recs, predicted = rendered_pair(photon, False, image_shift_px=(6.0, -4.5))
    e1, n1 = window_errors(photon, im1, im2, call, recs, predicted, passes=1)
    e2, n2 = window_errors(photon, im1, im2, call, recs, predicted, passes=2)
    m1, m2 = np.median(np.hypot(*e1.T)), np.median(np.hypot(*e2.T))
    print(f"median |error|: 1 pass {m1:.4f} px ({n1} windows), 2 passes {m2:.4f} px ({n2} windows)")
    assert m2 <= m1 + 0.01, (m1, m2)


# ---- the exact-arithmetic families of piv_correlation_cases.py: every window of every case, bit for bit --------------------
import piv_correlation_cases as cases      # noqa: E402

TAIL, SENTINEL = 3, 7


def device_correlate_with_tail(photon, case, planes=True):
    """photon_piv_correlate on buffers TAIL windows longer than the grid, filled with a sentinel: (vectors [n, 4], flags [n],
    planes [n, nS, nS] or None, the three tails)."""
    import torch
    n_rows, n_cols = case.grid
    n, ns2 = n_rows * n_cols, (2 * case.R + 1) ** 2
    a, b = torch.tensor(case.im1).cuda(), torch.tensor(case.im2).cuda()          # (copies: the cases are read-only)
    off = torch.from_numpy(np.ascontiguousarray(case.offset, np.int32)).cuda() if case.offset is not None else None
    vec = torch.full(((n + TAIL) * 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    flg = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    pl = torch.full(((n + TAIL) * ns2,), float(SENTINEL), dtype=torch.float32, device="cuda") if planes else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    h, w = case.im1.shape
    rc = photon.lib.photon_piv_correlate(p(a), p(b), w, h, case.win, case.step, case.R, p(off), p(vec), p(flg), p(pl),
                                         ctypes.byref(r), ctypes.byref(c), None)
    torch.cuda.synchronize()
    assert rc == 0 and (r.value, c.value) == (n_rows, n_cols)
    vec, flg = vec.cpu().numpy(), flg.cpu().numpy()
    pl = pl.cpu().numpy() if planes else None
    tails = (vec[4 * n:], flg[n:], pl[n * ns2:] if planes else None)
    return vec[:4 * n].reshape(n, 4), flg[:n], (pl[:n * ns2].reshape(n, 2 * case.R + 1, 2 * case.R + 1) if planes else None), tails


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def assert_matches_the_model_exactly(case, got_v, got_f, got_p, tails):
    """Every window against correlate_model: flags, planes, peak and ratio bit for bit (as f32); dx and dy bit for bit on
    the edge and parabolic paths and within 1 ulp on the Gaussian path (the f64 log); flat windows all NaN; the tails
    untouched.  Returns the number of Gaussian-path components that differ by that one ulp."""
    want_v, want_f, want_p = cases.model(case.name)
    path = cases.classify(case, want_v, want_f, want_p)
    flat, live = path["flat"], path["live"]
    assert np.array_equal(got_f, want_f), np.flatnonzero(got_f != want_f)[:5]
    assert np.isnan(got_v[flat]).all()
    want32 = want_v.astype(np.float32)
    if got_p is not None:
        assert np.isnan(got_p[flat]).all()
        diff = bits(got_p[live]) != bits(want_p[live].astype(np.float32))
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5])
    for col, what in ((2, "peak"), (3, "ratio")):
        assert np.array_equal(bits(got_v[live, col]), bits(want32[live, col])), what
    one_ulp = 0
    for col, ax in ((0, "x"), (1, "y")):
        gauss = path["gauss_" + ax]
        rest = live & ~gauss                                    # the edge, parabolic (and zero-denominator) paths
        assert np.array_equal(bits(got_v[rest, col]), bits(want32[rest, col])), ("d" + ax, "exact paths")
        g, w = got_v[gauss, col], want32[gauss, col]
        near = (g == w) | (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
        assert near.all(), ("d" + ax, "Gaussian path", g[~near][:5], w[~near][:5])
        one_ulp += int((g != w).sum())
    for t in tails:
        assert t is None or (t == SENTINEL).all()
    return one_ulp


@pytest.mark.parametrize("name", cases.names())
def test_every_window_of_the_exact_families_matches_the_model(photon, name):
    case = cases.all_cases()[name]
    cases.assert_exact(case)
    one_ulp = assert_matches_the_model_exactly(case, *device_correlate_with_tail(photon, case))
    print(f"{name}: {case.grid[0] * case.grid[1]} windows, {one_ulp} Gaussian-path components one ulp from the model")


@pytest.mark.parametrize("name", ["plan_w16_r5_s7", "plan_w32_r16_s32", "planted_w64_r9", "constant_a_w64_r32"])
def test_without_planes_the_vectors_and_flags_are_the_same_bits(photon, name):
    case = cases.all_cases()[name]
    v1, f1, _, _ = device_correlate_with_tail(photon, case, planes=True)
    v0, f0, p0, tails = device_correlate_with_tail(photon, case, planes=False)
    assert p0 is None and v0.tobytes() == v1.tobytes() and f0.tobytes() == f1.tobytes()
    assert_matches_the_model_exactly(case, v0, f0, None, tails)


@pytest.mark.parametrize("win", [32, 64])
def test_a_constant_region_is_flat_through_correlate_and_gets_no_weight(photon, win):
    """What the flag is for: a masked or saturated rectangle of a particle pair -- a constant that is no dyadic number and
    that an f32 mean of the window does not reproduce -- through both passes of PhotonLibrary.correlate.  Every window wholly
    inside it carries flag 2 and NaN, and weights_from_correlation gives it weight 0."""
    from photon_amd import bos_density as bd
    step = win // 2
    c = cases.pick_constant(64, 32, seed=7)       # (at win 32, R 16 every lane adds 2 pixels and no sum rounds: win 64's value)
    im1, im2 = particle_pair((256, 256), (2.4, -1.7), seed=21)
    y0, y1, x0, x1 = 64, 64 + 3 * win // 2 + win, 32, 32 + 2 * win + win // 2      # windows of several grid rows and columns
    im1[y0:y1, x0:x1] = c
    im2[y0:y1, x0:x1] = c
    n_rows, n_cols = pc.grid_shape(im1.shape, win, step)
    i, j = np.meshgrid(np.arange(n_rows), np.arange(n_cols), indexing="ij")
    inside = (i * step >= y0) & (i * step + win <= y1) & (j * step >= x0) & (j * step + win <= x1)
    assert inside.sum() >= 4
    for passes in (1, 2):
        vec, flags = photon.correlate(im1, im2, win=win, step=step, passes=passes)
        assert ((flags[inside] & pc.FLAG_FLAT) != 0).all(), (passes, flags[inside])
        assert np.isnan(vec[inside]).all(), passes
        weights = bd.weights_from_correlation(vec, flags, pc.normalized_median_test(vec))
        assert (weights[inside] == 0.0).all() and weights[~inside].sum() > 0
