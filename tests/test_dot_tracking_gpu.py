"""Dot tracking on the device (include/parallel_ray_tracing.h, section 8): every entry point against its host model
(photon_amd/dot_tracking.py), repeat bytes, refusals, PhotonLibrary.track_dots on analytic pairs and on the rendered
blob pair against the per-dot truth, against correlate(passes=2), through the density integration, and against the clock."""
import ctypes
import time

import numpy as np
import pytest

import bos_density_cases as bc
import dot_tracking_cases as cs
from photon_amd import bos_density as bd
from photon_amd import dot_tracking as dt
from photon_amd import piv_correlation as pc

pytestmark = pytest.mark.gpu

POS_TOL = 1e-3              # px, device fit against the f64 model: the bound section 5's subpixel fit is held to
DIAMETER_TOL = 1e-3         # relative
SHIFT_TOL = 2e-3            # px, per-dot shift of the device chain against the model's
MAX_EDGE_SHARE = 1e-3       # dots whose model distance from the pixel centre lies within POS_TOL of 1 px (status bit 2 may differ)

SHAPES = ((64, 64), (100, 130), (257, 300), (333, 1000), (1024, 1024))


# ---- helpers: the raw bindings on torch buffers -----------------------------------------------------------------------------
def device_detect(photon, im, threshold, scale=None, max_dots=4096, fill=-7):
    import torch
    h, w = im.shape
    a = torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda()
    peaks = torch.full((max_dots,), fill, dtype=torch.int32, device="cuda")
    count = torch.full((1,), fill, dtype=torch.int32, device="cuda")
    nb = photon.dots_scratch_bytes(w, h)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    photon.dots_detect(a.data_ptr(), w, h, threshold, 0 if sc is None else sc.data_ptr(), max_dots, peaks.data_ptr(), count.data_ptr(),
                       scratch.data_ptr(), nb)
    torch.cuda.synchronize()
    return peaks.cpu().numpy(), int(count.item())


def device_fit(photon, im, peaks, count, box_radius, sigma_w, iterations, background=0.0, fill=-7.0):
    import torch
    h, w = im.shape
    cap = max(len(peaks), 1)
    a = torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda()
    pk = torch.from_numpy(np.ascontiguousarray(np.resize(np.asarray(peaks, np.int32), cap) if len(peaks) else np.zeros(1, np.int32))).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    dots = torch.full((cap, 4), fill, dtype=torch.float32, device="cuda")
    status = torch.full((cap,), int(fill), dtype=torch.int32, device="cuda")
    photon.dots_fit(a.data_ptr(), w, h, pk.data_ptr(), cnt.data_ptr(), cap, box_radius, sigma_w, iterations, background, dots.data_ptr(),
                    status.data_ptr())
    torch.cuda.synchronize()
    return dots.cpu().numpy(), status.cpu().numpy()


def device_match(photon, d1, s1, d2, s2, radius, shape, predictor=None, reject_mask=0, cap1=None, cap2=None):
    """Returns (pair [cap1], shift [cap1, 4], npaired, device tensors for the window means); unwritten entries hold -7."""
    import torch
    h, w = shape
    n1, n2 = len(d1), len(d2)
    cap1, cap2 = cap1 or max(n1, 1), cap2 or max(n2, 1)

    def up(d, s, cap):
        dd = np.full((cap, 4), np.nan, np.float32)
        dd[:len(d)] = d
        ss = np.zeros(cap, np.int32)
        if s is not None:
            ss[:len(d)] = s
        return torch.from_numpy(dd).cuda(), torch.from_numpy(ss).cuda()

    td1, ts1 = up(d1, s1, cap1)
    td2, ts2 = up(d2, s2, cap2)
    c1, c2 = (torch.tensor([n], dtype=torch.int32, device="cuda") for n in (n1, n2))
    pair = torch.full((cap1,), -7, dtype=torch.int32, device="cuda")
    shift = torch.full((cap1, 4), -7.0, dtype=torch.float32, device="cuda")
    npaired = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    nb = photon.dots_scratch_bytes(w, h, radius, cap1, cap2)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    kw = {}
    if predictor is not None:
        field, win, step = predictor
        fld = torch.from_numpy(np.ascontiguousarray(field, np.float32)).cuda()
        kw = dict(d_field_ptr=fld.data_ptr(), field_stride=field.shape[2], n_rows=field.shape[0], n_cols=field.shape[1], win=win, step=step)
    photon.dots_match(td1.data_ptr(), ts1.data_ptr() if s1 is not None else 0, c1.data_ptr(), cap1, td2.data_ptr(),
                      ts2.data_ptr() if s2 is not None else 0, c2.data_ptr(), cap2, radius, w, h, pair.data_ptr(), shift.data_ptr(),
                      npaired.data_ptr(), scratch.data_ptr(), nb, reject_mask=reject_mask, **kw)
    torch.cuda.synchronize()
    return pair.cpu().numpy(), shift.cpu().numpy(), int(npaired.item()), (td1, pair, shift, c1, cap1)


def device_window_means(photon, handles, shape, win, step, min_count, anchor):
    import torch
    td1, pair, shift, c1, cap1 = handles
    h, w = shape
    r, c = pc.grid_shape(shape, win, step)
    vec = torch.full((r, c, 4), -7.0, dtype=torch.float32, device="cuda")
    flg = torch.full((r, c), -7, dtype=torch.int32, device="cuda")
    photon.dots_window_means(td1.data_ptr(), pair.data_ptr(), shift.data_ptr(), c1.data_ptr(), cap1, w, h, win, step, min_count, anchor,
                             vec.data_ptr(), flg.data_ptr())
    torch.cuda.synchronize()
    return vec.cpu().numpy(), flg.cpu().numpy()


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def compare_fit(dots, status, want, want_status, peaks, width, where):
    """The device's dots against the f64 model's: positions, diameters, the peak value, and the status -- equal except
    bit 2 on dots whose model distance from the peak pixel's centre lies within POS_TOL of 1 px; those are left out, at
    most MAX_EDGE_SHARE of the dots.  Returns the worst position difference."""
    assert np.array_equal(np.isnan(dots), np.isnan(want)), where
    dp = np.abs(dots[:, :2].astype(np.float64) - want[:, :2])
    worst = float(np.nanmax(dp)) if np.isfinite(dp).any() else 0.0
    assert worst <= POS_TOL, (where, worst)
    assert np.array_equal(dots[:, 2], want[:, 2].astype(np.float32), equal_nan=True), where
    with np.errstate(invalid="ignore"):
        rel = np.abs(dots[:, 3].astype(np.float64) / want[:, 3] - 1.0)
        pk = np.asarray(peaks, np.int64)
        dist = np.stack([np.abs(want[:, 0] - pk % width), np.abs(want[:, 1] - pk // width)], axis=1)
        edge = (np.abs(dist - 1.0) <= POS_TOL).any(axis=1)
    assert not (rel > DIAMETER_TOL).any(), (where, float(np.nanmax(rel)))
    assert edge.sum() <= MAX_EDGE_SHARE * len(status), (where, int(edge.sum()))
    assert np.array_equal(status[~edge], want_status[~edge]), where
    assert np.array_equal(status[edge] & ~dt.STATUS_PULLED, want_status[edge] & ~dt.STATUS_PULLED), where
    return worst


# ---- 8a. detect ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_detect_equals_the_model_exactly(photon, shape):
    im = cs.detection_image(shape, seed=shape[0] + shape[1])
    scale = float(np.nanmax(im))
    want, total = dt.detect_model(im, 0.25, scale)
    assert total > 3
    got, count = device_detect(photon, im, 0.25, scale, max_dots=total + 5)
    assert count == total and np.array_equal(got[:total], want) and (got[total:] == -7).all()
    # more dots than max_dots: the first ones, and the total
    cap = total // 2
    got, count = device_detect(photon, im, 0.25, scale, max_dots=cap)
    assert count == total and np.array_equal(got, want[:cap])
    # no scale pointer: the threshold as it is
    thr = float(np.float32(0.25) * np.float32(scale))
    want2, total2 = dt.detect_model(im, thr)
    got, count = device_detect(photon, im, thr, None, max_dots=total2 + 1)
    assert count == total2 and np.array_equal(got[:total2], want2)


def test_detect_hand_made_image_and_no_dots(photon):
    im, thr, want = cs.hand_image()
    got, count = device_detect(photon, im, thr, max_dots=16)
    assert count == len(want) and got[:count].tolist() == want and (got[count:] == -7).all()
    got, count = device_detect(photon, np.zeros((70, 65), np.float32), 0.5, max_dots=4)
    assert count == 0 and (got == -7).all()
    got, count = device_detect(photon, im, thr, float("nan"), max_dots=16)
    assert count == 0


def test_image_max_equals_the_model(photon):
    import torch
    for shape in SHAPES[1:4]:
        im = cs.detection_image(shape, seed=3)
        a = torch.from_numpy(im).cuda()
        out = torch.full((1,), -7.0, device="cuda")
        photon.dots_image_max(a.data_ptr(), shape[1], shape[0], out.data_ptr())
        assert out.item() == float(dt.image_max_model(im))
    a = torch.full((5, 5), float("nan"), device="cuda")
    photon.dots_image_max(a.data_ptr(), 5, 5, out.data_ptr())
    assert out.item() == 0.0


# ---- 8b. fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_agrees_with_the_f64_model(photon, shape):
    im = cs.detection_image(shape, seed=shape[0] + shape[1])
    peaks, total = dt.detect_model(im, 0.25, float(np.nanmax(im)))
    # the weight stays as narrow as the dots (sigma 1 px): under a wider one a crowded image's centroids creep towards their
    # neighbours round after round and cross the 1 px line at any distance, which the cap on status bit 2 does not expect
    for box_radius, sigma_w, iterations, background in ((3, 1.0, 4, 0.0), (7, 1.0, 16, 0.01), (1, 0.8, 1, 0.0), (3, 1.0, 0, 0.0)):
        want, want_status = dt.fit_model(im, peaks, box_radius, sigma_w, iterations, background)
        dots, status = device_fit(photon, im, peaks, total, box_radius, sigma_w, iterations, background)
        worst = compare_fit(dots, status, want, want_status, peaks, shape[1], (shape, box_radius, sigma_w, iterations))
        print(f"{shape}, box {box_radius}, sigma_w {sigma_w}, {iterations} rounds: {total} dots, worst |device - model| {worst:.2e} px")
    # a count below the capacity: the entries beyond it are not written; a count above it reads as the capacity
    dots, status = device_fit(photon, im, peaks, total - 2, 3, 1.0, 4)
    assert (dots[total - 2:] == -7.0).all() and (status[total - 2:] == -7).all() and (status[:total - 2] != -7).all()
    dots, status = device_fit(photon, im, peaks, total + 1000, 3, 1.0, 4)
    assert (status != -7).all()


def test_fit_status_bits_and_bad_indices(photon):
    im = np.zeros((16, 16), np.float32)
    im[1, 8] = im[8, 8] = 1.0
    im[8, 10] = im[8, 11] = 30.0
    peaks = [1 * 16 + 8, 8 * 16 + 8, 12 * 16 + 3, 16 * 16, -1]
    want, want_status = dt.fit_model(im, peaks, 3, 2.0, 4, 0.0)
    dots, status = device_fit(photon, im, peaks, len(peaks), 3, 2.0, 4)
    assert np.array_equal(status, want_status)
    compare_fit(dots, status, want, want_status, peaks, 16, "status bits")


# ---- 8c. match -------------------------------------------------------------------------------------------------------------
def fitted_pair(shape, seed):
    """Two frames' fitted dots (model) of a detection image and a shifted, re-noised copy: n1 != n2."""
    rng = np.random.default_rng(seed)
    h, w = shape
    n = max(8, int(0.005 * h * w))
    x, y = rng.uniform(0, w, n), rng.uniform(0, h, n)
    out = []
    for dx, dy, keep in ((0.0, 0.0, n), (1.2, -0.8, n - n // 10)):
        im = pc.particle_image(shape, x[:keep] + dx, y[:keep] + dy, 4.0) + rng.normal(0, 0.01, shape)
        peaks, _ = dt.detect_model(im, 0.25, float(im.max()))
        d, s = dt.fit_model(im, peaks, 3, 1.0, 4, 0.0)
        out.append((d.astype(np.float32), s))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_match_and_window_means_equal_the_models_exactly(photon, shape):
    (d1, s1), (d2, s2) = fitted_pair(shape, seed=shape[1])
    assert len(d1) != len(d2)
    rng = np.random.default_rng(2)
    win, step = 32, 16
    r, c = pc.grid_shape(shape, win, step)
    field = rng.normal((1.2, -0.8, 0, 0), 0.3, (r, c, 4)).astype(np.float32)
    field[rng.random((r, c)) < 0.05] = np.nan
    for radius, predictor, mask in ((3.0, None, 0), (1.0, (field, win, step), 0), (2.5, (field[..., :2].copy(), win, step), dt.STATUS_BOX_OUTSIDE),
                                    (40.0, None, 0)):
        want_pair, want_shift, want_n = dt.match_model(d1, s1, d2, s2, radius, predictor, mask)
        pair, shift, n, handles = device_match(photon, d1, s1, d2, s2, radius, shape, predictor, mask, cap1=len(d1) + 3, cap2=len(d2) + 1)
        assert n == want_n and want_n > 0, (radius, n, want_n)
        assert np.array_equal(pair[:len(d1)], want_pair) and (pair[len(d1):] == -7).all()
        assert shift[:len(d1)].tobytes() == want_shift.tobytes() and (shift[len(d1):] == -7.0).all()
        for w_, st_, min_count, anchor in ((32, 16, 3, 0), (16, 8, 1, 1), (64, 32, 5, 0)):
            if min(shape) < w_:
                continue
            want_vec, want_flags = dt.window_means_model(d1, want_pair, want_shift, shape, w_, st_, min_count, anchor)
            vec, flags = device_window_means(photon, handles, shape, w_, st_, min_count, anchor)
            assert np.array_equal(flags, want_flags)
            assert vec.tobytes() == want_vec.tobytes(), (radius, w_, anchor, np.nanmax(np.abs(vec - want_vec)))


def test_match_ties_and_empty_frames(photon):
    # points on a half-pixel lattice: many equal distances, in both directions
    rng = np.random.default_rng(9)
    shape = (96, 120)
    p1 = np.unique(rng.integers(0, (240, 192), (700, 2)), axis=0) * 0.5
    p2 = np.unique(rng.integers(0, (240, 192), (650, 2)), axis=0) * 0.5
    rng.shuffle(p1)
    rng.shuffle(p2)
    pad = lambda p: np.concatenate([p, np.ones((len(p), 2))], axis=1).astype(np.float32)      # noqa: E731
    d1, d2 = pad(p1), pad(p2)
    for radius in (0.5, 1.0, 1.5, 9.0):
        want_pair, want_shift, want_n = dt.match_model(d1, None, d2, None, radius)
        pair, shift, n, _ = device_match(photon, d1, None, d2, None, radius, shape)
        assert n == want_n and np.array_equal(pair, want_pair) and shift.tobytes() == want_shift.tobytes(), radius
    empty = np.zeros((0, 4), np.float32)
    pair, shift, n, _ = device_match(photon, d1, None, empty, None, 3.0, shape)
    assert n == 0 and (pair == -1).all() and np.isnan(shift).all()
    pair, shift, n, handles = device_match(photon, empty, None, d2, None, 3.0, shape)
    assert n == 0 and (pair == -7).all()
    vec, flags = device_window_means(photon, handles, shape, 32, 16, 1, 0)
    assert (flags == 2).all() and (vec[..., 2] == 0).all() and np.isnan(vec[..., 0]).all()


# ---- repeat bytes ----------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(photon):
    shape = (257, 300)
    im = cs.detection_image(shape, seed=5)
    scale = float(np.nanmax(im))
    a, b = (device_detect(photon, im, 0.25, scale) for _ in range(2))
    assert a[1] == b[1] and same_bytes(a[:1], b[:1])
    peaks, total = a[0][:a[1]], a[1]
    f1, f2 = (device_fit(photon, im, peaks, total, 3, 1.0, 4) for _ in range(2))
    assert same_bytes(f1, f2)
    (d1, s1), (d2, s2) = fitted_pair(shape, seed=8)
    m1, m2 = (device_match(photon, d1, s1, d2, s2, 3.0, shape) for _ in range(2))
    assert m1[2] == m2[2] and same_bytes(m1[:2], m2[:2])
    w1, w2 = (device_window_means(photon, m[3], shape, 32, 16, 3, 0) for m in (m1, m2))
    assert same_bytes(w1, w2)
    _, d, im1, im2, _, _ = next(cs.chain_pairs())
    r1, r2 = (photon.track_dots(im1, im2, sigma_w=d / 4, grid=(32, 16, 3, 0), **cs.CHAIN) for _ in range(2))
    assert r1.keys() == r2.keys() and all(np.asarray(r1[k]).tobytes() == np.asarray(r2[k]).tobytes() for k in r1)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    h, w, cap = 64, 80, 32
    im = torch.rand((h, w), device="cuda")
    ints = torch.full((6, cap), 7, dtype=torch.int32, device="cuda")           # peaks, count, status, pair, npaired, flags
    flt = torch.full((3, cap, 4), 7.0, device="cuda")                           # dots, shift, vectors (2 x 3 windows at win 32 / step 16)
    cnt = torch.tensor([5], dtype=torch.int32, device="cuda")
    sb = max(photon.dots_scratch_bytes(w, h), photon.dots_scratch_bytes(w, h, 3.0, cap, cap))
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    fld = torch.zeros((3, 4, 2), device="cuda")                                 # section 5's grid of 64 x 80, win 32, step 16
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731
    nan, inf = float("nan"), float("inf")
    capfd.readouterr()

    def refused(name, what, rc):
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, (name, what, rc)
        assert len(err.strip().splitlines()) == 1 and name in err, (name, what, err)
        assert (ints == 7).all().item() and (flt == 7.0).all().item(), (name, what)

    def sweep(name, fn, ok, changes):
        for what, change in changes:
            refused(name, what, fn(*[change.get(k, v) for k, v in enumerate(ok)]))

    sweep("photon_dots_image_max", L.photon_dots_image_max, (p(im), w, h, p(flt[0]), None),
          (("null image", {0: None}), ("null output", {3: None}), ("width 0", {1: 0})))
    sweep("photon_dots_detect", L.photon_dots_detect, (p(im), w, h, 0.5, None, cap, p(ints[0]), p(ints[1]), p(scratch), sb, None),
          (("null image", {0: None}), ("null peaks", {6: None}), ("null count", {7: None}), ("null scratch", {8: None}),
           ("small scratch", {9: sb // 64}), ("2 rows", {2: 2}), ("2 columns", {1: 2}), ("too many pixels", {1: 65536, 2: 65536}),
           ("max_dots 0", {5: 0}), ("threshold nan", {3: nan}), ("threshold inf", {3: inf})))
    sweep("photon_dots_fit", L.photon_dots_fit, (p(im), w, h, p(ints[0]), p(cnt), cap, 3, 1.0, 4, 0.0, p(flt[0]), p(ints[2]), None),
          (("null image", {0: None}), ("null peaks", {3: None}), ("null count", {4: None}), ("null dots", {10: None}), ("null status", {11: None}),
           ("max_dots 0", {5: 0}), ("box 0", {6: 0}), ("box 8", {6: 8}), ("sigma 0", {7: 0.0}), ("sigma nan", {7: nan}), ("sigma inf", {7: inf}),
           ("iterations -1", {8: -1}), ("iterations 17", {8: 17}), ("background nan", {9: nan}), ("width 0", {1: 0})))
    ok = (p(flt[0]), p(ints[2]), p(cnt), cap, p(flt[0]), p(ints[2]), p(cnt), cap, 0, p(fld), 2, 3, 4, 32, 16, 3.0, w, h, p(ints[3]), p(flt[1]),
          p(ints[4]), p(scratch), sb, None)
    assert pc.grid_shape((h, w), 32, 16) == (3, 4)
    sweep("photon_dots_match", L.photon_dots_match, ok,
          (("null dots 1", {0: None}), ("null dots 2", {4: None}), ("null count 1", {2: None}), ("null count 2", {6: None}), ("null pair", {18: None}),
           ("null shift", {19: None}), ("null npaired", {20: None}), ("null scratch", {21: None}), ("small scratch", {22: 64}), ("max1 0", {3: 0}),
           ("max2 0", {7: 0}), ("radius 0", {15: 0.0}), ("radius nan", {15: nan}), ("radius inf", {15: inf}), ("stride 3", {10: 3}),
           ("grid rows", {11: 4}), ("grid columns", {12: 3}), ("win 0", {13: 0}), ("step 0", {14: 0}), ("width 0", {16: 0})))
    sweep("photon_dots_window_means", L.photon_dots_window_means,
          (p(flt[0]), p(ints[3]), p(flt[1]), p(cnt), cap, w, h, 32, 16, 3, 0, p(flt[2]), p(ints[5]), None),
          (("null dots", {0: None}), ("null pair", {1: None}), ("null shift", {2: None}), ("null count", {3: None}), ("null vectors", {11: None}),
           ("null flags", {12: None}), ("max1 0", {4: 0}), ("win 0", {7: 0}), ("step 0", {8: 0}), ("image too small", {6: 31}),
           ("min_count 0", {9: 0}), ("anchor 2", {10: 2})))
    assert photon.dots_scratch_bytes(0, 5) == 0 and photon.dots_scratch_bytes(w, h, -1.0, cap, cap) == 0


# ---- the chain on analytic pairs -------------------------------------------------------------------------------------------
def test_chain_on_analytic_pairs_meets_the_conditions_and_the_model(photon):
    """The ten pairs of tests/test_dot_tracking.py on the device: the same conditions (0.80 tracked, 2 % wrong, the median
    within 1.5 x 0.0378 px), and per-dot shifts within 2e-3 px of the model's for every dot both pair identically."""
    from test_dot_tracking import CHAIN_WORST_MEDIAN
    for name, diameter, im1, im2, pos, shifts in cs.chain_pairs():
        res = photon.track_dots(im1, im2, sigma_w=diameter / 4, **cs.CHAIN)
        ref = dt.track_dots_model(im1, im2, sigma_w=diameter / 4, **cs.CHAIN)
        s = dt.score(res, pos, shifts)
        assert (res["count1"], res["count2"]) == (ref["count1"], ref["count2"])
        same = (res["pair"] == ref["pair"]) & (res["pair"] >= 0)
        diff = float(np.abs(res["shift"][same].astype(np.float64) - ref["shift"][same]).max())
        print(f"{name}: {res['count1']} / {res['count2']} dots, {res['npaired']} pairs ({int(same.sum())} as the model), tracked "
              f"{s['tracked']:.4f}, wrong {s['wrong']:.4f}, median {s['median']:.4f} px, 95th percentile {s['p95']:.4f} px, "
              f"worst |device - model| shift {diff:.2e} px")
        assert s["tracked"] >= cs.MIN_TRACKED and s["wrong"] <= cs.MAX_WRONG and s["median"] <= 1.5 * CHAIN_WORST_MEDIAN, name
        assert same.sum() >= 0.99 * ref["npaired"] and diff <= SHIFT_TOL, name


def test_track_dots_with_a_predictor_equals_the_model(photon):
    """A shift beyond the radius: nothing pairs without the predictor, the model's pairs with it (field as numpy [r, c, 4]
    and as a device tensor [r, c, 2])."""
    rng = np.random.default_rng(4)
    n, shape = 1200, (400, 520)
    x, y = rng.uniform(0, shape[1], n), rng.uniform(0, shape[0], n)
    im1 = pc.particle_image(shape, x, y, 4.0).astype(np.float32)
    im2 = pc.particle_image(shape, x + 6.3, y - 4.6, 4.0).astype(np.float32)
    kw = dict(sigma_w=1.0, threshold=0.25, relative=True, radius=1.5, grid=(32, 16, 3, 1))
    vectors, _ = photon.correlate(im1, im2, win=32, step=16)
    ref = dt.track_dots_model(im1, im2, predictor=(vectors, 32, 16), **kw)
    assert ref["npaired"] > 0.8 * ref["count1"] and dt.track_dots_model(im1, im2, **kw)["npaired"] < 0.1 * ref["count1"]
    res = photon.track_dots(im1, im2, predictor=(vectors, 32, 16), **kw)
    assert np.array_equal(res["pair"], ref["pair"]) and res["npaired"] == ref["npaired"]
    assert np.nanmax(np.abs(res["shift"].astype(np.float64) - ref["shift"])) <= SHIFT_TOL
    assert np.array_equal(res["flags"], ref["flags"]) and np.nanmax(np.abs(res["vectors"] - ref["vectors"])) <= SHIFT_TOL
    assert abs(np.nanmedian(res["shift"][:, 2]) - 6.3) < 0.01 and abs(np.nanmedian(res["shift"][:, 3]) + 4.6) < 0.01
    pred = photon.correlation_predictor(im1, im2, 32, 16)
    assert tuple(pred.shape) == pc.grid_shape(shape, 32, 16) + (2,)
    dev = photon.track_dots(im1, im2, predictor=(pred, 32, 16), **kw)
    assert dev["npaired"] > 0.8 * dev["count1"] and abs(np.nanmedian(dev["shift"][:, 2]) - 6.3) < 0.01


# ---- the rendered blob pair ------------------------------------------------------------------------------------------------
DOT_PX = 5.4                # e^-2 diameter of the blob scene's dots on the sensor, pixels
MARGIN = 4.0                # the truth must lie inside the sensor by more than this
# Median per-dot error of the f64 model on the two rendered images, px (measured on MI355X renders by this test: DESIGN.md
# section 4.3e; most dots lie where the blob barely moves them, and both frames render a dot from the same rays):
MODEL_MEDIAN = {False: 0.00144, True: 0.00091}


@pytest.fixture(scope="module")
def blob_pairs(photon, tmp_path_factory):
    """Both splats: (call_with, im1, im2, records 1, records 2) per diffraction setting."""
    wd = str(tmp_path_factory.mktemp("blob_dots"))
    out = {}
    for diffraction in (False, True):
        c1, c2 = bc.blob_calls(photon, wd, diffraction)
        im1, r1 = photon.render_moments(c1)
        im2, r2 = photon.render_moments(c2)
        out[diffraction] = (c2, im1.reshape(bc.N_PIX, bc.N_PIX).astype(np.float32), im2.reshape(bc.N_PIX, bc.N_PIX).astype(np.float32), r1, r2)
    return out


def rendered(photon, blob_pairs, diffraction):
    call, im1, im2, r1, r2 = blob_pairs[diffraction]
    truth = dt.true_dots(r1, r2, call.camera, call.lightray_number_per_particle, group=bc.DOT_POINTS)
    p = truth["pos1"]
    with np.errstate(invalid="ignore"):
        inside = (p[:, 0] > MARGIN) & (p[:, 0] < bc.N_PIX - 1 - MARGIN) & (p[:, 1] > MARGIN) & (p[:, 1] < bc.N_PIX - 1 - MARGIN)
    kw = dict(sigma_w=DOT_PX / 4, grid=(bc.WIN, bc.STEP, 3, 0), **cs.CHAIN)
    return call, im1, im2, truth, inside, kw


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_rendered_pair_per_dot_against_the_truth_and_the_model(photon, blob_pairs, diffraction):
    """(i) 0.80 of the true dots inside the sensor tracked, 2 % of them wrong at most; (ii) the device within 2e-3 px of
    the f64 model per dot, the model's median per-dot error within 1.5 x its recorded value (MODEL_MEDIAN)."""
    call, im1, im2, truth, inside, kw = rendered(photon, blob_pairs, diffraction)
    res = photon.track_dots(im1, im2, **kw)
    ref = dt.track_dots_model(im1, im2, **kw)
    s, sm = dt.score(res, truth["pos1"], truth["shift"], inside), dt.score(ref, truth["pos1"], truth["shift"], inside)
    same = (res["pair"] == ref["pair"]) & (res["pair"] >= 0)
    diff = float(np.abs(res["shift"][same].astype(np.float64) - ref["shift"][same]).max())
    name = "erf" if diffraction else "4-pixel"
    print(f"rendered {name}: {s['n']} true dots inside, {res['count1']} / {res['count2']} detected, {res['npaired']} pairs; device tracked "
          f"{s['tracked']:.4f}, wrong {s['wrong']:.4f}, median {s['median']:.4f} px, 95th percentile {s['p95']:.4f} px; model tracked "
          f"{sm['tracked']:.4f}, wrong {sm['wrong']:.4f}, median {sm['median']:.4f} px, 95th percentile {sm['p95']:.4f} px; "
          f"worst |device - model| shift {diff:.2e} px over {int(same.sum())} dots paired alike; status bit 2 on "
          f"{int((res['status1'] & 2 != 0).sum())} dots of frame 1")
    assert (res["count1"], res["count2"]) == (ref["count1"], ref["count2"])
    assert same.sum() >= 0.99 * ref["npaired"] and diff <= SHIFT_TOL
    assert s["tracked"] >= cs.MIN_TRACKED and s["wrong"] <= cs.MAX_WRONG
    assert sm["median"] <= 1.5 * MODEL_MEDIAN[diffraction]
    assert s["median"] <= 1.5 * MODEL_MEDIAN[diffraction] + SHIFT_TOL


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_rendered_pair_on_the_window_grid_against_two_pass_correlation(photon, blob_pairs, diffraction):
    """(iii) median |window mean - window_truth| of the tracked field <= 1.25 x that of correlate(passes=2), same pair."""
    call, im1, im2, truth, inside, kw = rendered(photon, blob_pairs, diffraction)
    res = photon.track_dots(im1, im2, **kw)
    vectors, flags = photon.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    want, _ = pc.window_truth(truth["pos1"], truth["shift"], (bc.N_PIX, bc.N_PIX), bc.WIN, bc.STEP, 3)
    e_t = np.linalg.norm(res["vectors"][..., :2] - want, axis=-1)
    e_c = np.linalg.norm(vectors[..., :2] - want, axis=-1)
    m_t, m_c = float(np.nanmedian(e_t)), float(np.nanmedian(e_c))
    print(f"rendered {'erf' if diffraction else '4-pixel'}, win {bc.WIN} / step {bc.STEP}: median |window mean - truth| tracked {m_t:.4f} px "
          f"({int(np.isfinite(e_t).sum())} windows), correlate(passes=2) {m_c:.4f} px ({int(np.isfinite(e_c).sum())} windows), ratio {m_t / m_c:.3f}")
    assert m_t <= 1.25 * m_c


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_rendered_pair_tracked_field_integrates_to_the_projection(photon, blob_pairs, diffraction):
    """(iv) reconstruct_tracked: relative L2 error of the projected density <= 1.5 x what the true shifts give in the same
    run, the argmax within one grid step, at most MAX_HOLES of the nodes NaN."""
    call, im1, im2, truth, inside, kw = rendered(photon, blob_pairs, diffraction)
    want, _ = pc.window_truth(truth["pos1"], truth["shift"], (bc.N_PIX, bc.N_PIX), bc.WIN, bc.STEP, 3)
    phi_true, _, st = bd.integrate_vectors(photon, want, np.where(np.isfinite(want[..., 0]), 0, 2), (bc.N_PIX, bc.N_PIX), call, bc.ORIGIN_Z,
                                           bc.EXTENT, bc.WIN, bc.STEP, weights="unit")
    assert st["converged"] == 1
    P, mid, h = bc.truth(call)
    rel_true, _, _ = bc.errors(phi_true, P, mid, h)
    phi, _, st = bd.reconstruct_tracked(photon, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, sigma_w=DOT_PX / 4,
                                        box_radius=cs.CHAIN["box_radius"], iterations=cs.CHAIN["iterations"], radius=cs.CHAIN["radius"])
    assert st["converged"] == 1
    rel, off, holes = bc.errors(phi, P, mid, h)
    phi0, _, _ = bd.reconstruct_tracked(photon, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, predict=False, sigma_w=DOT_PX / 4,
                                        box_radius=cs.CHAIN["box_radius"], iterations=cs.CHAIN["iterations"], radius=cs.CHAIN["radius"])
    print(f"rendered {'erf' if diffraction else '4-pixel'}: rel L2 error of the projected density, tracked {rel:.4f}, true shifts {rel_true:.4f} "
          f"(ratio {rel / rel_true:.3f}; without the correlation predictor {bc.errors(phi0, P, mid, h)[0]:.4f}), argmax offset ({off[0]:+.2f}, {off[1]:+.2f}) grid steps, {100 * holes:.1f} % of the nodes NaN")
    assert abs(off[0]) <= 1.0 and abs(off[1]) <= 1.0, off
    assert holes <= 0.1, holes
    assert rel <= 1.5 * rel_true


# ---- time ------------------------------------------------------------------------------------------------------------------
def test_tracking_is_not_slower_than_three_deformation_iterations_at_1024(photon):
    """Wall time of track_dots with a grid <= 1.5 x correlate_deform(iterations=3), 1024^2 analytic pair at 0.005 dots per
    pixel, win 32 / step 16: medians of 12 alternating synchronised calls."""
    import torch
    im1, im2, _, _ = cs.analytic_pair(1, 0.005, 4.0, n_pix=1024)
    a, b = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    calls = {"track": lambda: photon.track_dots(a, b, sigma_w=1.0, grid=(32, 16, 3, 0), **cs.CHAIN),
             "deform": lambda: photon.correlate_deform(a, b, 32, 16, 16, iterations=3)}
    times = {k: [] for k in calls}
    for rep in range(3 + 12):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append(1e3 * (time.perf_counter() - t0))
    t_track, t_deform = np.median(times["track"]), np.median(times["deform"])
    print(f"1024^2, win 32 / step 16, medians of 12 alternating calls: track_dots {t_track:.3f} ms, correlate_deform(iterations=3) "
          f"{t_deform:.3f} ms, ratio {t_track / t_deform:.3f}")
    assert t_track <= 1.5 * t_deform
