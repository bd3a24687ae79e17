"""photon_piv_background and photon_piv_preprocess on the GPU (include/parallel_ray_tracing.h, section 15): both bit for bit
against the host models on every path a caller can reach (16-byte and scalar reads, both modes, every radius, with and
without a background, in place), strides with untouched gaps, repeats, streams, the refusals, the wall series the feature
is for through preprocess_series and the correlators, and both calls on the clock against the torch composition."""
import ctypes

import numpy as np
import pytest

import piv_preprocess_cases as cs
from photon_amd import piv_preprocess as pp

pytestmark = pytest.mark.gpu

TAIL, SENTINEL = 5, 7.0
T = 32                  # the chain kernel's tile side (photon_piv_preprocess.hip, Chain<R>::T)


def vp(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset) if t is not None else None


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def strided(frames, stride, base=0):
    """The frames [N, h, w] laid `stride` floats apart from float `base` of a device buffer whose gaps hold the sentinel; the
    buffer starts 16-byte aligned (torch's allocator), so `base` decides the alignment of frame 0."""
    import torch
    n, h, w = frames.shape
    buf = np.full(base + (n - 1) * stride + h * w, SENTINEL, np.float32)
    for k in range(n):
        buf[base + k * stride:base + k * stride + h * w] = frames[k].ravel()
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def device_background(photon, frames, mode, stride=None, base=0, out_base=0):
    """photon_piv_background on frames laid out by `strided`, into a buffer with a sentinel tail.  Returns (plane, path)."""
    import torch
    n, h, w = frames.shape
    stride = h * w if stride is None else stride
    buf = strided(frames, stride, base)
    out = torch.full((out_base + h * w + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    path = photon.piv_background_path(buf.data_ptr() + 4 * base, stride, out.data_ptr() + 4 * out_base)
    rc = photon.lib.photon_piv_background(vp(buf, base), stride, n, w, h, mode, vp(out, out_base), None)
    torch.cuda.synchronize()
    assert rc == 0
    o = out.cpu().numpy()
    assert (o[:out_base] == SENTINEL).all() and (o[out_base + h * w:] == SENTINEL).all()
    return o[out_base:out_base + h * w].reshape(h, w), path


def device_chain(photon, frames, bg, radius, floor, stride=None, out_stride=None, base=0, stream=None):
    """photon_piv_preprocess into a buffer pre-filled with the sentinel: (out [N, h, w]) after checking that the gaps between
    the frames of the output and its tail are untouched."""
    import torch
    n, h, w = frames.shape
    stride = h * w if stride is None else stride
    out_stride = h * w if out_stride is None else out_stride
    buf = strided(frames, stride, base)
    d_bg = torch.from_numpy(np.ascontiguousarray(bg, np.float32)).cuda() if bg is not None else None
    out = torch.full(((n - 1) * out_stride + h * w + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = photon.lib.photon_piv_preprocess(vp(buf, base), stride, n, w, h, vp(d_bg), radius, 0.0 if floor is None else floor, vp(out),
                                          out_stride, ctypes.c_void_p(stream.cuda_stream) if stream is not None else None)
    torch.cuda.synchronize()
    assert rc == 0
    o = out.cpu().numpy()
    got = np.stack([o[k * out_stride:k * out_stride + h * w].reshape(h, w) for k in range(n)])
    for k in range(n):
        assert (o[k * out_stride + h * w:(k + 1) * out_stride if k < n - 1 else None] == SENTINEL).all(), f"gap after frame {k}"
    return got


def assert_same_bits(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], np.asarray(want)[bad][:5])


# ---- the background ------------------------------------------------------------------------------------------------------------
BG_SHAPES = [(1, 1), (1, 7), (33, 31), (129, 257)]


@pytest.mark.parametrize("n", [1, 2, 7, 64])
@pytest.mark.parametrize("shape", BG_SHAPES, ids=[f"{h}x{w}" for h, w in BG_SHAPES])
def test_the_background_equals_the_model_bit_for_bit_on_both_paths(photon, shape, n):
    """The 16-byte path needs both base pointers 16-byte aligned and a stride that is a multiple of 4 floats; every other
    layout reads pixel by pixel.  Strides w h, w h + 1, w h + 3 and 2 w h and a base moved by one float reach both, and
    w h mod 4 = 1, 3, 3, 1 on the four shapes reaches the 16-byte path's scalar tail (1 x 1 and 1 x 7: the tail alone and
    one run of 4 with a tail of 3).  The library reports the path; the rule is asserted here too."""
    h, w = shape
    frames = cs.particle_frames(shape, n, seed=h + n)
    taken = set()
    for mode in (pp.MODE_MIN, pp.MODE_MEAN):
        want = pp.background_model(frames, mode)
        for stride in (h * w, h * w + 1, h * w + 3, 2 * h * w):
            for base, out_base in ((0, 0), (1, 0), (0, 1)):
                got, path = device_background(photon, frames, mode, stride, base, out_base)
                assert path == int(base == 0 and out_base == 0 and stride % 4 == 0), (stride, base, out_base)
                taken.add(path)
                assert_same_bits(got, want, (mode, stride, base, out_base, path))
    assert taken == {0, 1}      # w h + 3 is a multiple of 4 on 1 x 1 and 129 x 257, w h + 1 on 1 x 7 and 33 x 31


def test_a_straddled_series_takes_every_other_frame(photon):
    frames = cs.particle_frames((33, 31), 8, seed=2)
    import torch
    buf = torch.tensor(frames).cuda()
    for first in (0, 1):
        got = photon.piv_background(buf[first].data_ptr(), 2 * 33 * 31, 4, 31, 33, pp.MODE_MIN)
        assert_same_bits(got.cpu().numpy(), pp.background_model(frames[first::2], pp.MODE_MIN), first)


# ---- the chain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,with_bg", [(r, b) for r in range(9) for b in (True, False) if r or b],
                         ids=lambda v: {True: "bg", False: "nobg"}.get(v, f"r{v}") if isinstance(v, bool) else f"r{v}")
def test_every_radius_equals_the_f32_model_bit_for_bit(photon, radius, with_bg):
    """Every instantiation piv_minmax_kernel<1 .. 8> and the radius-0 kernel, 70 x 90 (three tiles a side, the last ones
    partial), three frames in one call with both strides above w h: the gaps of the output stay at the sentinel.  (Radius 0
    without a background is refused.)"""
    frames = cs.particle_frames((70, 90), 3, seed=radius)
    bg = pp.background_model(frames, pp.MODE_MIN) if with_bg else None
    floor = 0.05 if radius else None
    want = pp.preprocess_model_f32(frames, bg, radius, floor)
    got = device_chain(photon, frames, bg, radius, floor, stride=70 * 90 + 5, out_stride=70 * 90 + 3)
    assert_same_bits(got, want, radius)


SMALL = [(1, 3), (3, 1), (5, 40), (1, 1)]
SIDES = [T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("shape", SMALL + [(s, T + 3) for s in SIDES] + [(T - 5, s) for s in SIDES],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_smaller_than_the_window_and_around_the_tile_side(photon, shape):
    """r = 8 (the widest halo: 16 pixels a side, more than some of these images), r = 5 and r = 1, with a background and, at
    r = 8, without.  Sides T - 1, T, T + 1 and 2 T + 1 in each axis: a last tile of 31, 32, 1 and 1 pixels."""
    frames = cs.particle_frames(shape, 2, seed=shape[0] * 100 + shape[1])
    bg = pp.background_model(frames, pp.MODE_MEAN)
    for radius, b in ((8, bg), (8, None), (5, bg), (1, bg), (0, bg)):
        floor = 0.1 if radius else None
        assert_same_bits(device_chain(photon, frames, b, radius, floor), pp.preprocess_model_f32(frames, b, radius, floor), (radius, b is None))


def test_a_strip_taller_than_the_grid(photon):
    """2 097 153 x 3 pixels: 65 537 tile rows, more than a grid's second dimension holds, and 6.3 million pixels, more than
    the background's 16 384 blocks of 256 lanes hold at one pixel a lane -- the strided loops of both kernels."""
    rng = np.random.default_rng(0)
    frames = rng.random((2, 65536 * T + 1, 3), dtype=np.float32)
    got, path = device_background(photon, frames, pp.MODE_MIN, base=1)
    assert path == 0
    assert_same_bits(got, pp.background_model(frames, pp.MODE_MIN), "background")
    assert_same_bits(device_chain(photon, frames[:1], None, 1, 0.5), pp.preprocess_model_f32(frames[:1], None, 1, 0.5), "chain")


def test_radius_zero_in_place(photon):
    import torch
    frames = cs.particle_frames((33, 47), 5, seed=1)
    bg = pp.background_model(frames, pp.MODE_MIN)
    stride = 33 * 47 + 2
    buf = strided(frames, stride)
    d_bg = torch.from_numpy(bg).cuda()
    rc = photon.lib.photon_piv_preprocess(vp(buf), stride, 5, 47, 33, vp(d_bg), 0, 0.0, vp(buf), stride, None)
    torch.cuda.synchronize()
    assert rc == 0
    o = buf.cpu().numpy()
    want = pp.preprocess_model_f32(frames, bg, 0)
    for k in range(5):
        assert_same_bits(o[k * stride:k * stride + 33 * 47].reshape(33, 47), want[k], k)
        if k < 4:
            assert (o[k * stride + 33 * 47:(k + 1) * stride] == SENTINEL).all()


def test_two_calls_and_another_stream_return_identical_bytes(photon):
    import torch
    frames = cs.particle_frames((100, 130), 4, seed=4)
    bg = pp.background_model(frames, pp.MODE_MIN)
    side = torch.cuda.Stream()
    for radius, floor in ((0, None), (5, 0.05), (8, 0.02)):
        first = device_chain(photon, frames, bg, radius, floor)
        assert first.tobytes() == device_chain(photon, frames, bg, radius, floor).tobytes()
        assert first.tobytes() == device_chain(photon, frames, bg, radius, floor, stream=side).tobytes()
    buf = torch.tensor(frames).cuda()
    for mode in (0, 1):
        first = photon.piv_background(buf.data_ptr(), 100 * 130, 4, 130, 100, mode).cpu().numpy()
        assert first.tobytes() == photon.piv_background(buf.data_ptr(), 100 * 130, 4, 130, 100, mode).cpu().numpy().tobytes()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = photon.piv_background(buf.data_ptr(), 100 * 130, 4, 130, 100, mode, stream=side.cuda_stream)
        side.synchronize()
        assert first.tobytes() == other.cpu().numpy().tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    h, w, n = 20, 24, 3
    npx = h * w
    frames = torch.rand(((n + 1) * npx + 64,), device="cuda")
    bg = torch.rand((npx,), device="cuda")
    out = torch.full((n * npx + 64,), SENTINEL, device="cuda")
    before = frames.clone()
    big = (1 << 22) + 1

    good_b = dict(frames=vp(frames), stride=npx, n=n, w=w, h=h, mode=0, out=vp(out))
    good_p = dict(frames=vp(frames), stride=npx, n=n, w=w, h=h, bg=vp(bg), radius=3, floor=0.1, out=vp(out), ostride=npx)
    inside = ctypes.c_void_p(frames.data_ptr() + 4 * (npx + 5))
    last = ctypes.c_void_p(frames.data_ptr() + 4 * (n * npx - 1))
    refused_b = [("null frames", dict(frames=None)), ("null out", dict(out=None)), ("no frame", dict(n=0)), ("n < 0", dict(n=-1)),
                 ("stride below one image", dict(stride=npx - 1)), ("stride 0", dict(stride=0)), ("stride < 0", dict(stride=-npx)),
                 ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("width 0", dict(w=0)), ("height 0", dict(h=0)),
                 ("width beyond the limit", dict(w=big, stride=big * h)), ("height beyond the limit", dict(h=big, stride=big * w)),
                 ("out inside the frames", dict(out=inside)), ("out on the last pixel", dict(out=last)), ("out is the frames", dict(out=vp(frames)))]
    refused_p = [("null frames", dict(frames=None)), ("null out", dict(out=None)), ("no frame", dict(n=0)),
                 ("frame stride below one image", dict(stride=npx - 1)), ("out stride below one image", dict(ostride=npx - 1)),
                 ("out stride 0", dict(ostride=0)), ("radius -1", dict(radius=-1)), ("radius 9", dict(radius=9)),
                 ("floor 0", dict(floor=0.0)), ("floor < 0", dict(floor=-0.1)), ("floor nan", dict(floor=float("nan"))),
                 ("floor inf", dict(floor=float("inf"))), ("radius 0, no background", dict(radius=0, bg=None)), ("width 0", dict(w=0)),
                 ("height beyond the limit", dict(h=big, stride=big * w, ostride=big * w)),
                 ("in place with a filter", dict(out=vp(frames))), ("out inside the frames", dict(out=inside)),
                 ("radius 0, out moved by a pixel", dict(radius=0, out=ctypes.c_void_p(frames.data_ptr() + 4))),
                 ("radius 0, in place at another stride", dict(radius=0, out=vp(frames), ostride=npx + 1)),
                 ("out is the background", dict(out=vp(bg), n=1))]
    capfd.readouterr()
    for entry, good, cases in (("photon_piv_background", good_b, refused_b), ("photon_piv_preprocess", good_p, refused_p)):
        for what, change in cases:
            a = dict(good, **change)
            if entry == "photon_piv_background":
                rc = L.photon_piv_background(a["frames"], a["stride"], a["n"], a["w"], a["h"], a["mode"], a["out"], None)
            else:
                rc = L.photon_piv_preprocess(a["frames"], a["stride"], a["n"], a["w"], a["h"], a["bg"], a["radius"], a["floor"], a["out"],
                                             a["ostride"], None)
            torch.cuda.synchronize()
            err = capfd.readouterr().err
            assert rc == 1, (entry, what)
            assert len(err.strip().splitlines()) == 1 and entry + ":" in err, (entry, what, err)
            assert (out == SENTINEL).all().item() and torch.equal(frames, before), (entry, what)
    # what is allowed next to them: the out plane right behind the span, the largest radius, the smallest floor
    assert L.photon_piv_background(vp(frames), npx, n, w, h, 1, vp(frames, n * npx), None) == 0
    assert L.photon_piv_preprocess(vp(frames), npx, n, w, h, None, 8, float(np.finfo(np.float32).tiny), vp(out), npx, None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == ""


# ---- what the feature is for ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_wall_series_on_the_device(photon, seed):
    """The CPU test's series through preprocess_series and the correlators: at most 2 of 25 windows within 0.3 px of the
    truth on the raw stacks, at least 24 processed -- for the ensemble of 8 pairs and for a single pair, without and with the
    filter.  The processed stacks are the models' bit for bit."""
    a, b = cs.wall_series(seed)
    win, step, R = cs.WALL_WIN, cs.WALL_STEP, cs.WALL_R
    counts = {"raw ensemble": cs.near_truth(photon.correlate_ensemble(np.array(a), np.array(b), win, step, R)[0]),
              "raw pair": cs.near_truth(photon.correlate(np.array(a[0]), np.array(b[0]), win, step, R)[0])}
    for name, radius, floor in (("minimum subtracted", 0, None), ("and filtered", cs.WALL_RADIUS, cs.WALL_FLOOR)):
        pa, pb = photon.preprocess_series(np.array(a), np.array(b), background="min", minmax_radius=radius, floor=floor)
        want_a, want_b = cs.wall_processed(seed, radius)
        assert_same_bits(pa.cpu().numpy(), want_a, name)
        assert_same_bits(pb.cpu().numpy(), want_b, name)
        vec, flags, count = photon.correlate_ensemble(pa, pb, win, step, R)
        assert (count == cs.WALL_PAIRS).all()
        counts[name + ", ensemble"] = cs.near_truth(vec)
        counts[name + ", pair"] = cs.near_truth(photon.correlate(pa[0], pb[0], win, step, R)[0])
    print(f"seed {seed} on the device, windows of 25 within {cs.WALL_WITHIN} px: {counts}")
    for name, c in counts.items():
        assert c <= 2 if name.startswith("raw") else c >= 24, (name, c)


def test_the_series_driver_takes_tensors_arrays_backgrounds_and_one_buffer(photon):
    import torch
    a, b = cs.wall_series(1)
    series = np.concatenate([a[:4], b[:1]])
    got = photon.preprocess_series(torch.from_numpy(series).cuda(), background="mean", minmax_radius=3, floor=0.1)
    bg = pp.background_model(series, pp.MODE_MEAN)
    assert tuple(got.shape) == series.shape
    assert_same_bits(got.cpu().numpy(), pp.preprocess_model_f32(series, bg, 3, 0.1), "one buffer, mean")
    for given in (bg, torch.from_numpy(bg).cuda()):
        assert_same_bits(photon.preprocess_series(series, background=given).cpu().numpy(), pp.preprocess_model_f32(series, bg, 0), "given plane")
    assert_same_bits(photon.preprocess_series(series, background=None, minmax_radius=2, floor=0.2).cpu().numpy(),
                     pp.preprocess_model_f32(series, None, 2, 0.2), "no background")
    for bad in (dict(background="median"), dict(minmax_radius=3), dict(minmax_radius=9, floor=0.1), dict(background=None),
                dict(background=bg[:5]), dict(minmax_radius=2, floor=0.0)):
        with pytest.raises(ValueError):
            photon.preprocess_series(series, **bad)
    with pytest.raises(ValueError):
        photon.preprocess_series(series[0])


# ---- on the clock --------------------------------------------------------------------------------------------------------------
def test_neither_call_is_slower_than_its_torch_counterpart(photon):
    """16 frames of 1024^2, device events around ten back-to-back calls (one call of 20 us between two events measures the
    host's launch path as much as the kernel), the sides alternating after two warm-up rounds, medians of five.  The background
    against torch.amin(stack, 0) and torch.mean(stack, 0); the chain at r = 5 against the composition a user of torch
    writes: subtract, clamp_min, max_pool2d of -d and of d, avg_pool2d of both, subtract, clamp, divide (torch pads where the
    library clips: other values at the border, the same work).  No margin: parity is the weakest acceptable outcome."""
    import torch
    import torch.nn.functional as F
    n, h, w, r, floor = 16, 1024, 1024, 5, 0.05
    g = torch.Generator(device="cuda").manual_seed(1)
    stack = torch.rand((n, h, w), device="cuda", generator=g)
    bg = photon.piv_background(stack.data_ptr(), h * w, n, w, h, 0)
    k = 2 * r + 1

    def torch_chain():
        d = (stack - bg).clamp_min(0).unsqueeze(1)
        mn, mx = -F.max_pool2d(-d, k, 1, r), F.max_pool2d(d, k, 1, r)
        lo, hi = F.avg_pool2d(mn, k, 1, r, count_include_pad=False), F.avg_pool2d(mx, k, 1, r, count_include_pad=False)
        return (d - lo).clamp_min(0) / (hi - lo).clamp_min(floor)

    def ms(fn, calls_per_round=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls_per_round):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls_per_round

    calls = {
        "background min": lambda: photon.piv_background(stack.data_ptr(), h * w, n, w, h, 0),
        "torch.amin": lambda: torch.amin(stack, 0),
        "background mean": lambda: photon.piv_background(stack.data_ptr(), h * w, n, w, h, 1),
        "torch.mean": lambda: torch.mean(stack, 0),
        "chain r 5": lambda: photon.piv_preprocess(stack.data_ptr(), h * w, n, w, h, bg.data_ptr(), r, floor),
        "torch chain": torch_chain,
    }
    times = {name: [] for name in calls}
    for rep in range(7):                                        # two warm-up rounds, then five
        for name, fn in calls.items():
            t = ms(fn)
            if rep >= 2:
                times[name].append(t)
    med = {name: float(np.median(v)) for name, v in times.items()}
    copy = photon.measure_copy_gbs(1 << 28, 5)                  # float4 copy, read + write, GB/s
    frame_bytes = 4.0 * h * w
    moved = {"background min": (n + 1) * frame_bytes, "background mean": (n + 1) * frame_bytes, "chain r 5": (2 * n + 1) * frame_bytes}
    for ours, theirs in (("background min", "torch.amin"), ("background mean", "torch.mean"), ("chain r 5", "torch chain")):
        rate = moved[ours] / med[ours] * 1e-6
        print(f"{n} x {h} x {w}: {ours} {med[ours]:.4f} ms, {theirs} {med[theirs]:.4f} ms, ratio {med[ours] / med[theirs]:.3f}; "
              f"{rate:.0f} GB/s = {rate / copy:.2f} of the copy rate ({copy:.0f} GB/s)")
    assert med["background min"] <= med["torch.amin"]
    assert med["background mean"] <= med["torch.mean"]
    assert med["chain r 5"] <= med["torch chain"]
