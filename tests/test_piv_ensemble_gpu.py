"""photon_piv_correlate_ensemble on the GPU (include/parallel_ray_tracing.h, section 14): one pair against
photon_piv_correlate bit for bit, the exact stacks against the f64 model bit for bit, particle stacks within section 5's
bounds, the addressing of a time series, the planes switch, repeats, flat windows, the refusals, the sparse stack the
feature is for, the two-pass driver, and one ensemble call against as many single calls on the clock."""
import ctypes

import numpy as np
import pytest

import piv_ensemble_cases as cs
import piv_tail_cases
import test_piv_correlation_gpu as single                 # CASES, particle_pair, device_correlate, the bounds of section 5
from photon_amd import piv_correlation as pc
from photon_amd import piv_ensemble as pe

pytestmark = pytest.mark.gpu

TAIL, SENTINEL = 3, 7


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def device_ensemble(photon, s1, s2, win, step, R, offset=None, planes=True, count=True):
    """photon_piv_correlate_ensemble on two stacks [N, h, w] (s2 None: s1 is a time series of N + 1 frames in one buffer),
    on output buffers TAIL windows longer than the grid and filled with a sentinel.  Returns (vectors [n, 4], flags [n],
    count [n] or None, planes [n, nS, nS] or None) after checking that the tails are untouched."""
    import torch
    a = torch.tensor(s1).cuda()
    h, w = a.shape[1:]
    if s2 is None:
        n_pairs, p2 = a.shape[0] - 1, ctypes.c_void_p(a.data_ptr() + 4 * h * w)
    else:
        b = torch.tensor(s2).cuda()
        n_pairs, p2 = a.shape[0], vp(b)
    n_rows, n_cols = pc.grid_shape((h, w), win, step)
    n, ns = n_rows * n_cols, 2 * R + 1
    off = torch.from_numpy(np.ascontiguousarray(offset, np.int32)).cuda() if offset is not None else None
    vec = torch.full(((n + TAIL) * 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    flg = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") if count else None
    pl = torch.full(((n + TAIL) * ns * ns,), float(SENTINEL), dtype=torch.float32, device="cuda") if planes else None
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    rc = photon.lib.photon_piv_correlate_ensemble(vp(a), p2, h * w, n_pairs, w, h, win, step, R, vp(off), vp(vec), vp(flg), vp(cnt), vp(pl),
                                                  ctypes.byref(r), ctypes.byref(c), None)
    torch.cuda.synchronize()
    assert rc == 0 and (r.value, c.value) == (n_rows, n_cols)
    vec, flg = vec.cpu().numpy(), flg.cpu().numpy()
    cnt = cnt.cpu().numpy() if count else None
    pl = pl.cpu().numpy() if planes else None
    assert (vec[4 * n:] == SENTINEL).all() and (flg[n:] == SENTINEL).all()
    assert cnt is None or (cnt[n:] == SENTINEL).all()
    assert pl is None or (pl[n * ns * ns:] == SENTINEL).all()
    return (vec[:4 * n].reshape(n, 4), flg[:n], cnt[:n] if count else None, pl[:n * ns * ns].reshape(n, ns, ns) if planes else None)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def case_offsets(case):
    win, R, step, shape, _, with_off = case
    if not with_off:
        return None
    return np.random.default_rng(R).integers(-3, 4, size=pc.grid_shape(shape, win, step) + (2,)).astype(np.int32)


# ---- one pair is section 5, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", single.CASES, ids=[f"w{c[0]}_r{c[1]}_s{c[2]}{'_off' if c[5] else ''}" for c in single.CASES])
def test_one_pair_returns_the_bits_of_photon_piv_correlate(photon, case):
    win, R, step, shape, shift, _ = case
    im1, im2 = single.particle_pair(shape, shift, seed=win * 100 + R + step)
    off = case_offsets(case)
    want_v, want_f, want_p = single.device_correlate(photon, im1, im2, win, step, R, off)
    v, f, c, p = device_ensemble(photon, im1[None], im2[None], win, step, R, off)
    assert v.tobytes() == want_v.tobytes() and f.tobytes() == want_f.tobytes() and p.tobytes() == want_p.tobytes()
    assert np.array_equal(c, np.where((want_f.ravel() & pc.FLAG_FLAT) != 0, 0, 1))


def test_one_pair_through_every_branch_of_the_peak_tail(photon):
    im1, im2, _, _ = piv_tail_cases.nine_windows()
    want_v, want_f, want_p = single.device_correlate(photon, im1, im2, 16, 16, 4)
    assert want_f.tolist() == [[6, 4, 5], [4, 0, 6], [5, 4, 4]]
    v, f, c, p = device_ensemble(photon, im1[None], im2[None], 16, 16, 4)
    assert v.tobytes() == want_v.tobytes() and f.tobytes() == want_f.tobytes() and p.tobytes() == want_p.tobytes()
    assert c.tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 1]


# ---- the exact stacks: the f64 model, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.exact_stacks()))
def test_exact_stacks_match_the_model_bit_for_bit(photon, name):
    """Flags, count, planes, peak and ratio equal the f64 model rounded to f32; dx and dy equal it or its f32 neighbour (the
    last bit of the Gaussian fit's f64 logarithm: the bound of section 5's exact test)."""
    s = cs.exact_stacks()[name]
    cs.assert_exact_stack(s)
    want_v, want_f, want_c, want_p = cs.exact_model(name)
    v, f, c, p = device_ensemble(photon, s.im1, s.im2, s.win, s.step, s.R, s.offset)
    assert np.array_equal(f, want_f) and np.array_equal(c, want_c)
    assert not (want_f & pc.FLAG_FLAT).any()
    diff = bits(p) != bits(want_p.astype(np.float32))
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5])
    want32 = want_v.astype(np.float32)
    for col, what in ((2, "peak"), (3, "ratio")):
        assert np.array_equal(bits(v[:, col]), bits(want32[:, col])), what
    one_ulp = 0
    for col in (0, 1):
        g, w = v[:, col], want32[:, col]
        near = (g == w) | (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
        assert near.all(), ("dx" if col == 0 else "dy", g[~near][:5], w[~near][:5])
        one_ulp += int((g != w).sum())
    print(f"{name}: {s.n_pairs} pairs, {f.size} windows, count {c.min()} to {c.max()}, {one_ulp} components one ulp from the model")


# ---- particle stacks: section 5's bounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.PARTICLE_STACKS, ids=[f"w{c[0]}_r{c[1]}_s{c[2]}{'_off' if c[5] else ''}" for c in cs.PARTICLE_STACKS])
def test_particle_stacks_are_close_to_the_host_model(photon, case):
    win, R, step, shape, shift, _ = case
    assert case in single.CASES
    s1, s2 = cs.particle_stack(shape, shift, cs.PARTICLE_PAIRS, seed=win + R)
    off = case_offsets(case)
    want_v, want_f, want_c, want_p = pe.correlate_ensemble_model(s1, s2, win, step, R, offset=off, planes=True)
    v, f, c, p = device_ensemble(photon, s1, s2, win, step, R, off)
    grid = want_f.shape
    assert np.array_equal(c.reshape(grid), want_c) and (want_c == cs.PARTICLE_PAIRS).all()
    clear = single.assert_close_to_the_host_model((v.reshape(grid + (4,)), f.reshape(grid), p.reshape(want_p.shape)), (want_v, want_f, want_p))
    assert clear.mean() > 0.5


# ---- addressing, the planes switch, repeats ---------------------------------------------------------------------------------
def test_a_time_series_in_one_buffer_gives_the_bytes_of_two_stacks(photon):
    s1, s2 = cs.particle_stack((70, 90), (1.4, -0.8), 4, seed=11)
    frames = np.concatenate([s1, s2[-1:]])
    series = device_ensemble(photon, frames, None, 16, 8, 4)
    stacks = device_ensemble(photon, frames[:-1], frames[1:], 16, 8, 4)
    assert same_bytes(series, stacks)
    assert (series[2] == 4).all()


@pytest.mark.parametrize("name", list(cs.exact_stacks()))
def test_without_planes_or_count_the_other_outputs_are_the_same_bytes(photon, name):
    s = cs.exact_stacks()[name]
    full = device_ensemble(photon, s.im1, s.im2, s.win, s.step, s.R, s.offset)
    bare = device_ensemble(photon, s.im1, s.im2, s.win, s.step, s.R, s.offset, planes=False)
    assert bare[3] is None and same_bytes(bare[:3], full[:3])
    bare = device_ensemble(photon, s.im1, s.im2, s.win, s.step, s.R, s.offset, planes=False, count=False)
    assert bare[2] is None and same_bytes(bare[:2], full[:2])


def test_two_calls_return_identical_bytes(photon):
    s1, s2 = cs.particle_stack((256, 256), (3.3, -2.7), 3, seed=5)
    for win, step, R in ((32, 16, 16), (64, 32, 32), (16, 8, 3)):
        assert same_bytes(device_ensemble(photon, s1, s2, win, step, R), device_ensemble(photon, s1, s2, win, step, R))


def test_a_window_flat_in_every_pair_is_flagged_and_the_others_are_untouched(photon):
    s1, s2 = cs.particle_stack((64, 96), (1.2, 0.7), 3, seed=9)
    base = device_ensemble(photon, s1, s2, 32, 32, 5)
    s1[:, 32:64, 32:64] = 0.37                  # window (1, 1) of im1 in every pair; (0, 2) in pair 1 only
    s1[1, 0:32, 64:96] = 0.11
    v, f, c, p = device_ensemble(photon, s1, s2, 32, 32, 5)
    dead, thin = 1 * 3 + 1, 0 * 3 + 2
    assert f[dead] == pc.FLAG_FLAT | pc.FLAG_OUTSIDE and c[dead] == 0 and np.isnan(v[dead]).all() and np.isnan(p[dead]).all()
    assert c[thin] == 2 and (f[thin] & pc.FLAG_FLAT) == 0 and np.isfinite(v[thin, :3]).all()
    rest = np.ones(6, bool)
    rest[[dead, thin]] = False
    assert (c[rest] == 3).all()
    for got, was in zip((v, f, c, p), base):
        assert got[rest].tobytes() == was[rest].tobytes()
    model = pe.correlate_ensemble_model(s1, s2, 32, 32, 5)
    assert np.array_equal(model[1].ravel(), f) and np.array_equal(model[2].ravel(), c)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.rand((3, 64, 80), device="cuda")
    vec = torch.full((64, 4), 7.0, device="cuda")
    flg = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p, v, f, k = (vp(t) for t in (im, vec, flg, cnt))
    good = dict(im1=p, im2=p, stride=64 * 80, pairs=3, width=80, height=64, win=16, step=8, radius=4, vec=v, flg=f)
    capfd.readouterr()
    for what, change in (("win 24", dict(win=24)), ("win 128", dict(win=128)), ("R 0", dict(radius=0)), ("R > win/2", dict(radius=9)),
                         ("step 0", dict(step=0)), ("image too small", dict(height=15, stride=80 * 15)), ("null im1", dict(im1=None)),
                         ("null im2", dict(im2=None)), ("vectors without flags", dict(flg=None)), ("no pair", dict(pairs=0)),
                         ("pairs < 0", dict(pairs=-2)), ("stride below one image", dict(stride=64 * 80 - 1)), ("stride 0", dict(stride=0)),
                         ("stride < 0", dict(stride=-64 * 80))):
        a = dict(good, **change)
        r, c = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_correlate_ensemble(a["im1"], a["im2"], a["stride"], a["pairs"], a["width"], a["height"], a["win"], a["step"],
                                             a["radius"], None, a["vec"], a["flg"], k, None, ctypes.byref(r), ctypes.byref(c), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, what
        assert len(err.strip().splitlines()) == 1 and "photon_piv_correlate_ensemble" in err, (what, err)
        assert r.value == -5 and c.value == -5, what
        assert (vec == 7.0).all().item() and (flg == 7).all().item() and (cnt == 7).all().item(), what
    r, c = ctypes.c_int(0), ctypes.c_int(0)                     # the size query: no launch, nothing written but the grid
    assert L.photon_piv_correlate_ensemble(p, p, 64 * 80, 3, 80, 64, 16, 8, 4, None, None, None, None, None, ctypes.byref(r), ctypes.byref(c),
                                           None) == 0
    torch.cuda.synchronize()
    assert (r.value, c.value) == ((64 - 16) // 8 + 1, (80 - 16) // 8 + 1)
    assert (vec == 7.0).all().item() and (flg == 7).all().item() and (cnt == 7).all().item()
    assert capfd.readouterr().err == ""


# ---- what the feature is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_sparse_pairs_give_a_field_only_together_on_the_device(photon, seed):
    """The device reproduces the model's valid vectors: all of the ensemble's, and each single pair's through
    photon_piv_correlate."""
    a, b = cs.sparse_stack(seed)
    want_ok, want_single, _ = cs.sparse_model(seed)
    vec, flags, count = photon.correlate_ensemble(np.array(a), np.array(b), cs.SPARSE_WIN, cs.SPARSE_STEP, cs.SPARSE_R)
    ok = cs.valid(vec)
    got_single = [cs.valid(photon.correlate(np.array(a[k]), np.array(b[k]), cs.SPARSE_WIN, cs.SPARSE_STEP, cs.SPARSE_R)[0])
                  for k in range(cs.SPARSE_PAIRS)]
    print(f"seed {seed} on the device: ensemble {int(ok.sum())} of {ok.size} within 0.5 px; single pairs "
          f"{[int(s.sum()) for s in got_single]} (model {[int(s.sum()) for s in want_single]})")
    assert np.array_equal(ok, want_ok) and ok.all()
    assert (count == cs.SPARSE_PAIRS).all() and not (flags & pc.FLAG_FLAT).any()
    for got, want in zip(got_single, want_single):
        assert np.array_equal(got, want) and not got.all()


def test_the_stack_driver_takes_tensors_arrays_and_time_series(photon):
    import torch
    s1, s2 = cs.particle_stack((70, 90), (1.4, -0.8), 3, seed=12)
    frames = np.concatenate([s1, s2[-1:]])
    want = device_ensemble(photon, frames[:-1], frames[1:], 32, 16, 16, planes=False)          # radius None = win // 2
    for args in ((frames,), (torch.from_numpy(frames).cuda(),), (frames[:-1], frames[1:]), (torch.from_numpy(frames[:-1]).cuda(), frames[1:])):
        vec, flags, count = photon.correlate_ensemble(*args, win=32, step=16)
        assert vec.shape == (3, 4, 4) and flags.shape == count.shape == (3, 4)
        assert same_bytes((vec, flags, count), want[:3])
    for bad in ((frames[0],), (frames[:1],), (s1, s2[:2])):
        with pytest.raises(ValueError):
            photon.correlate_ensemble(*bad)
    with pytest.raises(ValueError):
        photon.correlate_ensemble(frames, passes=3)
    with pytest.raises(ValueError):
        photon.correlate_ensemble(frames, win=24)


def test_two_passes_are_no_worse_than_one_when_the_shift_exceeds_the_radius(photon):
    shift = (7.4, -2.2)
    s1, s2 = cs.particle_stack((128, 128), shift, 6, seed=4)
    err = {}
    for passes in (1, 2):
        vec, flags, count = photon.correlate_ensemble(s1, s2, win=32, step=16, radius=6, passes=passes)
        assert (count == 6).all()
        err[passes] = np.hypot(vec[..., 0] - shift[0], vec[..., 1] - shift[1])
    m1, m2 = np.median(err[1]), np.median(err[2])
    print(f"shift {shift} px at radius 6, median |error|: 1 pass {m1:.4f} px, 2 passes {m2:.4f} px")
    assert m2 <= m1 + 0.01, (m1, m2)


# ---- on the clock -----------------------------------------------------------------------------------------------------------
def test_one_ensemble_call_is_no_slower_than_as_many_single_calls(photon):
    """1024^2, 8 pairs, device events, the two sides alternating after two warm-up rounds, medians of five: one ensemble call
    takes no longer than eight back-to-back photon_piv_correlate calls on the same pairs.  No margin: the ensemble call does
    a subset of that work (one peak tail and one launch instead of eight) on the same plan."""
    import torch
    rng = np.random.default_rng(1)
    n_pairs, h, w = 8, 1024, 1024
    frames = []
    for _ in range(n_pairs):
        n = 20_000
        x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
        frames.append([pc.particle_image((h, w), x + dx, y + dy).astype(np.float32) for dx, dy in ((0, 0), (3.3, -2.6))])
    a = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    b = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()

    def ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for win, step, R in ((32, 16, 8), (64, 32, 16)):
        def ensemble():
            return photon.piv_correlate_ensemble(a.data_ptr(), b.data_ptr(), h * w, n_pairs, w, h, win, step, R)

        def singles():
            return [photon.piv_correlate(a[k].data_ptr(), b[k].data_ptr(), w, h, win, step, R) for k in range(n_pairs)]
        calls = {"ensemble": ensemble, "eight single calls": singles}
        times = {k: [] for k in calls}
        for rep in range(7):                                    # two warm-up rounds, then five
            for k, fn in calls.items():
                t = ms(fn)
                if rep >= 2:
                    times[k].append(t)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"1024^2 x {n_pairs} pairs, win {win} step {step} R {R}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in med.items())
              + f", ratio {med['ensemble'] / med['eight single calls']:.3f}")
        assert med["ensemble"] <= med["eight single calls"]
