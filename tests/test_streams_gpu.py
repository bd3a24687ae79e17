"""Every stream-taking entry point, and every pipeline of photon_amd/library.py, on a HELD-BACK non-blocking stream.

The header promises "asynchronous on `stream`" and the pipelines "everything runs on the current stream"; on the null
stream a launch, memset or copy on the wrong handle, a wrapper that drops stream=, or a torch helper on another stream all
give the right bytes.  Here the order is made deterministic instead of lucky: on a torch.cuda.Stream() (non-blocking with
respect to the null stream) a delay is queued first, then an event `gate`, then the copies that fill the inputs, which
until then hold in-contract poison (stream_cases.py), then the call.  Whatever part of the call does not run on that stream
executes during the delay, reads poison or unfinished intermediates, and the bytes differ from the same call made on the
null stream with everything synchronised -- the bytes the rest of the suite holds against the host models.

The delay is device work (torch.cuda._sleep), never a host spin, and each case proves that it held:
  * a call that returns without waiting: `gate` has not been reached when the call returns (DELAY_MS);
  * a call that waits for its stream: the delay, measured with events, is at least 10 x the host time the null-stream run
    of the same case needed to return (12.5 x is asked for, within [5, 100] ms).

Measured on an MI355X, not derived (each case prints its pair; `pytest -s`): the delay kernel counts 2.39e6 ticks per ms.
The slowest case that waits is the pipeline correlate_multigrid_mask: delay 12.49 ms against 1.000 ms of host time on the
null stream; the slowest entry point is photon_tomo_reconstruct (16 iterations, 12^3 voxels, 288 rays): 8.16 ms against
0.651 ms.  Every other waiting case returns within 0.5 ms and gets the 5 ms minimum.  The calls that do not wait return
within 0.03 ms (photon_dots_match, 2 memsets and 5 launches) and are held behind 20 ms.  The whole module takes 2.3 s.

photon_tomo_backproject and photon_tomo_reconstruct promise no repeatable bits in general (f64 atomics); their cases use
rays for which the sums do not depend on the order (stream_cases.tomo_axis_rays), and photon_trace's image (the
statistics window) is held to the 1e-12 of its norm that the suite allows two runs of one trace.
"""
import ctypes
import os
import time

import numpy as np
import pytest

import stream_cases as sc

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 20.0                       # calls that do not wait: hundreds of times the few launches' queuing time; `gate` proves it
WAIT_FACTOR, ASK_FACTOR = 10.0, 12.5  # calls that wait: measured delay >= WAIT_FACTOR x host time; ASK_FACTOR is queued
MIN_WAIT_MS, MAX_WAIT_MS = 5.0, 100.0


# ---- the harness ---------------------------------------------------------------------------------------------------------------
class Rig:
    """The side stream and the delay kernel's rate.  torch.cuda._sleep counts ticks of the shader clock, which the chip
    lowers and raises: the rate is the largest of three measurements behind a warm-up and of every delay seen since, so
    that a delay comes out as long as asked for or longer.  Every case checks the delay it got."""
    def __init__(self):
        import torch
        self.side = torch.cuda.Stream()                     # non-blocking with respect to the null stream
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(10_000_000)                       # the kernel's first launch; the clock comes up
        torch.cuda.synchronize()
        self.ticks_per_ms = 0.0
        for _ in range(3):
            begin.record()
            torch.cuda._sleep(4_000_000)
            end.record()
            end.synchronize()
            self.seen(4_000_000, begin.elapsed_time(end))
        print(f"delay kernel: {self.ticks_per_ms:.0f} ticks per ms")

    def queue_delay(self, ms):
        import torch
        ticks = int(ms * self.ticks_per_ms)
        torch.cuda._sleep(ticks)                            # on the current stream
        return ticks

    def seen(self, ticks, ms):
        self.ticks_per_ms = max(self.ticks_per_ms, ticks / ms)


@pytest.fixture(scope="module")
def rig(photon):
    return Rig()


def wait_delay_ms(host_s):
    return min(max(ASK_FACTOR * host_s * 1e3, MIN_WAIT_MS), MAX_WAIT_MS)


class HeldBack:
    """with HeldBack(rig, ms) as hb: the delay and `gate` are queued on the side stream, which is torch's current stream
    inside the block (the late copies and a pipeline go there).  hb.held() right after a call that does not wait;
    hb.finish() waits for the stream; hb.delay_ms the measured delay."""
    def __init__(self, rig, ms):
        import torch
        self.rig, self.ms = rig, ms
        self.begin, self.gate, self.done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        self.ctx = torch.cuda.stream(rig.side)

    def __enter__(self):
        self.ctx.__enter__()
        self.begin.record()
        self.ticks = self.rig.queue_delay(self.ms)
        self.gate.record()
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)

    def held(self):
        return not self.gate.query()

    def finish(self):
        import torch
        self.done.record(self.rig.side)
        self.done.synchronize()
        torch.cuda.synchronize()
        self.delay_ms = self.begin.elapsed_time(self.gate)
        self.rig.seen(self.ticks, self.delay_ms)
        return self.delay_ms


def assert_delay_held(name, waits, held, delay_ms, host_s):
    print(f"{name}: delay {delay_ms:.2f} ms, null-stream host time {host_s * 1e3:.3f} ms, "
          + ("waits for its stream" if waits else f"returned before the gate: {held}"))
    if waits:
        assert delay_ms >= WAIT_FACTOR * host_s * 1e3, (name, delay_ms, host_s * 1e3)
    else:
        assert held, f"{name}: the call returned after the delay had passed; nothing was held back"


def device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the cases' arrays are read-only


def allocate(case, real):
    """The device buffers of one run: inputs real or poisoned, outputs at the sentinel, scratch zeroed."""
    import torch
    bufs = {}
    for name, a in case.inputs.items():
        t = device(a)
        bufs[name] = t if real else torch.full_like(t, case.poison.get(name, 0))
    for name, (shape, dtype) in case.outputs.items():
        bufs[name] = torch.full(tuple(shape), sc.SENTINEL, dtype=getattr(torch, dtype), device="cuda")
    for name, nbytes in case.scratch.items():
        bufs[name] = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")
    return bufs


def pointers(bufs):
    return {name: ctypes.c_void_p(t.data_ptr()) for name, t in bufs.items()}


def snapshot(case, bufs):
    return {name: bufs[name].cpu().numpy().tobytes() for name in (*case.inputs, *case.outputs)}


def null_stream_run(photon, case):
    """The call on the null stream from the real inputs, everything synchronised, twice (the first pays module loads and
    kernel attributes; both must agree: "two calls return the same bits").  Returns (bytes per buffer, host results, the
    host time of the second call)."""
    import torch
    runs = []
    for _ in range(2):
        bufs = allocate(case, real=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = case.call(photon, pointers(bufs), None)
        host_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        runs.append((snapshot(case, bufs), host))
    assert runs[0] == runs[1], "two null-stream calls on the same inputs differ"
    for name in case.outputs:
        assert runs[1][0][name] != allocate_sentinel_bytes(case, name), f"{name} was not written at all"
    return runs[1][0], runs[1][1], host_s


def allocate_sentinel_bytes(case, name):
    shape, dtype = case.outputs[name]
    return np.full(tuple(shape), sc.SENTINEL, dtype=dtype).tobytes()


def held_back_run(photon, rig, case, name, waits, host_s, on_side=True):
    """Poisoned inputs, then on the side stream: delay, gate, the late copies of the real inputs, the call (on_side=False: the
    call is handed stream 0, the mistake this module exists to find)."""
    import torch
    staging = {k: device(a) for k, a in case.inputs.items()}
    bufs = allocate(case, real=False)
    torch.cuda.synchronize()
    with HeldBack(rig, wait_delay_ms(host_s) if waits else DELAY_MS) as hb:
        for k, t in staging.items():
            bufs[k].copy_(t)
    host = case.call(photon, pointers(bufs), ctypes.c_void_p(rig.side.cuda_stream) if on_side else None)
    held = hb.held()
    hb.finish()
    assert_delay_held(name, waits, held, hb.delay_ms, host_s)
    return snapshot(case, bufs), host


# ---- 2. the entry points -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(sc.CASES))
def test_entry_point_on_a_held_back_stream(photon, rig, name):
    spec = sc.CASES[name]
    case = spec.build(photon)
    want, want_host, host_s = null_stream_run(photon, case)
    got, got_host = held_back_run(photon, rig, case, name, spec.waits, host_s)
    assert got_host == want_host, (name, got_host, want_host)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{name}: {differ} differ from the null-stream run: part of the call did not run on its stream"


@gpu
def test_untouched_entries_keep_the_sentinel(photon, rig):
    """What a call does not write still holds the sentinel in the bytes the held-back runs are compared with: peaks, dots and
    pairs beyond the counts."""
    ch = sc.dots_chain()
    n = int(ch[0]["count"][0])
    for name, outs in (("dots_detect_scaled", ("peaks",)), ("dots_fit", ("dots", "status")), ("dots_match_with_predictor", ("pair", "shift"))):
        case = sc.CASES[name].build(photon)
        want, _, _ = null_stream_run(photon, case)
        for out in outs:
            shape, dtype = case.outputs[out]
            a = np.frombuffer(want[out], dtype=dtype).reshape(shape)
            assert (a[n:] == sc.SENTINEL).all() and not (a[:n] == sc.SENTINEL).any(), (name, out)


# ---- 4. the harness can fail ---------------------------------------------------------------------------------------------------
@gpu
def test_a_call_on_the_wrong_stream_is_seen(photon, rig):
    """The mistake, made on purpose and harmlessly: photon_optflow_terms (one launch) is handed stream 0 while its inputs are
    filled behind the delay on the side stream.  It runs at once, reads the zeros, and its bytes differ."""
    case = sc.optflow_terms_case()
    want, _, host_s = null_stream_run(photon, case)
    got, _ = held_back_run(photon, rig, case, "optflow_terms on stream 0", False, host_s, on_side=False)
    assert got["terms"] != want["terms"], "a launch on the null stream was not told apart: the side stream is not held back"
    assert all(got[k] == want[k] for k in case.inputs)                  # the late copies arrived; only the launch was early


# ---- the statistics window around a trace --------------------------------------------------------------------------------------
@gpu
def test_statistics_window_on_a_held_back_stream(photon, rig):
    """photon_scene_stats_begin / photon_scene_stats_end around one photon_trace, behind a trace that leaves the counters
    dirty: a zeroing that ran early (during the delay) would let the window count both traces.  The image is a sum of f64
    atomics: two runs agree to 1e-12 of its norm (tests/test_segments_gpu.py, tests/test_pool_gpu.py), the counters exactly."""
    import torch
    from photon_amd import scenes
    call = scenes.bos_scene(n_dots=6, points_per_dot=20, rays_per_source=100)
    H, W = call.image_shape
    base = np.random.default_rng(41).uniform(1.0, 2.0, H * W).astype(np.float32)    # photon_trace accumulates into the image
    scene = photon.scene_create(call)
    counters = ("rays_launched", "rays_on_sensor", "sensor_taps", "rays_marched", "traces")

    def window(img, stream):
        scene.trace(img.data_ptr(), None, 0, stream=stream)
        scene.stats_begin(stream)
        scene.trace(img.data_ptr(), None, 0, stream=stream)
        st = scene.stats_end(stream)
        return {k: int(getattr(st, k)) for k in counters}

    for _ in range(2):                                                  # the first run pays the scene's source list and module loads
        img = device(base)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_stats = window(img, 0)
        host_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        want = img.cpu().numpy().astype(np.float64)
    assert want_stats["traces"] == 1 and want_stats["rays_launched"] > 0 and want_stats["rays_on_sensor"] > 0
    assert np.abs(want - base).max() > 0

    staging, img = device(base), torch.zeros(H * W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with HeldBack(rig, wait_delay_ms(host_s)) as hb:
        img.copy_(staging)
    got_stats = window(img, rig.side.cuda_stream)
    hb.finish()
    assert_delay_held("stats_window", True, False, hb.delay_ms, host_s)
    got = img.cpu().numpy().astype(np.float64)
    scene.free()
    assert got_stats == want_stats
    print(f"stats_window: rel_l2 = {np.linalg.norm(got - want) / np.linalg.norm(want):.3e}")
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


# ---- 3. the pipelines on a current stream that is not the default -------------------------------------------------------------
def flatten(result):
    """A pipeline's result as a list of bytes and plain values (device tensors are copied back on the current stream)."""
    import torch
    if isinstance(result, dict):
        return [x for k in sorted(result) for x in [k, *flatten(result[k])]]
    if isinstance(result, (tuple, list)):
        return [x for r in result for x in flatten(r)]
    if isinstance(result, torch.Tensor):
        result = result.cpu().numpy()
    if isinstance(result, np.ndarray):
        return [str(result.dtype), result.shape, result.tobytes()]
    return [result]


def _mask():
    m = np.zeros(sc.ODD, np.uint8)
    m[30:55, 40:70] = 1
    return m


def _pair_inputs(shape=sc.ODD, **more):
    im1, im2 = sc.pair(shape)
    return dict(im1=im1, im2=im2, **more)


def _tomo_inputs():
    o, d = sc.tomo_axis_rays()                  # a voxel's sum does not depend on the order of its terms: stream_cases.tomo_axis_rays
    rng = np.random.default_rng(51)
    return dict(p=rng.normal(0.0, 3.0, o.shape[0]), origins=o, dirs=d)


def _gradient_inputs():
    rng = np.random.default_rng(52)
    return dict(gx=rng.normal(0.0, 1.0, (33, 47)), gy=rng.normal(0.0, 1.0, (33, 47)), w=rng.uniform(0.2, 1.0, (33, 47)))


def _frames():
    return np.stack([sc.pair(sc.SMALL, seed=60 + k)[0] + np.float32(0.1) for k in range(4)])


# name -> (waits for the result, inputs: name -> numpy, the call on the device tensors)
PIPELINES = {
    "correlate": (True, _pair_inputs, lambda p, t: p.correlate(t["im1"], t["im2"], win=32, step=16, radius=8)),
    "correlate_two_passes": (True, _pair_inputs, lambda p, t: p.correlate(t["im1"], t["im2"], win=32, step=16, radius=8, passes=2)),
    "correlate_deform": (True, _pair_inputs, lambda p, t: p.correlate_deform(t["im1"], t["im2"], win=32, step=16, radius=8, iterations=2)),
    "correlate_multigrid_mask": (True, lambda: _pair_inputs(mask=_mask()),
                                 lambda p, t: p.correlate_multigrid(t["im1"], t["im2"], schedule=((64, 32), (32, 16), (16, 8)),
                                                                    iterations=(1, 1, 1), radius=8, mask=t["mask"])),
    "correlate_multigrid_phase": (True, _pair_inputs, lambda p, t: p.correlate_multigrid(t["im1"], t["im2"], schedule=((32, 16), (16, 8)),
                                                                                         iterations=(1, 1), method="phase")),
    "correlate_multigrid_gaussian": (True, _pair_inputs, lambda p, t: p.correlate_multigrid(t["im1"], t["im2"], schedule=((32, 16), (16, 8)),
                                                                                            iterations=(1, 1), radius=8, weighting="gaussian")),
    "correlate_ensemble": (True, lambda: dict(frames1=np.stack([sc.pair(sc.SMALL, seed=10 + k)[0] for k in range(3)]),
                                              frames2=np.stack([sc.pair(sc.SMALL, seed=10 + k)[1] for k in range(3)])),
                           lambda p, t: p.correlate_ensemble(t["frames1"], t["frames2"], win=16, step=8, radius=4)),
    "displacement_uncertainty": (True, lambda: _pair_inputs(field=sc.grid_field(sc.ODD, 32, 16, seed=5)),
                                 lambda p, t: p.displacement_uncertainty(t["im1"], t["im2"], t["field"], win=32, step=16)),
    "correlation_predictor": (False, _pair_inputs, lambda p, t: p.correlation_predictor(t["im1"], t["im2"], win=32, step=16, radius=8)),
    "optical_flow": (True, lambda: _pair_inputs(sc.SMALL), lambda p, t: p.optical_flow(t["im1"], t["im2"], win=32, step=16, warps=2, iterations=20)),
    "track_dots": (True, lambda: dict(im1=sc.dots_pair()[0], im2=sc.dots_pair()[1], field=sc.dots_chain()["field"]),
                   lambda p, t: p.track_dots(t["im1"], t["im2"], 0.25, relative=True, predictor=(t["field"], 32, 16), max_dots=sc.MAX_DOTS,
                                             grid=(32, 16, 2, 1))),
    "preprocess_series": (False, lambda: dict(frames=_frames()),
                          lambda p, t: p.preprocess_series(t["frames"], background="min", minmax_radius=3, floor=0.05)),
    "integrate_gradient": (True, _gradient_inputs, lambda p, t: p.integrate_gradient(t["gx"], t["gy"], w=t["w"], hy=1.5, tol=0.0,
                                                                                   max_iter=sc.SOLVER_ITERATIONS)),
    "tomo_reconstruct": (True, _tomo_inputs, lambda p, t: p.tomo_reconstruct(t["p"], *sc.TOMO_GRID, t["origins"], t["dirs"], lam=0.5, tol=0.0,
                                                                            max_iter=sc.SOLVER_ITERATIONS)),
}


@gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_pipeline_on_a_held_back_current_stream(photon, rig, name):
    """The driver under `with torch.cuda.stream(side)`, its device-tensor inputs (passed through uncopied) filled behind the
    delay: the bytes of the same call with the default current stream."""
    import torch
    waits, make_inputs, run = PIPELINES[name]
    inputs = make_inputs()
    for _ in range(2):                                                  # the first call pays module loads and kernel attributes
        tensors = {k: device(a) for k, a in inputs.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = run(photon, tensors)
        host_s = time.perf_counter() - t0
        want = flatten(result)
        torch.cuda.synchronize()

    staging = {k: device(a) for k, a in inputs.items()}
    tensors = {k: torch.zeros_like(t) for k, t in staging.items()}     # poison: zeros are in every driver's contract
    torch.cuda.synchronize()
    with HeldBack(rig, wait_delay_ms(host_s) if waits else DELAY_MS) as hb:
        for k, t in staging.items():
            tensors[k].copy_(t)
        result = run(photon, tensors)
        held = hb.held()
        got = flatten(result)                                           # copies back on the side stream, behind the work
    hb.finish()
    assert_delay_held(name, waits, held, hb.delay_ms, host_s)
    assert len(got) == len(want)
    differ = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not differ, f"{name}: results {differ} differ from the run on the default stream: part of the driver left the current stream"


# ---- 5. the inventory (needs no GPU) -------------------------------------------------------------------------------------------
def test_every_stream_taking_entry_point_has_a_stream_case():
    """An entry point with a `void *stream` parameter cannot ship without a held-back case here, or a side-stream test
    elsewhere that is named beside it."""
    with open(os.path.join(ROOT, "include", "parallel_ray_tracing.h"), encoding="utf-8") as f:
        declared = sc.declared_stream_entry_points(f.read())
    covered = sc.covered_entry_points()
    assert len(declared) == len(set(declared)) == 34, declared
    assert not [e for e in declared if e not in covered], "no stream case for these entry points"
    assert not [e for e in covered if e not in declared], "cases for entry points the header does not declare"
    assert len(sc.COVERED_ELSEWHERE) == 8
    for entry, where in sc.COVERED_ELSEWHERE.items():
        for path in where.split(", "):
            assert os.path.exists(os.path.join(ROOT, path)), (entry, path)
    from photon_amd.library import SIGNATURES
    assert not [e for e in declared if e not in SIGNATURES]
