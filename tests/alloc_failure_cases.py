"""Every device allocation of a call failed in turn: the procedure, and the cases of tests/test_alloc_failures_gpu.py.

All device memory of the library is asked for in photon_pool.hip, and photon_selftest_fail_alloc makes any REQUEST there fail
(one pool_malloc, or one device_malloc that does not come from it), so the code behind "on failure ... is left unmodified"
and "non-zero HIP / argument error (message on stderr)" runs without memory pressure and without a wild address.

The procedure, `sweep(lib, case, name)`.  `lib` offers fail_alloc(first, count, first_attempt_only) and alloc_stats(); a
case offers setup() (the long-lived objects), fresh() (what every measured call starts from, e.g. a scene that has not
grown yet), fill() (outputs at stream_cases.SENTINEL in every byte), call() -> (rc, host results), outputs() -> name ->
bytes, teardown(), and says in `kept_on_failure` which outputs the header promises untouched on failure, in `tolerance`
how two clean runs compare (None: bit for bit), in `tolerance_from` the test that makes that comparison, and in `varies`
the outputs that differ between any two runs (a handle's address, a measured rate: only "written or not" is compared).

  clean run    A = requests of one clean call; its host results and output bytes are kept.  A second clean run equals it.
  n = 1 .. A   in three modes -- request n fails; every request from n on fails; only the first hipMalloc of request n fails:
               fill, arm, call, disarm.
    failed     (first two modes) rc != 0; stderr has at least one line, every line starts with "photon:", none is empty;
               the `kept_on_failure` outputs hold the sentinel in every byte; `failure_line`, if the case names one,
               occurs in a line.
    swallowed  rc == 0 although a request failed: the results equal the clean run and no stderr line says "HIP error".
    first try  the call succeeds, equals the clean run, and the retry counter rose by one.  For n = 1 a decoy call runs
               first; the blocks that retries returned then rise by exactly the idle blocks read just before the call.
    always     the hook reports at least one injected failure (request n was made), and a disarmed repeat on the same
               long-lived objects equals the clean run.
  teardown     outstanding blocks and bytes are what they were before setup().
Returns a report: A, and per mode the n that failed and the n that were swallowed.
"""
import contextlib
import ctypes
import os
import tempfile

import numpy as np

from stream_cases import SENTINEL

LLONG_MAX = 2 ** 63 - 1
MODES = ("single", "full", "first_attempt")
SENTINEL_BYTE = SENTINEL & 0xFF


@contextlib.contextmanager
def captured_stderr():
    """File descriptor 2 into a temporary file for the duration: what the C library prints.  Yields a list that holds the
    text afterwards."""
    import sys
    sys.stderr.flush()
    out = []
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield out
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            out.append(tmp.read().decode(errors="replace"))


class AllocCase:
    """The interface of the procedure; the defaults are those of a case without long-lived objects."""
    kept_on_failure = None          # names of the outputs untouched on failure; None: all of them
    tolerance = None                # None: bits; else |x - y| <= tolerance |y| (2-norms) per output
    tolerance_from = None           # the test that compares two clean runs of this call that way
    failure_line = None             # a text one stderr line of a failed call contains
    concurrent = False              # the call allocates from several threads (PHOTON_DEVICES)
    varies = ()                     # outputs whose bytes differ between two clean runs (a handle's address, a measured rate)

    def setup(self):
        pass

    def fresh(self):
        pass

    def fill(self):
        raise NotImplementedError

    def call(self):
        raise NotImplementedError

    def outputs(self):
        raise NotImplementedError

    def teardown(self):
        pass


def same_results(case, got, want, what):
    (got_out, got_host), (want_out, want_host) = got, want
    assert got_host == want_host, f"{what}: host results {got_host} differ from the clean run's {want_host}"
    assert list(got_out) == list(want_out), what
    for k in want_out:
        if k in case.varies:                                        # an address, a time: written or not is all two runs share
            assert holds_sentinel(got_out[k]) == holds_sentinel(want_out[k]), f"{what}: {k} was not written"
            continue
        if case.tolerance is None or not isinstance(want_out[k], np.ndarray):
            g, w = (v.tobytes() if isinstance(v, np.ndarray) else bytes(v) for v in (got_out[k], want_out[k]))
            assert g == w, f"{what}: output {k} differs from the clean run in bits"
        else:
            g, w = got_out[k].astype(np.float64), want_out[k].astype(np.float64)
            assert np.linalg.norm(g - w) <= case.tolerance * np.linalg.norm(w), \
                f"{what}: output {k} differs from the clean run beyond {case.tolerance} ({case.tolerance_from})"


def holds_sentinel(a) -> bool:
    raw = np.frombuffer(a.tobytes() if isinstance(a, np.ndarray) else bytes(a), np.uint8)
    return bool((raw == SENTINEL_BYTE).all())


def _delta(after, before, key):
    return after[key] - before[key]


_TALLIES = {}


def tally_of(lib):
    """What the sweeps of this process caused on `lib` (injected failures, retries): its hook must show nothing else."""
    return _TALLIES.setdefault(id(lib), (lib, dict(injected_failures=0, oom_retries=0)))[1]


def sweep(lib, case, name):
    before_setup = lib.alloc_stats()
    case.setup()
    try:
        report = _sweep(lib, case, name)
    finally:
        lib.fail_alloc(0)
        case.teardown()
    after = lib.alloc_stats()
    for key in ("outstanding_blocks", "outstanding_bytes"):
        assert after[key] == before_setup[key], \
            f"{name}: {key} is {after[key]} after teardown and was {before_setup[key]} before setup: a block leaked"
    return report


def _measured(case):
    case.fill()
    rc, host = case.call()
    return rc, (case.outputs(), host)


def _sweep(lib, case, name):
    case.fresh()
    s0 = lib.alloc_stats()
    rc, clean = _measured(case)
    A = _delta(lib.alloc_stats(), s0, "requests")
    assert rc == 0, f"{name}: the clean call failed with {rc}"
    assert A >= 1, f"{name}: the clean call made no allocation request"
    assert not any(holds_sentinel(v) for v in clean[0].values()), f"{name}: an output of the clean call still holds the sentinel"
    case.fresh()
    s0 = lib.alloc_stats()
    rc, again = _measured(case)
    assert rc == 0 and _delta(lib.alloc_stats(), s0, "requests") == A, f"{name}: a second clean call does not make {A} requests"
    same_results(case, again, clean, f"{name}: second clean run")

    report = dict(A=A, failed={m: [] for m in MODES}, swallowed={m: [] for m in MODES})
    for mode in MODES:
        for n in range(1, A + 1):
            what = f"{name}, {mode}, request {n} of {A}"
            if mode == "first_attempt" and n == 1:
                case.fresh()
                rc, _ = _measured(case)                          # the decoy: its blocks go back to the cache
                assert rc == 0, what
            case.fresh()
            case.fill()
            before = lib.alloc_stats()
            with captured_stderr() as err:
                lib.fail_alloc(n, LLONG_MAX if mode == "full" else 1, mode == "first_attempt")
                try:
                    rc, host = case.call()
                finally:
                    lib.fail_alloc(0)
            got = (case.outputs(), host)
            after = lib.alloc_stats()
            lines = err[0].splitlines()
            injected = _delta(after, before, "injected_failures")
            for key, count in tally_of(lib).items():
                tally_of(lib)[key] = count + _delta(after, before, key)
            assert injected >= 1, f"{what}: the request was never made ({_delta(after, before, 'requests')} requests)"
            assert mode == "full" or injected == 1, f"{what}: {injected} failures injected"
            if mode == "first_attempt":
                assert rc == 0, f"{what}: the call failed with {rc} although only the first attempt did: no retry\n{err[0]}"
                same_results(case, got, clean, what)
                assert _delta(after, before, "oom_retries") == 1, f"{what}: {_delta(after, before, 'oom_retries')} retries taken"
                if n == 1:
                    returned = _delta(after, before, "retry_blocks_returned")
                    # with worker threads another request may take a cached block between this one's number and its trim
                    assert returned == before["idle_blocks"] or (case.concurrent and 0 <= returned < before["idle_blocks"]), \
                        f"{what}: the retry returned {returned} blocks of {before['idle_blocks']} idle ones"
            elif rc != 0:
                report["failed"][mode].append(n)
                assert lines, f"{what}: the call failed with {rc} and said nothing on stderr"
                bad = [ln for ln in lines if not ln.startswith("photon:")]
                assert not bad, f"{what}: stderr lines that are empty or do not begin with 'photon:': {bad}"
                kept = list(got[0]) if case.kept_on_failure is None else case.kept_on_failure
                for k in kept:
                    assert holds_sentinel(got[0][k]), f"{what}: output {k} was written although the call failed with {rc}"
                if case.failure_line:
                    assert any(case.failure_line in ln for ln in lines), f"{what}: no stderr line contains {case.failure_line!r}: {lines}"
            else:
                report["swallowed"][mode].append(n)
                same_results(case, got, clean, f"{what} (the call succeeded)")
                bad = [ln for ln in lines if "HIP error" in ln]
                assert not bad, f"{what}: the call succeeded and printed {bad}"
            rc, repeat = _measured(case)                          # disarmed, on the same long-lived objects
            assert rc == 0, f"{what}: the disarmed repeat failed with {rc}: unusable after a failure"
            same_results(case, repeat, clean, f"{what}: disarmed repeat")
    return report


# ---- the cases of the GPU file -----------------------------------------------------------------------------------------------
def sentinel_bytes(obj):
    ctypes.memset(ctypes.addressof(obj), SENTINEL_BYTE, ctypes.sizeof(obj))


class EntryCase(AllocCase):
    """One entry point on device buffers and host outputs.  inputs: name -> numpy (uploaded once); outputs: name -> (shape,
    dtype) on the device; host: name -> a ctypes object or numpy array the call writes through; fn(lib, b, h, o) -> rc with b
    the device pointers, h the host objects and o what make(photon) created in setup() (name -> object with free()); release(h): what a successful call created is given back."""
    def __init__(self, photon, inputs, outputs, host, fn, release=None, results=None, make=None, **attrs):
        self.photon, self.inputs, self.device_outputs, self.host, self.fn = photon, inputs, outputs, host, fn
        self.release, self.results, self.make, self.objects = release, results, make, {}
        for k, v in attrs.items():
            setattr(self, k, v)

    def setup(self):
        import torch
        self.objects = self.make(self.photon) if self.make else {}      # long-lived handles (a volume, a flow): name -> object with free()
        self.bufs = {k: torch.from_numpy(np.array(a, order="C")).cuda() for k, a in self.inputs.items()}
        for k, (shape, dtype) in self.device_outputs.items():
            self.bufs[k] = torch.empty(tuple(shape), dtype=getattr(torch, dtype), device="cuda")
        torch.cuda.synchronize()

    def fill(self):
        import torch
        for k in self.device_outputs:
            self.bufs[k].view(torch.uint8).fill_(SENTINEL_BYTE)
        for obj in self.host.values():
            if isinstance(obj, np.ndarray):
                obj.view(np.uint8).fill(SENTINEL_BYTE)
            else:
                sentinel_bytes(obj)
        torch.cuda.synchronize()

    def call(self):
        import torch
        b = {k: ctypes.c_void_p(t.data_ptr()) for k, t in self.bufs.items()}
        rc = self.fn(self.photon.lib, b, self.host, self.objects)
        torch.cuda.synchronize()
        self._snapshot = {k: self.bufs[k].cpu().numpy() for k in self.device_outputs}      # before release() gives a handle back
        self._snapshot.update({k: (obj.copy() if isinstance(obj, np.ndarray) else bytes(obj)) for k, obj in self.host.items()})
        host = self.results(self.host) if (self.results and rc == 0) else None
        if rc == 0 and self.release:
            self.release(self.host)
        return rc, host

    def outputs(self):
        return self._snapshot

    def teardown(self):
        self.bufs = None
        for obj in self.objects.values():
            obj.free()
        self.objects = {}


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


CASES = {}          # name -> builder(photon, workdir) -> AllocCase


def case(name):
    def register(build):
        assert name not in CASES
        CASES[name] = build
        return build
    return register


# ---- solvers with pooled scratch: outputs and statistics untouched on failure, bits on success -----------------------------------
def _solver(photon, base, stats_type, fn):
    return EntryCase(photon, base.inputs, base.outputs, dict(stats=stats_type()), fn, results=lambda h: h["stats"].as_dict(),
                     tolerance_from="tests/test_dirty_memory_gpu.py::test_solver_on_recycled_pool_blocks (bytes)")


@case("integrate_gradient")
def _(photon, workdir):
    import stream_cases as sc
    from photon_amd.library import photon_integrate_stats_t
    base = sc.CASES["integrate_gradient"].build(None)
    ny, nx = base.outputs["phi"][0]
    return _solver(photon, base, photon_integrate_stats_t, lambda lib, b, h, o: lib.photon_integrate_gradient(
        b["gx"], b["gy"], b["w"], None, None, nx, ny, 1.0, 1.5, 0.0, sc.SOLVER_ITERATIONS, b["phi"], ctypes.byref(h["stats"]), None))


@case("tomo_reconstruct")
def _(photon, workdir):
    import stream_cases as sc
    from photon_amd.library import photon_tomo_stats_t
    base = sc.CASES["tomo_reconstruct"].build(None)
    dims, sp, og = sc._grid_args()
    n_rays = base.inputs["p"].size
    return _solver(photon, base, photon_tomo_stats_t, lambda lib, b, h, o: lib.photon_tomo_reconstruct(
        b["p"], b["w"], b["support"], *dims, _ptr(sp), _ptr(og), b["origins"], b["dirs"], n_rays, 0.5, 0.0, sc.SOLVER_ITERATIONS, b["f"],
        ctypes.byref(h["stats"]), None))


@case("tomo_reconstruct_deflections")
def _(photon, workdir):
    import stream_cases as sc
    from photon_amd.library import photon_tomo_stats_t
    from test_dirty_memory_gpu import deflections_solver_case
    base = deflections_solver_case()
    dims, sp, og = sc._grid_args()
    n_rays = base.inputs["g1"].size
    return _solver(photon, base, photon_tomo_stats_t, lambda lib, b, h, o: lib.photon_tomo_reconstruct_deflections(
        b["g1"], b["g2"], b["w"], b["support"], *dims, _ptr(sp), _ptr(og), b["origins"], b["dirs"], b["t1"], b["t2"], n_rays, 0.5, 0.0,
        sc.SOLVER_ITERATIONS, b["f"], ctypes.byref(h["stats"]), None))


# ---- one-shot buffers ---------------------------------------------------------------------------------------------------------------
@case("postprocess_u16")
def _(photon, workdir):
    import stream_cases as sc
    base = sc.CASES["postprocess_u16"].build(None)
    h_, w_ = sc.SMALL
    return EntryCase(photon, base.inputs, base.outputs, dict(rows=ctypes.c_int(), cols=ctypes.c_int()),
                     lambda lib, b, h, o: lib.photon_postprocess_u16(b["image"], w_, h_, 3.0, 12, 1, 0.0, 99, 0, 0, b["out"], ctypes.byref(h["rows"]),
                                                                     ctypes.byref(h["cols"]), None),
                     kept_on_failure=["out"])


@case("measure_copy_gbs")
def _(photon, workdir):
    return EntryCase(photon, {}, {}, dict(gbs=ctypes.c_double()),
                     lambda lib, b, h, o: lib.photon_measure_copy_gbs(4096, 1, ctypes.byref(h["gbs"])), varies=("gbs",))


@case("selftest_normal_range_math")
def _(photon, workdir):
    rng = np.random.default_rng(91)
    n = 300
    a, b_ = (rng.uniform(0.5, 2.0, n).astype(np.float32) for _ in range(2))
    return EntryCase(photon, {}, {}, {k: np.empty(n, np.float32) for k in ("quot", "rcp", "root")},
                     lambda lib, b, h, o: lib.photon_selftest_normal_range_math(n, _ptr(a), _ptr(b_), _ptr(h["quot"]), _ptr(h["rcp"]), _ptr(h["root"])))


@case("selftest_morton_order")
def _(photon, workdir):
    rng = np.random.default_rng(92)
    x, y = (rng.uniform(-1.0, 1.0, 1000).astype(np.float32) for _ in range(2))
    return EntryCase(photon, {}, {}, dict(perm=np.empty(777, np.int32)),
                     lambda lib, b, h, o: lib.photon_selftest_morton_order(_ptr(x), _ptr(y), 1000, 100, 777, _ptr(h["perm"])))


GAUSS = dict(spacing=(1000.0, 1000.0, 1000.0), origin=(-7500.0, -7500.0, 300000.0), rho0=1.225, amp=0.2, sigma=3000.0)


def gaussian_volume(photon, n=16, interpolation=1):
    g = GAUSS
    centre = [g["origin"][a] + g["spacing"][a] * (n - 1) / 2.0 for a in range(3)]
    return photon.volume_gaussian(n, g["spacing"], g["origin"], g["rho0"], g["amp"], centre, g["sigma"], interpolation)


def _rays(vol, n=256):
    """n rays from above the volume heading down through it (tests/test_parity_gpu.py::test_march_bit_exact)."""
    i = vol.info()
    rng = np.random.default_rng(93)
    lo, hi = np.array(i.min_bound), np.array(i.max_bound)
    pos = np.stack([rng.uniform(lo[a], hi[a], n) for a in range(3)], 1)
    pos[:, 2] = hi[2] + 500.0
    d = np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), -np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pos.astype(np.float32), d.astype(np.float32)


def _volume_rays(photon, queued, interpolation):
    """pos and dir are in/out: the call's copies start from the rays every time, so only `steps` can hold the sentinel."""
    n = 256
    state = {}

    def make(photon):
        vol = gaussian_volume(photon, 16, interpolation)
        state["rays"] = _rays(vol, n)
        return dict(vol=vol)

    def fn(lib, b, h, o):
        h["pos"][:], h["dir"][:] = state["rays"]
        if queued:
            return lib.photon_trace_volume_rays_queued(o["vol"].handle, 2, n, _ptr(h["pos"]), _ptr(h["dir"]), 2)
        return lib.photon_trace_volume_rays(o["vol"].handle, 2, n, _ptr(h["pos"]), _ptr(h["dir"]), _ptr(h["steps"]))
    host = dict(pos=np.empty((n, 3), np.float32), dir=np.empty((n, 3), np.float32))
    if not queued:
        host["steps"] = np.empty(n, np.int32)
    return EntryCase(photon, {}, {}, host, fn, make=make, kept_on_failure=[] if queued else ["steps"])


case("trace_volume_rays")(lambda photon, workdir: _volume_rays(photon, False, 1))
case("trace_volume_rays_queued_linear")(lambda photon, workdir: _volume_rays(photon, True, 1))
case("trace_volume_rays_queued_cubic")(lambda photon, workdir: _volume_rays(photon, True, 2))


@case("volume_sample")
def _(photon, workdir):
    n = 200
    state = {}

    def make(photon):
        vol = gaussian_volume(photon, 16, 2)
        i = vol.info()
        rng = np.random.default_rng(94)
        state["coords"] = np.stack([rng.uniform(i.min_bound[a], i.max_bound[a], n) for a in range(3)], 1).astype(np.float32)
        return dict(vol=vol)
    return EntryCase(photon, {}, {}, dict(out=np.empty((n, 4), np.float32)),
                     lambda lib, b, h, o: lib.photon_volume_sample(o["vol"].handle, n, _ptr(state["coords"]), _ptr(h["out"])), make=make)


# ---- creators: *out starts at a recognisable non-null value and keeps it on failure ---------------------------------------------------
def _creator(photon, fn, free, make=None, host=None, results=None, **attrs):
    """fn(lib, out, h, o) -> rc with out = byref(the handle); results(lib, handle, h) is read before the handle is freed."""
    host = dict(host or {}, handle=ctypes.c_void_p())
    got = {}

    def call(lib, b, h, o):
        rc = fn(lib, ctypes.byref(h["handle"]), h, o)
        got["results"] = results(lib, h["handle"], h) if (results and rc == 0) else None
        return rc
    return EntryCase(photon, {}, {}, host, call, release=lambda h: getattr(photon.lib, free)(h["handle"]), results=lambda h: got["results"],
                     make=make, varies=("handle",), **attrs)


def _volume_bytes(lib, handle, h):
    from photon_amd.library import photon_volume_info_t
    info = photon_volume_info_t()
    assert lib.photon_volume_info(handle, ctypes.byref(info)) == 0
    out = np.empty((info.nz, info.ny, info.nx, 4), np.float32)
    assert lib.photon_volume_download(handle, int(info.interpolation == 2), _ptr(out)) == 0
    return bytes(info), out.tobytes()


def _density(n):
    from photon_amd import scenes
    g = GAUSS
    return scenes.gaussian_blob_density(n, g["spacing"][0], g["origin"], sigma=g["sigma"])


for _interp in (1, 2):
    @case(f"volume_from_density_interp{_interp}")
    def _(photon, workdir, interp=_interp):
        rho = np.ascontiguousarray(_density(9), np.float32)
        sp, og = np.array(GAUSS["spacing"]), np.array(GAUSS["origin"])
        return _creator(photon, lambda lib, out, h, o: lib.photon_volume_from_density(_ptr(rho), 9, 9, 9, _ptr(sp), _ptr(og), interp, out),
                        "photon_volume_free", results=_volume_bytes)

    @case(f"volume_load_nrrd_interp{_interp}")
    def _(photon, workdir, interp=_interp):
        from photon_amd import scenes
        path = scenes.write_nrrd(os.path.join(workdir, "alloc_failures_12.nrrd"), _density(12), GAUSS["spacing"], GAUSS["origin"]).encode()
        return _creator(photon, lambda lib, out, h, o: lib.photon_volume_load_nrrd(path, interp, out), "photon_volume_free", results=_volume_bytes)

    @case(f"volume_gaussian_interp{_interp}")
    def _(photon, workdir, interp=_interp):
        sp, og = np.array(GAUSS["spacing"]), np.array(GAUSS["origin"])
        centre = og + sp * 7.5
        return _creator(photon, lambda lib, out, h, o: lib.photon_volume_gaussian(16, 16, 16, _ptr(sp), _ptr(og), GAUSS["rho0"], GAUSS["amp"], _ptr(centre),
                                                                                  GAUSS["sigma"], interp, out),
                        "photon_volume_free", results=_volume_bytes)


@case("density_gaussian_write_nrrd")
def _(photon, workdir):
    """No handle and no array: the output is the file, read back as the call's result."""
    path = os.path.join(workdir, "alloc_failures_gauss8.nrrd")
    sp, og = np.array(GAUSS["spacing"]), np.array(GAUSS["origin"])
    centre = og + sp * 3.5

    def fn(lib, b, h, o):
        if os.path.exists(path):
            os.remove(path)
        h["rc"].value = lib.photon_density_gaussian_write_nrrd(path.encode(), 8, 8, 8, _ptr(sp), _ptr(og), GAUSS["rho0"], GAUSS["amp"], _ptr(centre),
                                                               GAUSS["sigma"])
        return h["rc"].value
    return EntryCase(photon, {}, {}, dict(rc=ctypes.c_int()), fn, results=lambda h: open(path, "rb").read(), kept_on_failure=[])


def _flow_grid():
    from photon_amd import piv_pairs as pp
    return pp.uniform_flow((40.0, -25.0, 5.0), PIV_BOX[0], PIV_BOX[1], 3)


PIV_BOX = ((-3.0e4, -3.0e4, -7.5e3), (3.0e4, 3.0e4, 7.5e3))
PIV_CDF = np.cumsum(np.full(27, 1.0 / 27.0))
Z_OBJECT = 7.0e5


def _sources_bytes(lib, handle, h):
    n = lib.photon_sources_count(handle)
    out = [np.empty(n, t) for t in (np.float32, np.float32, np.float32, np.float64, np.int32)]
    assert lib.photon_sources_download(handle, *(_ptr(a) for a in out)) == 0
    return tuple(a.tobytes() for a in out)


@case("flow_from_grid")
def _(photon, workdir):
    u, v, w, spacing, origin = _flow_grid()
    comps = [np.ascontiguousarray(a, np.float32) for a in (u, v, w)]
    nz, ny, nx = comps[0].shape
    sp, og = np.array(spacing, np.float64), np.array(origin, np.float64)
    return _creator(photon, lambda lib, out, h, o: lib.photon_flow_from_grid(*(_ptr(c) for c in comps), nx, ny, nz, _ptr(sp), _ptr(og), out),
                    "photon_flow_free")


def _piv_args(seed, n):
    lo, hi = (np.array(v, np.float64) for v in PIV_BOX)
    return (seed, n, _ptr(lo), _ptr(hi), Z_OBJECT, 730.0, 500.0, _ptr(PIV_CDF), PIV_CDF.size), (lo, hi)


@case("sources_piv")
def _(photon, workdir):
    args, keep = _piv_args(1234, 1501)
    return _creator(photon, lambda lib, out, h, o: lib.photon_sources_piv(*args, out), "photon_sources_free", results=_sources_bytes, keep=keep)


@case("sources_bos")
def _(photon, workdir):
    from photon_amd import scenes
    centres, disc = scenes.bos_pattern(n_dots=9, points_per_dot=31, seed=8)
    dx, dy, tx, ty = (np.ascontiguousarray(a, np.float64) for a in (centres[:, 0], centres[:, 1], disc[:, 0], disc[:, 1]))
    return _creator(photon, lambda lib, out, h, o: lib.photon_sources_bos(_ptr(dx), _ptr(dy), dx.size, _ptr(tx), _ptr(ty), tx.size, Z_OBJECT, 10.0, out),
                    "photon_sources_free", results=_sources_bytes)


@case("sources_piv_advected")
def _(photon, workdir):
    """With a diameter table, a flow and world_xyz, so that every block of the call is asked for.  world_xyz is not promised
    untouched; it is compared on success."""
    n = 1501
    args, keep = _piv_args(21, n)
    return _creator(photon, lambda lib, out, h, o: lib.photon_sources_piv_advected(*args, o["flow"].handle, 1.0, 4, _ptr(h["world"]), out),
                    "photon_sources_free", make=lambda photon: dict(flow=photon.flow_from_grid(*_flow_grid())),
                    host=dict(world=np.empty((n, 3), np.float64)), results=_sources_bytes, keep=keep, kept_on_failure=["handle", "world"])


def scene_args(call, out, sources=()):
    """The arguments of photon_scene_create (photon_amd.library.PhotonLibrary._scene_create); the packed structs are returned
    as well: they must outlive the call."""
    packed = call.pack()
    sd, ls, elems, centers, planes, sysidx, cam = packed
    return (ctypes.c_float(call.lens_pitch), ctypes.c_float(call.image_distance), ctypes.byref(sd), call.scattering_type.encode(), ctypes.byref(ls),
            *sources, int(call.lightray_number_per_particle), ctypes.c_float(call.beam_wavelength), ctypes.c_float(call.aperture_f_number),
            len(call.elements), _ptr(centers), elems, _ptr(planes), _ptr(sysidx), ctypes.byref(cam), ctypes.c_float(call.ray_cone_pitch_ratio),
            out), packed


@case("scene_create_mie")
def _(photon, workdir):
    from photon_amd import scenes
    call = scenes.piv_scene(n_particles=300, rays_per_source=16, mie=True, polydisperse=True, seed=3, n_pixels=64)

    def fn(lib, out, h, o):
        args, keep = scene_args(call, out)
        return lib.photon_scene_create(*args)
    return _creator(photon, fn, "photon_scene_free")


@case("scene_create_large_sources")
def _(photon, workdir):
    """70 000 sources: every source array is beyond the 256 KiB of the scene's one packed upload and gets a block of its own."""
    from photon_amd import scenes
    call = scenes.piv_scene(n_particles=70_000, rays_per_source=2, mie=False, seed=4, n_pixels=64)

    def fn(lib, out, h, o):
        args, keep = scene_args(call, out)
        return lib.photon_scene_create(*args)
    return _creator(photon, fn, "photon_scene_free")


@case("scene_create_from_sources")
def _(photon, workdir):
    from photon_amd import scenes
    call = scenes.piv_scene(n_particles=300, rays_per_source=16, mie=True, polydisperse=True, seed=3, n_pixels=64)

    def fn(lib, out, h, o):
        args, keep = scene_args(call, out, (o["sources"].handle,))
        return lib.photon_scene_create_from_sources(*args)
    return _creator(photon, fn, "photon_scene_free",
                    make=lambda photon: dict(sources=photon.sources_piv(77, 300, *PIV_BOX, Z_OBJECT, 730.0, 500.0, PIV_CDF)))


# ---- calls that grow a scene ------------------------------------------------------------------------------------------------------------
POOL_TOLERANCE = dict(tolerance=1e-12, tolerance_from="tests/test_pool_gpu.py::test_block_cache_recycles_and_trims (same)")


def grow_call(workdir=None):
    """About 2 000 sources x 16 rays on a 256 x 256 sensor; the dot field is wider than the sensor sees, so the source cull
    of the volume-free path has sources to drop (its list is then asked for)."""
    from photon_amd import scenes
    return scenes.bos_scene(n_dots=20, points_per_dot=100, rays_per_source=16, n_pixels=256, seed=6)


class TraceCase(AllocCase):
    """photon_trace and its kin on a scene that every measured call gets FRESH (nothing grown yet: fresh()), so that the
    requests of a call repeat; the disarmed repeat then runs on the scene the armed call left behind.
    trace(lib, scene, vol, image, records) -> rc; prepare(scene): the setters of the variant."""
    def __init__(self, photon, trace, interpolation=0, prepare=None, records=False, **attrs):
        self.photon, self.trace, self.interpolation, self.prepare, self.with_records = photon, trace, interpolation, prepare, records
        self.scene = self.vol = None
        for k, v in dict(POOL_TOLERANCE, **attrs).items():
            setattr(self, k, v)

    def setup(self):
        import torch
        self.rt_call = grow_call()
        h, w = self.rt_call.image_shape
        self.image = torch.empty(h * w, dtype=torch.float32, device="cuda")
        self.records = torch.empty((self.rt_call.num_sources, 8), dtype=torch.float64, device="cuda") if self.with_records else None
        self.vol = gaussian_volume_in_front(self.photon, self.interpolation) if self.interpolation else None

    def fresh(self):
        if self.scene is not None:
            self.scene.free()
        self.scene = self.photon.scene_create(self.rt_call)
        if self.prepare:
            self.prepare(self.scene)

    def fill(self):
        import torch
        self.image.view(torch.uint8).fill_(SENTINEL_BYTE)
        if self.records is not None:
            self.records.view(torch.uint8).fill_(SENTINEL_BYTE)
        torch.cuda.synchronize()

    def call(self):
        import torch
        rc = self.trace(self.photon.lib, self.scene, self.vol, ctypes.c_void_p(self.image.data_ptr()),
                        ctypes.c_void_p(self.records.data_ptr()) if self.records is not None else None)
        torch.cuda.synchronize()
        return rc, None

    def outputs(self):
        out = dict(image=self.image.cpu().numpy())
        if self.records is not None:
            out["records"] = self.records.cpu().numpy()
        return out

    def teardown(self):
        if self.scene is not None:
            self.scene.free()
        if self.vol is not None:
            self.vol.free()
        self.scene = self.vol = self.image = self.records = None


def gaussian_volume_in_front(photon, interpolation, n=32):
    """A 32^3 Gaussian blob between the lens and the dot pattern, as scenes.bos_volume places its volumes."""
    from photon_amd import scenes
    rho, sp, org = scenes.bos_volume(n)
    return photon.volume_from_density(rho, sp, org, interpolation)


def _trace(algorithm, begin=0, end=None):
    def trace(lib, scene, vol, image, records):
        e = scene.num_sources if end is None else end
        if records is not None:
            return lib.photon_trace_moments(scene.handle, vol.handle if vol else None, algorithm, begin, e, image, records, None)
        return lib.photon_trace(scene.handle, vol.handle if vol else None, algorithm, begin, e, image, None, None)
    return trace


# the image is read-modify-write: what a failed trace leaves in it is not promised; the procedure holds rc and stderr
TRACE = dict(kept_on_failure=[])
case("trace_without_volume")(lambda photon, workdir: TraceCase(photon, _trace(0), **TRACE))
case("trace_euler_linear")(lambda photon, workdir: TraceCase(photon, _trace(1), 1, **TRACE))
case("trace_rk4_linear")(lambda photon, workdir: TraceCase(photon, _trace(2), 1, **TRACE))
case("trace_rk4_cubic")(lambda photon, workdir: TraceCase(photon, _trace(2), 2, **TRACE))
case("trace_rk45_extra")(lambda photon, workdir: TraceCase(photon, _trace(3), 1, **TRACE))
case("trace_segmented_linear")(lambda photon, workdir: TraceCase(photon, _trace(2), 1, prepare=lambda s: s.set_march_segments(3), **TRACE))
case("trace_segmented_cubic")(lambda photon, workdir: TraceCase(photon, _trace(2), 2, prepare=lambda s: s.set_march_segments(3), **TRACE))
case("trace_lens_major")(lambda photon, workdir: TraceCase(photon, _trace(2), 2, prepare=lambda s: s.set_ray_order(1), **TRACE))
case("trace_moments")(lambda photon, workdir: TraceCase(photon, _trace(2), 1, records=True, **TRACE))
case("trace_moments_without_volume")(lambda photon, workdir: TraceCase(photon, _trace(0), records=True, **TRACE))


@case("set_march_profile_then_trace")
def _(photon, workdir):
    def trace(lib, scene, vol, image, records):
        rc = lib.photon_scene_set_march_profile(scene.handle, 1)
        return rc or _trace(2)(lib, scene, vol, image, records)
    return TraceCase(photon, trace, 1, **TRACE)


@case("trace_regrows_the_workspace")
def _(photon, workdir):
    """A trace of a quarter of the sources, then, without a wait in between, one of all of them: the workspace regrows
    behind the first launch (scene_reserve).  The image holds both traces."""
    def trace(lib, scene, vol, image, records):
        rc = _trace(2, 0, scene.num_sources // 4)(lib, scene, vol, image, records)
        return rc or _trace(2)(lib, scene, vol, image, records)
    return TraceCase(photon, trace, 1, **TRACE)


# ---- the drop-in call ---------------------------------------------------------------------------------------------------------------------
DEVICES_TOLERANCE = dict(tolerance=1e-7, tolerance_from="tests/test_devices_gpu.py::test_eight_shards_repeat_the_same_image (same)")


class RenderCase(AllocCase):
    """start_ray_tracing (void: `failed` = the image still holds the sentinel in every byte) or, with moments,
    photon_start_ray_tracing_moments.  cold: every call finds the device's volume cache stale (the file's mtime moves)."""
    failure_line = "image left untouched"

    def __init__(self, photon, rt_call, moments=False, cold=False, dump_dirs=(), **attrs):
        self.photon, self.rt_call, self.moments, self.cold, self.dump_dirs = photon, rt_call, moments, cold, dump_dirs
        self.kept_on_failure = ["image"]
        self.tick = 0
        for k, v in dict(DEVICES_TOLERANCE, **attrs).items():
            setattr(self, k, v)

    def setup(self):
        self.image = self.rt_call.new_image()
        self.records = np.empty((self.rt_call.num_sources, 8), np.float64) if self.moments else None

    def fresh(self):
        if self.cold:
            self.tick += 1
            os.utime(self.rt_call.density_grad_filename, ns=(10 ** 18 + self.tick * 10 ** 9,) * 2)

    def fill(self):
        self.image.view(np.uint8).fill(SENTINEL_BYTE)
        if self.records is not None:
            self.records.view(np.uint8).fill(SENTINEL_BYTE)
        for d in self.dump_dirs:
            for f in os.listdir(d):
                os.remove(os.path.join(d, f))

    def call(self):
        if self.moments:
            status = []
            self.rt_call.invoke(lambda *args: status.append(self.photon.start_ray_tracing_moments(*args)), self.image, extra=(_ptr(self.records),))
            assert (status[0] != 0) == holds_sentinel(self.image), f"rc {status[0]} and the image disagree about the call's outcome"
            return status[0], None
        self.rt_call.invoke(self.photon.start_ray_tracing, self.image)
        return int(holds_sentinel(self.image)), None

    def outputs(self):
        out = dict(image=self.image.copy())
        if self.records is not None:
            out["records"] = self.records.copy()
        for d in self.dump_dirs:
            for f in sorted(os.listdir(d)):
                out[f"{os.path.basename(d)}/{f}"] = np.fromfile(os.path.join(d, f), np.uint8)
        return out


def _render_call(workdir, volume, n_pixels=128):
    from photon_amd import scenes
    path = ""
    if volume:
        rho, sp, org = scenes.bos_volume(32)
        path = scenes.write_nrrd(os.path.join(workdir, f"alloc_failures_{volume}_32.nrrd"), rho, sp, org)
    return scenes.bos_scene(n_dots=20, points_per_dot=100, rays_per_source=16, n_pixels=n_pixels, seed=6, density_grad_filename=path)


for _moments in (False, True):
    _tag = "_moments" if _moments else ""
    case(f"start_ray_tracing{_tag}_without_volume")(lambda photon, workdir, m=_moments: RenderCase(photon, _render_call(workdir, ""), m))
    case(f"start_ray_tracing{_tag}_cold_volume")(lambda photon, workdir, m=_moments: RenderCase(photon, _render_call(workdir, "cold"), m, cold=True))
    case(f"start_ray_tracing{_tag}_warm_volume")(lambda photon, workdir, m=_moments: RenderCase(photon, _render_call(workdir, "warm"), m))


@case("start_ray_tracing_with_dumps")
def _(photon, workdir):
    """The image-2 call of conftest.dump_pair_calls: final and intermediate ray dumps, through a volume.  The dump files
    are outputs too: deleted before every call, compared after a successful one (files a failed call wrote are not promised away)."""
    from conftest import dump_pair_calls
    root = os.path.join(workdir, "alloc_failure_dumps")
    os.makedirs(root, exist_ok=True)
    call = dump_pair_calls(root)[1]
    return RenderCase(photon, call, dump_dirs=(call.lightray_position_save_path, call.lightray_direction_save_path))


# warmed up before the first reading: the device's volume cache outlives the case, and holds a volume of the case's size from then on
WARM = {name for name in CASES if "_volume" in name and name.startswith("start_ray_tracing")} | {"start_ray_tracing_with_dumps"}


def warm_up(case):
    """One clean call, so that the per-device volume cache (which outlives the case) holds the case's volume."""
    case.setup()
    case.fill()
    rc, _ = case.call()
    case.teardown()
    assert rc == 0


# ---- Python drivers: an armed failure raises PhotonError, the next call on the same object returns the clean result ----------------------
class DriverCase(AllocCase):
    """run(photon, tensors) -> the driver's result; rc = 1 when it raised PhotonError.  The drivers allocate their outputs
    themselves: a failed call hands nothing out, so nothing can be held to the sentinel."""
    kept_on_failure = []

    def __init__(self, photon, make_inputs, run):
        self.photon, self.make_inputs, self.run = photon, make_inputs, run

    def setup(self):
        import torch
        self.tensors = {k: torch.from_numpy(np.array(a, order="C")).cuda() for k, a in self.make_inputs().items()}
        torch.cuda.synchronize()

    def fill(self):
        self.result = None

    def call(self):
        import torch
        from photon_amd.library import PhotonError
        from test_streams_gpu import flatten
        try:
            self.result = flatten(self.run(self.photon, self.tensors))
        except PhotonError:
            torch.cuda.synchronize()
            return 1, None
        torch.cuda.synchronize()
        return 0, self.result

    def outputs(self):
        return {}

    def teardown(self):
        self.tensors = None


for _name in ("integrate_gradient", "tomo_reconstruct"):
    @case(f"driver_{_name}")
    def _(photon, workdir, name=_name):
        from test_streams_gpu import PIPELINES
        _, make_inputs, run = PIPELINES[name]
        return DriverCase(photon, make_inputs, run)


@case("driver_bos_density_reconstruct")
def _(photon, workdir):
    """bos_density.reconstruct: correlate (two passes), then integrate_vectors; the camera geometry is a small BOS scene's."""
    import stream_cases as sc
    from photon_amd import bos_density as bd
    from photon_amd import scenes
    geometry = scenes.bos_scene(n_dots=4, points_per_dot=4, rays_per_source=4, n_pixels=64)
    return DriverCase(photon, lambda: dict(zip(("im1", "im2"), sc.pair(sc.SMALL))),
                      lambda p, t: bd.reconstruct(p, t["im1"], t["im2"], geometry, 300000.0, 66300.0, 16, 8, passes=2))


@case("driver_piv_pair_frame")
def _(photon, workdir):
    """The second frame of a PIV pair as photon_amd.piv_pairs describes it: the particle field advected through a flow on the
    device, a scene from those sources, one trace.  Whatever was created is freed on the way out of a failure too."""
    from photon_amd import scenes
    pcall = scenes.piv_scene(n_particles=300, rays_per_source=16, mie=True, polydisperse=True, seed=3, n_pixels=64)
    z_object = float(np.mean(pcall.src_z))

    def run(photon, t):
        import torch
        made = []
        try:
            made.append(photon.flow_from_grid(*_flow_grid()))
            made.append(photon.sources_piv_advected(21, 300, *PIV_BOX, z_object, 730.0, 500.0, PIV_CDF, flow=made[0], t=1.0, steps=4))
            made.append(photon.scene_create_from_sources(pcall, made[1]))
            image = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
            made[2].trace(image.data_ptr())
            torch.cuda.synchronize()
            return image
        finally:
            for obj in reversed(made):
                obj.free()
    return DriverCase(photon, dict, run)
