"""Every entry point and every pipeline of photon_amd/library.py on memory whose previous contents the test controls.

The library promises "needs no defined start" in three places: photon_pool.hip hands freed device blocks to the next call of
the same size unzeroed, the dots and optical-flow entries take scratch from the caller without a word about its contents,
and every Python driver allocates its outputs and intermediates with torch.empty.  Elsewhere in the suite outputs start at
one sentinel, scratch at zero and torch.empty at zeroed pages or at the previous correct answer of the same shape: a kernel
that reads an output or a scratch word before it writes it, or leaves part of an output unwritten, gives the same answer
twice.  Here the start differs between the runs that are compared, and every comparison is byte equality.

1. Entry points (stream_cases.CASES, and the cases below for the entries that table lists as covered elsewhere).
   Clean runs: the null stream, everything synchronised, scratch zeroed, the outputs at sentinel -77 and then at +91.  An
   output element is WRITTEN when both runs give it the same bytes, UNTOUCHED when it holds each run's sentinel, and
   anything else fails: the result depends on what the output held.  Dirty runs: the outputs filled bytewise with 0xFF (NaN
   / -1) and then with 0x7F (3.39e38 / 1.38e306 / 2139062143); every written element equals the clean run, every untouched
   one still holds the fill, every input (in/out buffers among them) is compared whole, the host results are equal.
   Caller scratch: float-only scratch (photon_optflow_iterate's d_tmp) takes the two byte fills; scratch whose words become
   indices (d_scratch of photon_dots_detect and photon_dots_match) takes STALE contents -- what the same call left after a
   decoy: the case with every floating input reversed in flat order, integer and byte inputs kept -- and the repeating int32
   word 1, which as a count, offset, cursor, list entry or mask stays inside every buffer of the call: a read before the
   write shows as wrong bytes and never as a wild address.

   Which kernel writes and which reads each region of the two index scratch layouts (photon_dots.hip), in launch order; no
   word is read before the same call has written it:
     photon_dots_detect, pieces = detect_pieces(width, height), a multiple of 64:
       masks  u64[pieces]      written: detect_mask_kernel, every piece (the grid is pieces / 64 workgroups of 64 pieces)
                               read:    detect_write_kernel, piece < pieces
       counts int[pieces + 1]  written: detect_mask_kernel [0, pieces); scan_kernel rewrites [0, pieces) as offsets and
                               writes the total into [pieces] (never read)
                               read:    scan_kernel [0, pieces), after the mask kernel; detect_write_kernel [0, pieces)
     photon_dots_match, n1 / n2 = the clamped counts, cells = nx ny of the cell grid:
       tgt    f32[max1][2]     written: match_count_kernel, k < n1 (NaN for a dot that takes no part)
                               read:    match_fill_kernel and match_search_kernel k < n1; nearest<false> at list1 entries
       start1/start2 int[cells + 1] each, cur1/cur2 int[cells] each: one hipMemsetAsync on the call's stream zeroes all
                               4 cells + 2 words first
                               written: match_count_kernel (atomic counts), scan_kernel (offsets, [cells] = total)
                               read:    scan_kernel, match_fill_kernel (start + cursor), nearest (start[c], start[c + 1])
       list1  int[max1], list2 int[max2]
                               written: match_fill_kernel, one slot per counted dot: slots [0, total) are all filled, as
                               the fill tests what the count tested (a finite target; takes_part)
                               read:    nearest, slots [start[c], min(start[c + 1], max)) only
       jstar  int[max1], istar int[max2]
                               written: match_search_kernel, k < n1 and k < n2
                               read:    match_pair_kernel: jstar[k], k < n1; istar[j] with j = jstar[k] >= 0, an entry of
                               list2 and so a dot index < n2
     d_npaired is zeroed by its own hipMemsetAsync on the stream before match_pair_kernel adds to it.

2. photon_tomo_backproject, photon_tomo_reconstruct, photon_tomo_deflect_adjoint and photon_tomo_reconstruct_deflections
   add a voxel's terms with f64 atomics in no fixed order.  Their cases use rays for which the sums do not depend on the
   order, so these are held to BYTES as well, the deflection solver included (the tolerance of
   test_tomo_deflection_gpu.py::test_fixed_iteration_parity is not used): stream_cases.tomo_axis_rays for section 9; for the
   deflection adjoint the same rays with vectors in multiples of 1/4 and whole numbers in y and v (every product and sum is
   exact); for the deflection solver the same rays with t1 = e_y on the rays along x, e_x on the rays along y, t2 = 0, and
   positive weights only on the x rays of the even z slices and the y rays of the odd ones, the last row of each left out
   (deflections_solver_case: a voxel receives at most two terms that are not 0).

3. The drivers (PIPELINES of test_streams_gpu.py) with torch.empty replaced by a wrapper that allocates and then fills by
   dtype: floating NaN (a third run: the largest finite value), int32 -1, uint8 the int32 word 1.

4. photon_integrate_gradient, photon_tomo_reconstruct and photon_tomo_reconstruct_deflections on blocks the pool recycles
   from a decoy of the same sizes but another structure.

The module makes about 300 tiny calls and takes a few seconds; the classification, the fills, the decoys' contracts and a
lint of the drivers' allocations need no GPU.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import piv_preprocess_cases as ppc
import stream_cases as sc
from photon_amd import dot_tracking as dt
from photon_amd import piv_correlation as pc
from photon_amd import piv_preprocess as pp
from stream_cases import Case
from test_streams_gpu import PIPELINES, device, flatten, pointers, snapshot

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINELS = (-77, 91)
FILLS = (0xFF, 0x7F)


# ---- fills and the classification (numpy only) ---------------------------------------------------------------------------------
def byte_fill(shape, dtype, byte):
    """An array of `shape` and `dtype` whose every byte is `byte`."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    return np.full(n * dtype.itemsize, byte, np.uint8).view(dtype).reshape(shape)


def word_fill(nbytes, word=1):
    """`nbytes` bytes (a multiple of 4) of the repeating int32 `word`."""
    assert nbytes % 4 == 0
    return np.full(nbytes // 4, word, np.int32).view(np.uint8)


def element_bytes(a):
    """a [n elements] as u8 [n, itemsize]."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)


def same_elements(a, b):
    return (element_bytes(a) == element_bytes(b)).all(axis=1)


def classify(run_a, run_b, start_a, start_b):
    """Two runs of one call whose output started at start_a and at start_b (arrays of the output's shape): the masks (written,
    untouched, dependent) over the flat elements.  Written: the same bytes in both runs.  Untouched: each run still holds its
    start.  Dependent: neither -- the result depends on the output's previous contents."""
    assert not same_elements(start_a, start_b).any(), "the two starts must differ in every element"
    written = same_elements(run_a, run_b)
    untouched = same_elements(run_a, start_a) & same_elements(run_b, start_b)
    return written, untouched, ~(written | untouched)


def scratch_start(case, how):
    """name -> u8 array: caller scratch zeroed (None), filled with a byte, or with the int32 word 1 ("word")."""
    out = {}
    for name, nbytes in case.scratch.items():
        n = max(int(nbytes), 16)
        out[name] = np.zeros(n, np.uint8) if how is None else (word_fill(n) if how == "word" else np.full(n, how, np.uint8))
    return out


def decoy_inputs(case):
    """The case's inputs with every floating one reversed in flat order; integer and byte inputs (peaks, counts, pairs,
    status, offsets, masks, support) are kept, so every index stays in contract."""
    return {name: (np.ascontiguousarray(np.asarray(a).ravel()[::-1].reshape(np.shape(a))) if np.asarray(a).dtype.kind == "f" else a)
            for name, a in case.inputs.items()}


def check_case(case, run, name, index_scratch=False):
    """The whole procedure on one case.  run(out_start, scratch_start, inputs) -> (after, host, scratch_after): `after` holds
    every input and output by name as arrays, the other two the host results and the scratch bytes.  Returns the clean
    run's (after, host, written masks)."""
    shapes = {k: (tuple(shape), np.dtype(dtype)) for k, (shape, dtype) in case.outputs.items()}
    starts = [{k: np.full(shape, s, dtype) for k, (shape, dtype) in shapes.items()} for s in SENTINELS]
    (a, host_a, _), (b, host_b, _) = (run(start, scratch_start(case, None), case.inputs) for start in starts)
    assert host_a == host_b, (name, host_a, host_b)
    for k in case.inputs:
        assert a[k].tobytes() == b[k].tobytes(), f"{name}: input {k} differs between two clean runs"
    written = {}
    for k in shapes:
        w, u, bad = classify(a[k], b[k], starts[0][k], starts[1][k])
        assert not bad.any(), (f"{name}: {int(bad.sum())} elements of output {k} are neither written nor untouched (first at "
                               f"{np.flatnonzero(bad)[:5].tolist()}): the result depends on the output's previous contents")
        assert w.any(), f"{name}: output {k} was not written at all"
        written[k] = w

    if index_scratch:                                               # stale: what the same call leaves after the decoy
        _, _, stale = run(starts[0], scratch_start(case, None), decoy_inputs(case))
        scratches = [stale, scratch_start(case, "word")]
    else:
        scratches = [scratch_start(case, fill) for fill in FILLS]
    for fill, scratch in zip(FILLS, scratches):
        start = {k: byte_fill(shape, dtype, fill) for k, (shape, dtype) in shapes.items()}
        got, host, _ = run(start, scratch, case.inputs)
        what = f"{name}, outputs filled with {fill:#x}"
        assert host == host_a, (what, host, host_a)
        for k in case.inputs:
            assert got[k].tobytes() == a[k].tobytes(), f"{what}: input {k} differs from the clean run"
        for k in shapes:
            same, kept = same_elements(got[k], a[k]), same_elements(got[k], start[k])
            bad = written[k] & ~same
            assert not bad.any(), f"{what}: {int(bad.sum())} written elements of {k} differ from the clean run (first at {np.flatnonzero(bad)[:5].tolist()})"
            bad = ~written[k] & ~kept
            assert not bad.any(), f"{what}: {int(bad.sum())} untouched elements of {k} lost the fill (first at {np.flatnonzero(bad)[:5].tolist()})"
    return a, host_a, written


# ---- 5. the harness can fail: the classification and the fills on numpy arrays with a fake call (no GPU) ------------------------
def fake_run(case, behaviour):
    """A call on numpy arrays: out[:4] = 2 x[:4] and out[4:] stays; `behaviour` adds a bug."""
    def run(out_start, scratch, inputs):
        out = out_start["out"].copy()
        x = np.asarray(inputs["x"])
        out[:4] = 2.0 * x[:4]
        if behaviour == "reads_output":
            out[2] = out_start["out"][2] + x[2]                 # out += ..., as photon_tomo_backproject's v
        elif behaviour == "reads_output_where_finite":
            out[3] = x[3] if np.isfinite(out_start["out"][3]) and abs(out_start["out"][3]) < 1e30 else 0.0
        elif behaviour == "unwritten_tail":
            out[3] = out_start["out"][3]
        elif behaviour == "reads_scratch":
            out[1] = x[1] + float(scratch["tmp"].view(np.float32)[0])
        elif behaviour == "clobbers_beyond":
            out[5] = 0.0
        return dict(x=x.copy(), out=out), (4,), {k: v.copy() for k, v in scratch.items()}
    return run


def test_fills():
    assert np.isnan(byte_fill((2, 3), "float32", 0xFF)).all() and np.isnan(byte_fill((3,), "float64", 0xFF)).all()
    assert (byte_fill((3,), "int32", 0xFF) == -1).all() and (byte_fill((3,), "int16", 0xFF) == -1).all()
    assert (byte_fill((3,), "float32", 0x7F).view(np.uint32) == 0x7F7F7F7F).all() and (byte_fill((3,), "float64", 0x7F).view(np.uint64) == 0x7F7F7F7F7F7F7F7F).all()
    assert np.allclose(byte_fill((3,), "float32", 0x7F), 3.39e38, rtol=1e-2) and np.allclose(byte_fill((3,), "float64", 0x7F), 1.38e306, rtol=1e-2)
    assert (byte_fill((3,), "int32", 0x7F) == 2139062143).all() and byte_fill((2, 3), "float64", 0x7F).shape == (2, 3)
    assert (word_fill(16).view(np.int32) == 1).all() and word_fill(16).dtype == np.uint8 and word_fill(16).size == 16
    case = Case({}, {}, None, scratch=dict(s=40, tiny=0))
    assert scratch_start(case, None)["s"].size == 40 and scratch_start(case, None)["tiny"].size == 16
    assert (scratch_start(case, "word")["s"].view(np.int32) == 1).all() and (scratch_start(case, 0x7F)["s"] == 0x7F).all()


def test_classification_tells_written_untouched_and_dependent():
    sa, sb = np.full(6, -77.0), np.full(6, 91.0)
    a, b = sa.copy(), sb.copy()
    a[:3] = b[:3] = (1.0, -77.0, np.nan)                         # a true -77 and a NaN are written all the same
    a[3], b[3] = -76.0, 92.0                                      # out += 1
    written, untouched, bad = classify(a, b, sa, sb)
    assert written.tolist() == [True, True, True, False, False, False]
    assert untouched.tolist() == [False, False, False, False, True, True]
    assert bad.tolist() == [False, False, False, True, False, False]
    with pytest.raises(AssertionError):
        classify(a, b, sa, sa)


def test_the_procedure_passes_a_sound_call_and_fails_every_bug():
    x = np.arange(1.0, 9.0, dtype=np.float32)
    case = Case(dict(x=x), dict(out=((8,), "float32")), None, scratch=dict(tmp=16))
    after, host, written = check_case(case, fake_run(case, None), "sound")
    assert written["out"].tolist() == [True] * 4 + [False] * 4 and host == (4,) and (after["out"][:4] == 2.0 * x[:4]).all()
    for bug, message in (("reads_output", "neither written nor untouched"), ("reads_output_where_finite", "differ from the clean run"),
                         ("reads_scratch", "differ from the clean run")):
        with pytest.raises(AssertionError, match=message):
            check_case(case, fake_run(case, bug), bug)
    # An element the call forgets, or a constant beyond its extent, is the same in every run: the procedure reports the
    # extent (the written mask) and the GPU tests hold it to the documented one (BEYOND_THE_COUNT, and whole everywhere else).
    assert check_case(case, fake_run(case, "unwritten_tail"), "tail")[2]["out"].tolist() == [True] * 3 + [False] * 5
    assert check_case(case, fake_run(case, "clobbers_beyond"), "beyond")[2]["out"].tolist() == [True] * 4 + [False, True, False, False]


def test_index_scratch_gets_the_stale_and_the_word_fill_and_never_a_byte_fill():
    seen = []
    x = np.arange(1.0, 9.0, dtype=np.float32)
    case = Case(dict(x=x, n=np.array([3], np.int32)), dict(out=((8,), "float32")), None, scratch=dict(tmp=16))
    inner = fake_run(case, None)

    def run(out_start, scratch, inputs):
        seen.append((scratch["tmp"].copy(), np.asarray(inputs["x"]).copy(), inputs["n"]))
        after, host, _ = inner(out_start, scratch, inputs)
        after["n"] = np.asarray(inputs["n"]).copy()
        return after, host, dict(tmp=np.full(16, len(seen), np.uint8))       # what this call "left" in scratch
    check_case(case, run, "index", index_scratch=True)
    assert len(seen) == 5
    assert all((s == 0).all() for s, _, _ in seen[:3])                       # two clean runs and the decoy start from zeroes
    assert (seen[2][1] == x[::-1]).all() and seen[2][2] is case.inputs["n"]  # the decoy: floats reversed, integers kept
    assert (seen[3][0] == 3).all() and (seen[3][1] == x).all()               # stale: what the decoy's call left
    assert (seen[4][0].view(np.int32) == 1).all()
    assert not any((s == f).all() for s, _, _ in seen for f in FILLS)


# ---- the decoys stay in contract (no GPU) ----------------------------------------------------------------------------------------
class Sizes:
    """What the builders of the table ask the library for, without one: a scratch size and the sweeps per launch."""
    @staticmethod
    def dots_scratch_bytes(*args):
        return 64

    @staticmethod
    def optflow_iterations_per_launch():
        return 4


def test_decoys_keep_shapes_and_integers_and_reverse_the_floats():
    for name, spec in sc.CASES.items():
        case = spec.build(Sizes)
        decoy = decoy_inputs(case)
        assert list(decoy) == list(case.inputs)
        for k, a in case.inputs.items():
            a, d = np.asarray(a), np.asarray(decoy[k])
            assert d.shape == a.shape and d.dtype == a.dtype and d.flags["C_CONTIGUOUS"], (name, k)
            if a.dtype.kind == "f":
                assert d.tobytes() == a.ravel()[::-1].tobytes(), (name, k)
            else:
                assert d is case.inputs[k], (name, k)


def test_the_host_models_accept_the_decoys():
    """dot_tracking and piv_correlation take the decoys of the dots cases (whose stale scratch the GPU test uses) and of a
    correlator case without raising, and every index they return is inside its array."""
    h, w = sc.ODD
    im = decoy_inputs(sc.CASES["dots_detect_scaled"].build(Sizes))["im"]
    peaks, total = dt.detect_model(im, 0.25, dt.image_max_model(im), sc.MAX_DOTS)
    assert 0 < peaks.size <= sc.MAX_DOTS and peaks.min() >= 0 and peaks.max() < h * w and total >= peaks.size

    fit = decoy_inputs(sc.CASES["dots_fit"].build(None))
    n = int(fit["count"][0])
    dots, status = dt.fit_model(fit["im"], fit["peaks"][:n])
    assert dots.shape == (n, 4) and status.shape == (n,)

    m = decoy_inputs(sc.CASES["dots_match_with_predictor"].build(Sizes))
    n1, n2 = int(m["count1"][0]), int(m["count2"][0])
    pair, shift, npaired = dt.match_model(m["dots1"][:n1], m["status1"][:n1], m["dots2"][:n2], m["status2"][:n2], 3.0, (m["field"], 32, 16))
    assert pair.shape == (n1,) and shift.shape == (n1, 4) and 0 <= npaired <= min(n1, n2)
    assert ((pair >= -1) & (pair < n2)).all()

    wm = decoy_inputs(sc.CASES["dots_window_means"].build(None))
    n1 = int(wm["count1"][0])
    vectors, flags = dt.window_means_model(wm["dots1"][:n1], wm["pair"][:n1], wm["shift"][:n1], sc.ODD, 32, 16, 2, 1)[:2]
    assert vectors.shape[:2] == pc.grid_shape(sc.ODD, 32, 16) == flags.shape

    c = decoy_inputs(sc.CASES["correlate_win16"].build(None))
    out = pc.correlate_model(c["im1"], c["im2"], 16, 8, 4)
    assert out[0].shape[:2] == pc.grid_shape(sc.SMALL, 16, 8)


# ---- 3b. the drivers allocate through torch.empty, torch.zeros and torch.full alone (no GPU) -------------------------------------
def test_the_drivers_allocate_device_tensors_through_empty_zeros_and_full_alone():
    """test_pipeline_on_dirty_torch_empty replaces torch.empty: an uninitialised tensor from empty_like, new_empty or
    empty_strided (or their kin) would pass it by."""
    offenders = []
    for path in sorted(glob.glob(os.path.join(ROOT, "photon_amd", "*.py"))):
        for no, line in enumerate(open(path, encoding="utf-8"), 1):
            code = line.split("#", 1)[0]
            if re.search(r"\b(empty_like|new_empty|empty_strided|new_empty_strided|empty_permuted|empty_quantized)\b", code) \
                    or re.search(r"\btorch\.(Float|Double|Int|Byte|Long|Half)?Tensor\s*\(", code) or re.search(r"\.new\s*\(", code):
                offenders.append(f"{os.path.basename(path)}:{no}: {code.strip()}")
    assert not offenders, "uninitialised device tensors that do not come from torch.empty:\n" + "\n".join(offenders)
    text = open(os.path.join(ROOT, "photon_amd", "library.py"), encoding="utf-8").read()
    # the patch has something to catch: one site per allocation, the seven grid entry points share _grid_call's (44 sites before that)
    assert len(re.findall(r"\btorch\.empty\(", text)) >= 20 and "torch.empty(" in text[text.index("def _grid_call("):text.index("def version(")]
    assert not re.search(r"^\s*(from torch import|import torch\.)", text, flags=re.M) and not re.search(r"^import torch", text, flags=re.M), \
        "library.py must look torch.empty up per call (import torch inside the methods): the test patches the attribute"


# ---- the GPU side of the procedure ----------------------------------------------------------------------------------------------
def gpu_run(photon, case):
    """check_case's `run` on the device: the null stream, everything synchronised."""
    def run(out_start, scratch, inputs):
        import torch
        bufs = {k: device(a) for k, a in (*inputs.items(), *out_start.items(), *scratch.items())}
        torch.cuda.synchronize()
        host = case.call(photon, pointers(bufs), None)
        torch.cuda.synchronize()
        after = snapshot(case, bufs)
        shapes = {**{k: (np.shape(a), np.asarray(a).dtype) for k, a in inputs.items()}, **{k: (a.shape, a.dtype) for k, a in out_start.items()}}
        return ({k: np.frombuffer(after[k], dtype=shapes[k][1]).reshape(shapes[k][0]) for k in after}, host,
                {k: bufs[k].cpu().numpy() for k in scratch})
    return run


# ---- 1. every case of the stream table -------------------------------------------------------------------------------------------
BEYOND_THE_COUNT = {("dots_detect_scaled", "peaks"), ("dots_fit", "dots"), ("dots_fit", "status"), ("dots_match_with_predictor", "pair"),
                    ("dots_match_with_predictor", "shift")}


@gpu
@pytest.mark.parametrize("name", list(sc.CASES))
def test_entry_point_on_dirty_outputs_and_scratch(photon, name):
    case = sc.CASES[name].build(photon)
    index = any(e in ("photon_dots_detect", "photon_dots_match") for e in sc.CASES[name].entries)
    assert index == bool(case.scratch and "optflow" not in name), name     # index scratch: the dots cases; float scratch: d_tmp
    _, _, written = check_case(case, gpu_run(photon, case), name, index_scratch=index)
    # The extent: by contract nothing is left untouched but the entries beyond frame 1's count in the dots calls.
    n = int(sc.dots_chain()[0]["count"][0])
    for k, w in written.items():
        if (name, k) in BEYOND_THE_COUNT:
            rows = w.reshape(sc.MAX_DOTS, -1)
            assert rows[:n].all() and not rows[n:].any(), f"{name}: {k} is not written up to the count {n} and left alone beyond it"
        else:
            assert w.all(), f"{name}: {int((~w).sum())} elements of {k} are left unwritten"


# ---- 2. the entries the stream table lists as covered elsewhere -------------------------------------------------------------------
EXTRA = {}


def extra(name):
    def register(build):
        assert name not in EXTRA and name not in sc.CASES
        EXTRA[name] = build
        return build
    return register


BG_TAIL, GAP = 5, 7.0


def strided(frames, stride):
    """frames [n, h, w] laid `stride` floats apart, the gaps at GAP (test_piv_preprocess_gpu.py::strided)."""
    n, h, w = frames.shape
    buf = np.full((n - 1) * stride + h * w, GAP, np.float32)
    for k in range(n):
        buf[k * stride:k * stride + h * w] = frames[k].ravel()
    return buf


def _background(mode, stride, path):
    """7 frames of 33 x 31 (w h = 1023): stride 1024 takes the 16-byte path, 1023 the scalar one; the plane has a tail."""
    h, w, n = 33, 31, 7
    frames = ppc.particle_frames((h, w), n, seed=h + n)

    def call(photon, b, stream):
        assert photon.piv_background_path(b["frames"].value, stride, b["out"].value) == path
        photon._call("photon_piv_background", b["frames"], stride, n, w, h, mode, b["out"], stream)
        return path
    return Case(dict(frames=strided(frames, stride)), dict(out=((h * w + BG_TAIL,), "float32")), call)


for _mode in (pp.MODE_MIN, pp.MODE_MEAN):
    for _stride, _path in ((1024, 1), (1023, 0)):
        extra(f"background_mode{_mode}_path{_path}")(lambda photon, m=_mode, s=_stride, p=_path: _background(m, s, p))


@extra("preprocess_radius0_in_place")
def _(photon):
    """test_piv_preprocess_gpu.py::test_radius_zero_in_place: the frames are the output, so an input here."""
    h, w, n = 33, 47, 5
    frames = ppc.particle_frames((h, w), n, seed=1)
    stride = h * w + 2

    def call(photon, b, stream):
        photon._call("photon_piv_preprocess", b["frames"], stride, n, w, h, b["bg"], 0, 0.0, b["frames"], stride, stream)
    return Case(dict(frames=strided(frames, stride), bg=pp.background_model(frames, pp.MODE_MIN)), {}, call)


@extra("preprocess_radius3_background")
def _(photon):
    """70 x 90 (three tiles a side, the last ones partial), both strides above w h: the gaps and the tail stay untouched."""
    h, w, n = 70, 90, 3
    frames = ppc.particle_frames((h, w), n, seed=3)
    stride, out_stride = h * w + 5, h * w + 3

    def call(photon, b, stream):
        photon._call("photon_piv_preprocess", b["frames"], stride, n, w, h, b["bg"], 3, 0.05, b["out"], out_stride, stream)
    return Case(dict(frames=strided(frames, stride), bg=pp.background_model(frames, pp.MODE_MIN)),
                dict(out=(((n - 1) * out_stride + h * w + BG_TAIL,), "float32")), call)


def _frames_call(entry, data, outs, n_rays):
    dims, sp, og = sc._grid_args()

    def call(photon, b, stream):
        photon._call(entry, *(b[k] for k in data), *dims, sp.ctypes.data_as(ctypes.c_void_p), og.ctypes.data_as(ctypes.c_void_p), b["origins"],
                     b["dirs"], b["t1"], b["t2"], n_rays, *(b[k] for k in outs), stream)
    return call


@extra("tomo_deflect")
def _(photon):
    """The forward operator gathers per ray in a fixed order: any rays.  The axis rays and 112 oblique ones with random
    vectors, one of them not finite (a miss: both outputs are written as 0)."""
    rng = np.random.default_rng(71)
    o_axis, d_axis = sc.tomo_axis_rays()
    o = np.concatenate([o_axis, rng.uniform(-3.0, 14.0, (112, 3))])
    d = np.concatenate([d_axis, rng.normal(0.0, 1.0, (112, 3))])
    n_rays = o.shape[0]
    t1, t2 = rng.normal(size=(n_rays, 3)), rng.normal(size=(n_rays, 3))
    t2[2, 1] = np.nan
    call = _frames_call("photon_tomo_deflect", ("f",), ("g1", "g2"), n_rays)
    return Case(dict(f=rng.normal(0.0, 1.0, sc.TOMO_GRID[0][::-1]), origins=o, dirs=d, t1=t1, t2=t2),
                dict(g1=((n_rays,), "float64"), g2=((n_rays,), "float64")), call)


@extra("tomo_deflect_adjoint")
def _(photon):
    """v += D^T y: v is in/out by contract, so an input.  The axis rays cross every plane at a node (the bilinear fractions
    are 0 or 1), the vectors are multiples of 1/4, y and v whole numbers: every tap and every sum is exact in any order."""
    rng = np.random.default_rng(72)
    o, d = sc.tomo_axis_rays()
    n_rays = o.shape[0]
    t1, t2 = (rng.integers(-8, 9, (n_rays, 3)) / 4.0 for _ in range(2))
    y1, y2 = (rng.integers(-8, 9, n_rays).astype(np.float64) for _ in range(2))
    call = _frames_call("photon_tomo_deflect_adjoint", ("y1", "y2"), ("v",), n_rays)
    return Case(dict(y1=y1, y2=y2, origins=o, dirs=d, t1=t1, t2=t2, v=rng.integers(-8, 9, sc.TOMO_GRID[0][::-1]).astype(np.float64)), {}, call)


def deflections_solver_case(decoy=False):
    """photon_tomo_reconstruct_deflections on stream_cases' grid, rays and iteration count with bits that do not depend on the
    order of the adjoint's atomics.  Ray (j, k) along +x with t1 = e_y taps, in every plane i, voxel (i, j, k) with -1 and (i, j
    + 1, k) with +1 (the z fraction is 0, or 1 in the last slice: the other row's weights are 0, and so are all of t2 = 0);
    the ray of the last row j = 11 would tap the voxels of ray j = 10 again and takes no part (weight 0, as every ray that
    is not in its slice's family).  So a voxel of an even slice receives two terms that are not 0 (from rays j and j - 1),
    likewise along +y with t1 = e_x in the odd slices, and a + b = b + a; a term of weight 0 is an exact 0.
    decoy: other data, another support, other zero weights, the same sizes."""
    from photon_amd.library import photon_tomo_stats_t
    n = sc.TOMO_N
    dims, sp, og = sc._grid_args()
    rng = np.random.default_rng(74 if decoy else 73)
    o, d = sc.tomo_axis_rays()
    n_rays = o.shape[0]
    row, k = (v.ravel() for v in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))     # tomo_axis_rays' order, both families
    t1 = np.concatenate([np.tile([0.0, 1.0, 0.0], (n * n, 1)), np.tile([1.0, 0.0, 0.0], (n * n, 1))])
    takes_part = np.concatenate([(k % 2 == 0) & (row < n - 1), (k % 2 == 1) & (row < n - 1)])
    w = np.where(takes_part, rng.uniform(0.5, 2.0, n_rays), 0.0)
    kk, jj, ii = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    if decoy:
        w[3::7] = 0.0
        support = ((ii >= 2) & (jj <= 8)).astype(np.uint8)
    else:
        w[5::19] = 0.0
        support = (((ii - 5.5) ** 2 + (jj - 5.5) ** 2 + (kk - 5.5) ** 2) <= 30.0).astype(np.uint8)
    assert (w > 0).sum() >= 100

    def call(photon, b, stream):
        st = photon_tomo_stats_t()
        photon._call("photon_tomo_reconstruct_deflections", b["g1"], b["g2"], b["w"], b["support"], *dims, sp.ctypes.data_as(ctypes.c_void_p),
                     og.ctypes.data_as(ctypes.c_void_p), b["origins"], b["dirs"], b["t1"], b["t2"], n_rays, 0.5, 0.0, sc.SOLVER_ITERATIONS, b["f"],
                     ctypes.byref(st), stream)
        return st.as_dict()
    return Case(dict(g1=rng.normal(0.0, 3.0, n_rays), g2=rng.normal(0.0, 3.0, n_rays), w=w, support=support, origins=o, dirs=d, t1=t1,
                     t2=np.zeros((n_rays, 3))), dict(f=(dims[::-1], "float64")), call)


extra("tomo_reconstruct_deflections")(lambda photon: deflections_solver_case())


def test_the_deflection_solver_case_gives_a_voxel_at_most_two_terms():
    """deflections_solver_case's claim, counted with the host model's taps: over the rays of positive weight no voxel has
    more than two taps whose weight (for t1; t2 = 0) is not 0."""
    from photon_amd import tomography as tm
    case = deflections_solver_case()
    i = case.inputs
    taps = tm.deflection_taps(*sc.TOMO_GRID, i["origins"], i["dirs"], i["t1"], i["t2"])
    assert not (taps.weights[1] != 0).any()                         # t2 = 0
    assert set(np.unique(np.abs(taps.weights[0])).tolist()) == {0.0, 1.0}
    live = (i["w"][taps.ray] > 0) & (taps.weights[0] != 0)
    per_voxel = np.bincount(taps.voxel[live], minlength=taps.n_voxels)
    assert per_voxel.max() == 2 and (per_voxel > 0).sum() > 1000


@gpu
@pytest.mark.parametrize("name", list(EXTRA))
def test_entries_covered_elsewhere_on_dirty_outputs(photon, name):
    case = EXTRA[name](photon)
    _, host, written = check_case(case, gpu_run(photon, case), name)
    if name.startswith("background"):
        assert written["out"][:33 * 31].all() and not written["out"][33 * 31:].any()
    elif name == "preprocess_radius3_background":
        w, px, stride = written["out"], 70 * 90, 70 * 90 + 3
        keep = np.zeros(w.size, bool)
        for k in range(3):
            keep[k * stride:k * stride + px] = True
        assert (w == keep).all()                                    # the frames written, the gaps and the tail untouched
    elif name == "tomo_reconstruct_deflections":
        assert written["f"].all() and host["iterations"] == sc.SOLVER_ITERATIONS and host["rays_used"] > 100 and host["unknowns"] > 500
    else:
        assert all(w.all() for w in written.values())


@gpu
def test_an_accumulating_output_is_reported(photon):
    """photon_tomo_backproject computes v += A^T y by contract.  Handed to the procedure as an OUTPUT, v is neither written
    (the two runs differ by the sentinels) nor untouched wherever A^T y is not 0: the procedure must say so."""
    real = sc.CASES["tomo_backproject"].build(photon)
    v = real.inputs["v"]
    case = Case({k: a for k, a in real.inputs.items() if k != "v"}, dict(v=(v.shape, "float64")), real.call)
    with pytest.raises(AssertionError, match="neither written nor untouched"):
        check_case(case, gpu_run(photon, case), "tomo_backproject with v as an output")


# ---- 3. the drivers on dirty torch.empty ------------------------------------------------------------------------------------------
class DirtyEmpty:
    """torch.empty, then a fill by dtype on the current stream: floating `floating`, int32 -1 (no peak, no pair, every status
    bit, a count that clamps to 0), uint8 (the raw dots scratch) the repeating int32 word 1."""
    def __init__(self, real, floating):
        self.real, self.floating, self.calls = real, floating, 0

    def __call__(self, *args, **kwargs):
        import torch
        t = self.real(*args, **kwargs)
        if not t.is_cuda:
            return t
        self.calls += 1
        if t.dtype.is_floating_point:
            t.fill_(float("nan") if self.floating == "nan" else torch.finfo(t.dtype).max)
        elif t.dtype == torch.int32:
            t.fill_(-1)
        elif t.dtype == torch.uint8:
            assert t.numel() % 4 == 0
            t.view(torch.int32).fill_(1)
        else:
            raise AssertionError(f"torch.empty of {t.dtype}: no fill is defined for it")
        return t


@gpu
@pytest.mark.parametrize("name", list(PIPELINES))
def test_pipeline_on_dirty_torch_empty(photon, monkeypatch, name):
    import torch
    _, make_inputs, run = PIPELINES[name]
    inputs = make_inputs()
    want = flatten(run(photon, {k: device(a) for k, a in inputs.items()}))
    torch.cuda.synchronize()
    for floating in ("nan", "max"):
        dirty = DirtyEmpty(torch.empty, floating)
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", dirty)
            got = flatten(run(photon, {k: device(a) for k, a in inputs.items()}))
            torch.cuda.synchronize()
        assert dirty.calls >= 1, f"{name}: the driver never called torch.empty: the test would pass vacuously"
        assert len(got) == len(want)
        differ = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not differ, f"{name}: results {differ} differ when torch.empty returns {floating}-filled memory ({dirty.calls} allocations)"


# ---- 4. recycled pool blocks in the solvers ----------------------------------------------------------------------------------------
def integrate_case(ny, nx, decoy=False):
    """The real case: stream_cases' (weights with a hole, the outer frame fixed at 0).  decoy: the same size with another hole
    in w, a `fixed` mask with interior anchors at values that are not 0, and NaN gradients at other nodes -- so that what the
    real run expects to be zero or live in a recycled block is neither."""
    from photon_amd.library import photon_integrate_stats_t
    rng = np.random.default_rng(80 + 2 * ny + int(decoy))
    gx, gy, w = rng.normal(0.0, 1.0, (ny, nx)), rng.normal(0.0, 1.0, (ny, nx)), rng.uniform(0.2, 1.0, (ny, nx))
    inputs = dict(gx=gx, gy=gy, w=w)
    if decoy:
        w[ny // 3:ny // 3 + 2, nx // 3:nx // 3 + 3] = 0.0
        fixed = np.zeros((ny, nx), np.uint8)
        fixed[0, 0] = fixed[ny // 2, nx // 2] = fixed[ny - 1, nx // 4] = 1
        gx[ny - 1, nx - 1] = gy[ny // 2, 0] = np.nan
        inputs.update(fixed=fixed, value=rng.normal(5.0, 2.0, (ny, nx)))
    elif ny > 12:
        w[10:13, 20:24] = 0.0

    def call(photon, b, stream):
        st = photon_integrate_stats_t()
        photon._call("photon_integrate_gradient", b["gx"], b["gy"], b["w"], b.get("fixed"), b.get("value"), nx, ny, 1.0, 1.5, 0.0,
                     sc.SOLVER_ITERATIONS, b["phi"], ctypes.byref(st), stream)
        return st.as_dict()
    return Case(inputs, dict(phi=((ny, nx), "float64")), call)


def tomo_decoy():
    """stream_cases' tomo_reconstruct case with other data, another support and other zero weights."""
    real = sc.CASES["tomo_reconstruct"].build(None)
    rng = np.random.default_rng(81)
    n_rays = real.inputs["p"].size
    w = rng.uniform(0.5, 2.0, n_rays)
    w[3::11] = 0.0
    kk, jj, ii = np.meshgrid(*(np.arange(sc.TOMO_N),) * 3, indexing="ij")
    return Case(dict(real.inputs, p=rng.normal(0.0, 3.0, n_rays), w=w, support=((ii >= 3) & (kk <= 9)).astype(np.uint8)), real.outputs, real.call)


POOLED = {
    "integrate_33x47": (lambda: sc.CASES["integrate_gradient"].build(None), lambda: integrate_case(33, 47, decoy=True)),
    "integrate_2x2": (lambda: integrate_case(2, 2), lambda: integrate_case(2, 2, decoy=True)),
    "integrate_3x3": (lambda: integrate_case(3, 3), lambda: integrate_case(3, 3, decoy=True)),
    "tomo_reconstruct": (lambda: sc.CASES["tomo_reconstruct"].build(None), tomo_decoy),
    "tomo_reconstruct_deflections": (deflections_solver_case, lambda: deflections_solver_case(decoy=True)),     # bytes: see the module's head
}


def test_pool_decoys_have_the_sizes_of_their_cases():
    for name, (real, decoy) in POOLED.items():
        r, d = real(), decoy()
        assert r.outputs == d.outputs, name
        for k in r.inputs:
            assert np.shape(r.inputs[k]) == np.shape(d.inputs[k]) and np.asarray(r.inputs[k]).dtype == np.asarray(d.inputs[k]).dtype, (name, k)
        assert any(np.asarray(r.inputs[k]).tobytes() != np.asarray(d.inputs[k]).tobytes() for k in r.inputs), name


@gpu
@pytest.mark.parametrize("name", list(POOLED))
def test_solver_on_recycled_pool_blocks(photon, name):
    """Trim, the real case (A1, on fresh blocks), the decoy (its blocks go back to the cache), the real case again (A2, on
    the decoy's blocks, which the exact-size cache hands over): A2 is A1 in bytes and statistics."""
    if os.environ.get("PHOTON_POOL_MAX_MB", "").strip() == "0":
        pytest.skip("PHOTON_POOL_MAX_MB=0: the block cache is off, nothing is recycled")
    real, decoy = (make() for make in POOLED[name])
    start = {k: byte_fill(shape, dtype, 0xFF) for k, (shape, dtype) in real.outputs.items()}
    photon.lib.photon_trim_caches()
    a1, host1, _ = gpu_run(photon, real)(start, {}, real.inputs)
    d, host_d, _ = gpu_run(photon, decoy)(start, {}, decoy.inputs)
    a2, host2, _ = gpu_run(photon, real)(start, {}, real.inputs)
    out = next(iter(real.outputs))
    assert d[out].tobytes() != a1[out].tobytes(), f"{name}: the decoy computes what the case does"
    assert host2 == host1, (name, host1, host2)
    for k in a1:
        assert a2[k].tobytes() == a1[k].tobytes(), f"{name}: {k} differs on blocks recycled from the decoy"
