"""Case table of tests/test_streams_gpu.py: one small call per stream-taking entry point of include/parallel_ray_tracing.h,
more where a call has branches that launch differently.  Importing this module needs neither a GPU nor torch: a case is
built (numpy inputs, ctypes call) only when a test asks for it.

A case names its device buffers and says how to call the library on them:
  inputs    name -> numpy array: the REAL contents.  The held-back run starts from poison and copies these in late, on the
            side stream.  Every input is compared after the call as well (an in/out buffer must change the same way).
  poison    name -> fill value for an input other than 0.  Poison is always a value the call's contract accepts, so that a
            launch on the wrong stream computes wrong bytes and never a wild address: images, fields, weights and counts 0,
            pairs and peaks -1 (no pair; section 8b's status 8).
  outputs   name -> (shape, dtype): filled with SENTINEL before the call; what the call leaves alone still holds it.
  scratch   name -> bytes: caller scratch, zero-filled (detect_write_kernel and match_fill_kernel index with what they read
            from it), contents unspecified afterwards and not compared.
  call      f(photon, b, stream) with b: name -> ctypes.c_void_p; returns the host results to compare (or None).
"""
import ctypes
import functools

import numpy as np

from photon_amd import dot_tracking as dt
from photon_amd import piv_correlation as pc
from photon_amd import piv_weighting as pw

SENTINEL = -77

# stream-taking entry points that already run on a side stream elsewhere in the suite
COVERED_ELSEWHERE = {
    "photon_trace": "tests/test_segments_gpu.py, tests/test_pool_gpu.py",
    "photon_trace_moments": "tests/test_segments_gpu.py",
    "photon_scene_check": "tests/test_segments_gpu.py",
    "photon_tomo_deflect": "tests/test_tomo_deflection_gpu.py",
    "photon_tomo_deflect_adjoint": "tests/test_tomo_deflection_gpu.py",
    "photon_tomo_reconstruct_deflections": "tests/test_tomo_deflection_gpu.py",
    "photon_piv_background": "tests/test_piv_preprocess_gpu.py",
    "photon_piv_preprocess": "tests/test_piv_preprocess_gpu.py",
}

# cases that test_streams_gpu.py runs by a procedure of their own (they need a scene)
SPECIAL = {"stats_window": ("photon_scene_stats_begin", "photon_scene_stats_end")}

SMALL, ODD = (64, 80), (97, 130)                  # image shapes (height, width): a multiple of every tile, and of none


class Case:
    def __init__(self, inputs, outputs, call, scratch=None, poison=None):
        self.inputs, self.outputs, self.call = inputs, outputs, call
        self.scratch, self.poison = scratch or {}, poison or {}


class Spec:
    """name, the entry points the case runs, whether the call waits for its stream before it returns, the builder."""
    def __init__(self, name, entries, waits, build):
        self.name, self.entries, self.waits, self.build = name, entries, waits, build


CASES = {}


def case(name, *entries, waits=False):
    def register(build):
        assert name not in CASES
        CASES[name] = Spec(name, entries, waits, build)
        return build
    return register


def covered_entry_points():
    """entry point -> where it runs on a side stream: this module's cases, or the file that covers it already."""
    out = {e: f"tests/test_streams_gpu.py::{s.name}" for s in CASES.values() for e in s.entries}
    out.update({e: f"tests/test_streams_gpu.py::{name}" for name, entries in SPECIAL.items() for e in entries})
    for e, where in COVERED_ELSEWHERE.items():
        assert e not in out, f"{e} has a case here and is listed as covered elsewhere"
        out[e] = where
    return out


def declared_stream_entry_points(header_text: str):
    """Every photon_* declaration of the header with a `void *stream` parameter, in the header's order."""
    import re
    code = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(photon_\w+)\s*\(([^;]*?)\)\s*;", code) if re.search(r"void\s*\*\s*stream\b", m.group(2))]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(shape, seed=1, shift=(1.6, -1.1), per_px=0.03):
    """A particle image pair f32 [h, w] (frame 2 = frame 1 moved by `shift`), read-only."""
    rng = np.random.default_rng(seed)
    h, w = shape
    n = int(per_px * (h + 16) * (w + 16))
    x, y, amp = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n), rng.uniform(0.5, 1.0, n)
    out = []
    for dx, dy in ((0.0, 0.0), shift):
        im = (pc.particle_image(shape, x + dx, y + dy, 2.5, amp) + 0.02 * rng.random(shape)).astype(np.float32)
        im.setflags(write=False)
        out.append(im)
    return tuple(out)


def grid_field(shape, win, step, seed, cols=2):
    """A vector grid f32 [n_rows, n_cols, cols] around (1.6, -1.1)."""
    rng = np.random.default_rng(seed)
    r, c = pc.grid_shape(shape, win, step)
    f = rng.normal(0.0, 0.3, (r, c, cols)).astype(np.float32)
    f[..., 0] += 1.6
    f[..., 1] -= 1.1
    return f


def dense_field(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.8, (*shape, 2)).astype(np.float32)


def _f(v):
    return float(v)


# ---- section 5, 13, 14, 17, 18: the correlators --------------------------------------------------------------------------------
def _correlator_buffers(shape, win, step, R, offsets, planes, seed=1):
    im1, im2 = pair(shape, seed)
    r, c = pc.grid_shape(shape, win, step)
    inputs = dict(im1=im1, im2=im2)
    if offsets:
        inputs["offset"] = np.random.default_rng(seed + 7).integers(-2, 3, (r * c, 2)).astype(np.int32)
    outputs = dict(vectors=((r, c, 4), "float32"), flags=((r, c), "int32"))
    if planes:
        outputs["planes"] = ((r, c, 2 * R + 1, 2 * R + 1), "float32")
    return inputs, outputs, (r, c)


def _direct(shape, win, step, R, offsets=False, planes=False):
    inputs, outputs, _ = _correlator_buffers(shape, win, step, R, offsets, planes)
    h, w = shape

    def call(photon, b, stream):
        photon._call("photon_piv_correlate", b["im1"], b["im2"], w, h, win, step, R, b.get("offset"), b["vectors"], b["flags"],
                     b.get("planes"), None, None, stream)
    return Case(inputs, outputs, call)


@case("correlate_win16", "photon_piv_correlate")
def _(photon):
    return _direct(SMALL, 16, 8, 4)


@case("correlate_win32_offsets_planes", "photon_piv_correlate")
def _(photon):
    return _direct(ODD, 32, 16, 8, offsets=True, planes=True)


@case("correlate_win64", "photon_piv_correlate")
def _(photon):
    return _direct(ODD, 64, 16, 8, planes=True)


def _weighted(shape, win, step, R, offsets=False, planes=False):
    inputs, outputs, _ = _correlator_buffers(shape, win, step, R, offsets, planes)
    inputs["weight"] = pw.window_weights(win).astype(np.float32)        # poison 0: the sum of the weights is 0, a flat window
    h, w = shape

    def call(photon, b, stream):
        photon._call("photon_piv_correlate_weighted", b["im1"], b["im2"], b["weight"], w, h, win, step, R, b.get("offset"), b["vectors"],
                     b["flags"], b.get("planes"), None, None, stream)
    return Case(inputs, outputs, call)


@case("weighted_win16", "photon_piv_correlate_weighted")
def _(photon):
    return _weighted(SMALL, 16, 8, 4, planes=True)


@case("weighted_win32_offsets", "photon_piv_correlate_weighted")
def _(photon):
    return _weighted(ODD, 32, 16, 8, offsets=True)


@case("weighted_win64", "photon_piv_correlate_weighted")
def _(photon):
    return _weighted(ODD, 64, 16, 8)


def _masked(shape, win, step, R, offsets=False, planes=False):
    inputs, outputs, (r, c) = _correlator_buffers(shape, win, step, R, offsets, planes)
    h, w = shape
    m1, m2 = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)      # poison 0: nothing excluded
    m1[h // 3:h // 3 + 20, w // 4:w // 4 + 25] = 1                      # a body that masks some windows out and others in part
    m2[h // 3 + 2:h // 3 + 22, w // 4 + 1:w // 4 + 26] = 255
    inputs.update(mask1=m1, mask2=m2)
    outputs["valid"] = ((r, c, 2), "int32")

    def call(photon, b, stream):
        photon._call("photon_piv_correlate_masked", b["im1"], b["im2"], b["mask1"], b["mask2"], w, h, win, step, R, win * win // 2,
                     b.get("offset"), b["vectors"], b["flags"], b["valid"], b.get("planes"), None, None, stream)
    return Case(inputs, outputs, call)


@case("masked_win16", "photon_piv_correlate_masked")
def _(photon):
    return _masked(SMALL, 16, 8, 4, planes=True)


@case("masked_win32_offsets", "photon_piv_correlate_masked")
def _(photon):
    return _masked(ODD, 32, 16, 8, offsets=True)


@case("masked_win64", "photon_piv_correlate_masked")
def _(photon):
    return _masked(ODD, 64, 16, 8)


def _phase(shape, win, step, R, mode, offsets=False, planes=False):
    inputs, outputs, _ = _correlator_buffers(shape, win, step, R, offsets, planes)
    h, w = shape

    def call(photon, b, stream):
        photon._call("photon_piv_correlate_phase", b["im1"], b["im2"], w, h, win, step, R, b.get("offset"), mode, win / 4.0, 2.5,
                     b["vectors"], b["flags"], b.get("planes"), None, None, stream)
    return Case(inputs, outputs, call)


@case("phase_circular_win16", "photon_piv_correlate_phase")
def _(photon):
    return _phase(SMALL, 16, 8, 4, mode=0, planes=True)


@case("phase_win32_offsets", "photon_piv_correlate_phase")
def _(photon):
    return _phase(ODD, 32, 16, 8, mode=1, offsets=True, planes=True)


@case("phase_win64", "photon_piv_correlate_phase")
def _(photon):
    return _phase(ODD, 64, 16, 8, mode=1)


def _ensemble(shape, win, step, R, offsets=False, planes=False, n_pairs=3):
    inputs, outputs, (r, c) = _correlator_buffers(shape, win, step, R, offsets, planes)
    frames = [pair(shape, seed=10 + k) for k in range(n_pairs)]
    inputs["im1"], inputs["im2"] = (np.stack([f[k] for f in frames]) for k in (0, 1))
    outputs["count"] = ((r, c), "int32")
    h, w = shape

    def call(photon, b, stream):
        photon._call("photon_piv_correlate_ensemble", b["im1"], b["im2"], h * w, n_pairs, w, h, win, step, R, b.get("offset"), b["vectors"],
                     b["flags"], b["count"], b.get("planes"), None, None, stream)
    return Case(inputs, outputs, call)


@case("ensemble_win16", "photon_piv_correlate_ensemble")
def _(photon):
    return _ensemble(SMALL, 16, 8, 4, planes=True)


@case("ensemble_win32_offsets", "photon_piv_correlate_ensemble")
def _(photon):
    return _ensemble(ODD, 32, 16, 8, offsets=True)


@case("ensemble_win64", "photon_piv_correlate_ensemble")
def _(photon):
    return _ensemble(ODD, 64, 16, 8)


def _uncertainty(shape, win, step, reach):
    im1, im2 = pair(shape, seed=3, shift=(0.05, -0.03))                 # a matched pair: what is left between the frames is noise
    r, c = pc.grid_shape(shape, win, step)
    h, w = shape

    def call(photon, b, stream):
        photon._call("photon_piv_uncertainty", b["im1"], b["im2"], w, h, win, step, reach, b["sigma"], b["flags"], b["stats"], None, None,
                     stream)
    return Case(dict(im1=im1, im2=im2), dict(sigma=((r, c, 2), "float32"), flags=((r, c), "int32"), stats=((r, c, 2, 4), "float64")), call)


@case("uncertainty_win16", "photon_piv_uncertainty")
def _(photon):
    return _uncertainty(SMALL, 16, 8, 2)


@case("uncertainty_win32", "photon_piv_uncertainty")
def _(photon):
    return _uncertainty(ODD, 32, 16, 4)


@case("uncertainty_win64", "photon_piv_uncertainty")
def _(photon):
    return _uncertainty(ODD, 64, 16, 1)


@case("regrid", "photon_piv_regrid")
def _(photon):
    h, w = ODD
    src = grid_field(ODD, 32, 16, seed=5, cols=4)
    sr, sc = src.shape[:2]
    dr, dc = pc.grid_shape(ODD, 16, 8)

    def call(photon, b, stream):
        photon._call("photon_piv_regrid", b["src"], 4, sr, sc, 32, 16, w, h, 16, 8, b["dst"], None, None, stream)
    return Case(dict(src=src), dict(dst=((dr, dc, 2), "float32")), call)


# ---- section 7: image deformation ----------------------------------------------------------------------------------------------
@case("bspline_coefficients", "photon_piv_bspline_coefficients")
def _(photon):
    h, w = ODD

    def call(photon, b, stream):
        photon._call("photon_piv_bspline_coefficients", b["im"], w, h, b["coef"], stream)
    return Case(dict(im=pair(ODD)[0]), dict(coef=(ODD, "float32")), call)


@case("deform", "photon_piv_deform")
def _(photon):
    h, w = ODD
    field = grid_field(ODD, 32, 16, seed=6)
    r, c = field.shape[:2]

    def call(photon, b, stream):
        photon._call("photon_piv_deform", b["coef"], w, h, b["field"], 2, r, c, 32, 16, -0.5, b["out"], stream)
    return Case(dict(coef=pair(ODD)[0], field=field), dict(out=(ODD, "float32")), call)


def _validate(with_pred):
    r, c = 9, 13
    rng = np.random.default_rng(8)
    vectors = grid_field((r * 8 + 8, c * 8 + 8), 16, 8, seed=9, cols=4)[:r, :c].copy()
    vectors[4, 6, :2] = (9.0, -7.0)                                     # an outlier
    vectors[2, 3] = np.nan
    flags = np.zeros((r, c), np.int32)
    flags[2, 3] = 2                                                     # a flat window
    inputs = dict(vectors=vectors, flags=flags)
    if with_pred:
        inputs["pred"] = rng.normal(0.0, 0.5, (r, c, 2)).astype(np.float32)

    def call(photon, b, stream):
        photon._call("photon_piv_validate", b.get("pred"), b["vectors"], b["flags"], r, c, 0.1, 2.0, b["field"], b["smooth"], b["status"], stream)
    return Case(inputs, dict(field=((r, c, 2), "float32"), smooth=((r, c, 2), "float32"), status=((r, c), "int32")), call)


@case("validate", "photon_piv_validate")
def _(photon):
    return _validate(False)


@case("validate_with_predictor", "photon_piv_validate")
def _(photon):
    return _validate(True)


# ---- section 12: dense optical flow --------------------------------------------------------------------------------------------
@case("field_to_pixels", "photon_piv_field_to_pixels")
def _(photon):
    h, w = ODD
    field = grid_field(ODD, 32, 16, seed=11)
    r, c = field.shape[:2]

    def call(photon, b, stream):
        photon._call("photon_piv_field_to_pixels", b["field"], 2, r, c, 32, 16, w, h, b["dense"], stream)
    return Case(dict(field=field), dict(dense=((h, w, 2), "float32")), call)


@case("deform_dense", "photon_piv_deform_dense")
def _(photon):
    h, w = ODD

    def call(photon, b, stream):
        photon._call("photon_piv_deform_dense", b["coef"], w, h, b["dense"], 0.5, b["out"], stream)
    return Case(dict(coef=pair(ODD)[1], dense=dense_field(ODD, 12)), dict(out=(ODD, "float32")), call)


def optflow_terms_case(shape=ODD):
    """photon_optflow_terms with a field: the single-launch call the harness's self-check hands the wrong stream."""
    h, w = shape
    w1, w2 = pair(shape, seed=4, shift=(0.3, -0.2))

    def call(photon, b, stream):
        photon._call("photon_optflow_terms", b["w1"], b["w2"], w, h, b["u0"], 1.3, 5.0, b["terms"], stream)
    return Case(dict(w1=w1, w2=w2, u0=dense_field(shape, 13)), dict(terms=((h, w, 4), "float32")), call)


@case("optflow_terms", "photon_optflow_terms")
def _(photon):
    return optflow_terms_case()


def _iterate(photon, sweeps_of_T):
    """sweeps_of_T(T) sweeps: 0 is the copy, T one launch without d_tmp, 2T + 1 three launches -- d_tmp, d_out, d_tmp... so that
    both parities of the alternation are written and read."""
    h, w = ODD
    T = photon.optflow_iterations_per_launch()
    n = sweeps_of_T(T)
    rng = np.random.default_rng(14)
    ix, iy, c = (rng.normal(0.0, 1.0, ODD) for _ in range(3))
    terms = np.stack([ix, iy, c, 1.0 / (5.0 + ix * ix + iy * iy)], axis=-1).astype(np.float32)
    scratch = dict(tmp=h * w * 2 * 4) if n > T else {}

    def call(photon, b, stream):
        photon._call("photon_optflow_iterate", b["terms"], b["u"], w, h, n, b["out"], b.get("tmp"), stream)
    return Case(dict(terms=terms, u=dense_field(ODD, 15)), dict(out=((h, w, 2), "float32")), call, scratch=scratch)


@case("optflow_iterate_copy", "photon_optflow_iterate")
def _(photon):
    return _iterate(photon, lambda T: 0)


@case("optflow_iterate_one_launch", "photon_optflow_iterate")
def _(photon):
    return _iterate(photon, lambda T: T)


@case("optflow_iterate_three_launches", "photon_optflow_iterate")
def _(photon):
    return _iterate(photon, lambda T: 2 * T + 1)


# ---- section 8: dot tracking ---------------------------------------------------------------------------------------------------
MAX_DOTS = 256


@functools.lru_cache(maxsize=None)
def dots_pair():
    """Two frames of well separated dots on ODD, frame 2 moved by about (1.3, -0.7): (im1, im2)."""
    rng = np.random.default_rng(21)
    h, w = ODD
    pts = []
    while len(pts) < 60:
        p = rng.uniform((6, 6), (w - 6, h - 6))
        if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= 64.0 for q in pts):
            pts.append(p)
    p = np.array(pts)
    amp = rng.uniform(0.5, 1.0, len(pts))
    ims = []
    for dx, dy in ((0.0, 0.0), (1.3, -0.7)):
        ims.append((pc.particle_image(ODD, p[:, 0] + dx, p[:, 1] + dy, 4.0, amp) + 0.005 * rng.random(ODD)).astype(np.float32))
    return tuple(ims)


@functools.lru_cache(maxsize=None)
def dots_chain():
    """The host models' results down the chain, as the inputs of the later calls: peaks / counts / dots / status per frame
    (padded to MAX_DOTS), the predictor field, pair and shift."""
    out = {}
    for k, im in enumerate(dots_pair()):
        peaks, total = dt.detect_model(im, 0.25, dt.image_max_model(im), MAX_DOTS)
        dots, status = dt.fit_model(im, peaks)
        n = peaks.size
        assert 30 <= n == total < MAX_DOTS
        pad_peaks = np.full(MAX_DOTS, -1, np.int32)
        pad_peaks[:n] = peaks
        pad_dots, pad_status = np.zeros((MAX_DOTS, 4), np.float32), np.zeros(MAX_DOTS, np.int32)
        pad_dots[:n], pad_status[:n] = dots, status
        out[k] = dict(peaks=pad_peaks, count=np.array([n], np.int32), dots=pad_dots, status=pad_status, n=n)
    field = grid_field(ODD, 32, 16, seed=22)
    field[..., 0] += 1.3 - 1.6
    field[..., 1] += -0.7 + 1.1
    field *= np.float32(0.9)                                             # a predictor, not the answer
    pair_, shift, npaired = dt.match_model(out[0]["dots"][:out[0]["n"]], out[0]["status"][:out[0]["n"]], out[1]["dots"][:out[1]["n"]],
                                           out[1]["status"][:out[1]["n"]], 3.0, (field, 32, 16))
    assert npaired >= 20
    pad_pair, pad_shift = np.full(MAX_DOTS, -1, np.int32), np.zeros((MAX_DOTS, 4), np.float32)
    pad_pair[:pair_.size], pad_shift[:pair_.size] = pair_, shift
    out.update(field=field, pair=pad_pair, shift=pad_shift)
    return out


@case("dots_image_max", "photon_dots_image_max")
def _(photon):
    h, w = ODD

    def call(photon, b, stream):
        photon._call("photon_dots_image_max", b["im"], w, h, b["top"], stream)
    return Case(dict(im=dots_pair()[0]), dict(top=((1,), "float32")), call)


@case("dots_detect_scaled", "photon_dots_image_max", "photon_dots_detect")
def _(photon):
    """The threshold is a fraction of the maximum that photon_dots_image_max leaves on the device, on the same stream."""
    h, w = ODD
    nbytes = photon.dots_scratch_bytes(w, h)

    def call(photon, b, stream):
        photon._call("photon_dots_image_max", b["im"], w, h, b["top"], stream)
        photon._call("photon_dots_detect", b["im"], w, h, 0.25, b["top"], MAX_DOTS, b["peaks"], b["count"], b["scratch"], nbytes, stream)
    return Case(dict(im=dots_pair()[0]), dict(top=((1,), "float32"), peaks=((MAX_DOTS,), "int32"), count=((1,), "int32")), call,
                scratch=dict(scratch=nbytes))


@case("dots_fit", "photon_dots_fit")
def _(photon):
    h, w = ODD
    f = dots_chain()[0]

    def call(photon, b, stream):
        photon._call("photon_dots_fit", b["im"], w, h, b["peaks"], b["count"], MAX_DOTS, 3, 1.0, 4, 0.0, b["dots"], b["status"], stream)
    return Case(dict(im=dots_pair()[0], peaks=f["peaks"], count=f["count"]), dict(dots=((MAX_DOTS, 4), "float32"), status=((MAX_DOTS,), "int32")),
                call, poison=dict(peaks=-1))


@case("dots_match_with_predictor", "photon_dots_match")
def _(photon):
    h, w = ODD
    ch = dots_chain()
    field = ch["field"]
    r, c = field.shape[:2]
    nbytes = photon.dots_scratch_bytes(w, h, 3.0, MAX_DOTS, MAX_DOTS)
    inputs = dict(dots1=ch[0]["dots"], status1=ch[0]["status"], count1=ch[0]["count"], dots2=ch[1]["dots"], status2=ch[1]["status"],
                  count2=ch[1]["count"], field=field)

    def call(photon, b, stream):
        photon._call("photon_dots_match", b["dots1"], b["status1"], b["count1"], MAX_DOTS, b["dots2"], b["status2"], b["count2"], MAX_DOTS, 0,
                     b["field"], 2, r, c, 32, 16, 3.0, w, h, b["pair"], b["shift"], b["npaired"], b["scratch"], nbytes, stream)
    return Case(inputs, dict(pair=((MAX_DOTS,), "int32"), shift=((MAX_DOTS, 4), "float32"), npaired=((1,), "int32")), call,
                scratch=dict(scratch=nbytes))


@case("dots_window_means", "photon_dots_window_means")
def _(photon):
    h, w = ODD
    ch = dots_chain()
    r, c = pc.grid_shape(ODD, 32, 16)

    def call(photon, b, stream):
        photon._call("photon_dots_window_means", b["dots1"], b["pair"], b["shift"], b["count1"], MAX_DOTS, w, h, 32, 16, 2, 1, b["vectors"],
                     b["flags"], stream)
    return Case(dict(dots1=ch[0]["dots"], pair=ch["pair"], shift=ch["shift"], count1=ch[0]["count"]),
                dict(vectors=((r, c, 4), "float32"), flags=((r, c), "int32")), call, poison=dict(pair=-1))


# ---- section 9: tomography; section 6: gradient integration --------------------------------------------------------------------
TOMO_N = 12
TOMO_GRID = ((TOMO_N,) * 3, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
SOLVER_ITERATIONS = 16


def tomo_axis_rays():
    """Rays along +x through every (j, k) node and along +y through every (i, k) node of the grid: 288.  On this grid of unit
    spacing every plane such a ray crosses has ONE tap of weight 1 and three of weight 0, and every voxel is a weight-1 tap
    of two rays.  photon_tomo_backproject and photon_tomo_reconstruct add a voxel's terms with f64 atomics in an order that
    is not fixed and promise no repeatable bits in general; with at most two terms that are not 0 per voxel the sum does not
    depend on the order (a + b = b + a, and adding 0 is exact), so these rays give the same bytes on every run and the
    byte comparison of the held-back run is sound for these two calls as well."""
    n = TOMO_N
    a, b = (v.ravel().astype(np.float64) for v in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    origins = np.concatenate([np.stack([np.full(n * n, -5.0), a, b], axis=1), np.stack([a, np.full(n * n, -5.0), b], axis=1)])
    dirs = np.concatenate([np.tile([1.0, 0.0, 0.0], (n * n, 1)), np.tile([0.0, 1.0, 0.0], (n * n, 1))])
    return np.ascontiguousarray(origins), np.ascontiguousarray(dirs)


def _grid_args():
    dims, spacing, origin = TOMO_GRID
    sp, og = np.array(spacing, np.float64), np.array(origin, np.float64)       # host arrays of three, alive with the closure
    return dims, sp, og


@case("tomo_project", "photon_tomo_project")
def _(photon):
    dims, sp, og = _grid_args()
    rng = np.random.default_rng(31)
    o_axis, d_axis = tomo_axis_rays()
    n_more = 112                                                        # oblique rays through the grid: four taps per plane
    o = np.concatenate([o_axis, rng.uniform(-3.0, 14.0, (n_more, 3))])
    d = np.concatenate([d_axis, rng.normal(0.0, 1.0, (n_more, 3))])
    n_rays = o.shape[0]

    def call(photon, b, stream):
        photon._call("photon_tomo_project", b["f"], *dims, sp.ctypes.data_as(ctypes.c_void_p), og.ctypes.data_as(ctypes.c_void_p), b["origins"],
                     b["dirs"], n_rays, b["p"], stream)
    return Case(dict(f=rng.normal(0.0, 1.0, dims[::-1]), origins=o, dirs=d), dict(p=((n_rays,), "float64")), call)


@case("tomo_backproject", "photon_tomo_backproject")
def _(photon):
    """v += A^T y with whole numbers in y and in v: every sum is exact in any order (tomo_axis_rays)."""
    dims, sp, og = _grid_args()
    rng = np.random.default_rng(32)
    o, d = tomo_axis_rays()
    n_rays = o.shape[0]
    y = rng.integers(-8, 9, n_rays).astype(np.float64)
    v = rng.integers(-8, 9, dims[::-1]).astype(np.float64)

    def call(photon, b, stream):
        photon._call("photon_tomo_backproject", b["y"], *dims, sp.ctypes.data_as(ctypes.c_void_p), og.ctypes.data_as(ctypes.c_void_p),
                     b["origins"], b["dirs"], n_rays, b["v"], stream)
    return Case(dict(y=y, origins=o, dirs=d, v=v), {}, call)


@case("tomo_reconstruct", "photon_tomo_reconstruct", waits=True)
def _(photon):
    from photon_amd.library import photon_tomo_stats_t
    dims, sp, og = _grid_args()
    rng = np.random.default_rng(33)
    o, d = tomo_axis_rays()
    n_rays = o.shape[0]
    k, j, i = np.meshgrid(*(np.arange(TOMO_N),) * 3, indexing="ij")
    support = (((i - 5.5) ** 2 + (j - 5.5) ** 2 + (k - 5.5) ** 2) <= 30.0).astype(np.uint8)
    w = rng.uniform(0.5, 2.0, n_rays)
    w[::17] = 0.0                                                       # rays that take no part

    def call(photon, b, stream):
        st = photon_tomo_stats_t()
        photon._call("photon_tomo_reconstruct", b["p"], b["w"], b["support"], *dims, sp.ctypes.data_as(ctypes.c_void_p),
                     og.ctypes.data_as(ctypes.c_void_p), b["origins"], b["dirs"], n_rays, 0.5, 0.0, SOLVER_ITERATIONS, b["f"], ctypes.byref(st),
                     stream)
        return st.as_dict()
    return Case(dict(p=rng.normal(0.0, 3.0, n_rays), w=w, support=support, origins=o, dirs=d), dict(f=(dims[::-1], "float64")), call)


@case("integrate_gradient", "photon_integrate_gradient", waits=True)
def _(photon):
    from photon_amd.library import photon_integrate_stats_t
    ny, nx = 33, 47
    rng = np.random.default_rng(34)
    w = rng.uniform(0.2, 1.0, (ny, nx))
    w[10:13, 20:24] = 0.0                                               # a hole

    def call(photon, b, stream):
        st = photon_integrate_stats_t()
        photon._call("photon_integrate_gradient", b["gx"], b["gy"], b["w"], None, None, nx, ny, 1.0, 1.5, 0.0, SOLVER_ITERATIONS, b["phi"],
                     ctypes.byref(st), stream)
        return st.as_dict()
    return Case(dict(gx=rng.normal(0.0, 1.0, (ny, nx)), gy=rng.normal(0.0, 1.0, (ny, nx)), w=w), dict(phi=((ny, nx), "float64")), call)


# ---- section 4: sensor post-processing -----------------------------------------------------------------------------------------
def _postprocess(noise):
    h, w = SMALL
    image = (pair(SMALL)[0] * np.float32(900.0)).astype(np.float32)     # in/out with noise: compared after the call like every input

    def call(photon, b, stream):
        rows, cols = ctypes.c_int(0), ctypes.c_int(0)
        photon._call("photon_postprocess_u16", b["image"], w, h, 3.0, 12, 1, noise, 99, 0, 0, b["out"], ctypes.byref(rows), ctypes.byref(cols),
                     stream)
        return rows.value, cols.value
    return Case(dict(image=image), dict(out=(SMALL, "int16")), call)    # the uint16 picture, its sentinel the bytes of int16 -77


@case("postprocess_u16", "photon_postprocess_u16", waits=True)
def _(photon):
    return _postprocess(0.0)


@case("postprocess_u16_noise", "photon_postprocess_u16", waits=True)
def _(photon):
    return _postprocess(0.05)
