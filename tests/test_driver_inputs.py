"""The drivers' ingest rule (PhotonLibrary's docstring) without a GPU: the variants of driver_input_cases.py are what they
are named for, library._on_device on device="cpu" turns each into the bytes of np.ascontiguousarray(a, target) under
warnings-as-errors and writes nothing, the refusals name their argument, photon_amd/*.py makes tensors of callers' arrays
nowhere else, and every array argument of every public driver has a row in the GPU module's table.

Before the helper (torch.as_tensor(x).to(dtype).contiguous()) these variants failed (the table in DESIGN 4.3u):
negative strides and a foreign byte order with torch's ValueError, read-only arrays and memmaps with its "not writable"
UserWarning; a nested list of f64 gradients lost its low bits without a word."""
import glob
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import driver_input_cases as cases

torch = pytest.importorskip("torch")
from photon_amd import library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sources():
    """name -> (the C-contiguous array, the torch dtype a driver wants of it, nonzero)."""
    rng = np.random.default_rng(7)
    counts = np.rint(20 + 200 * rng.random((3, 10, 14))).astype(np.float32)             # whole numbers: the integer dtypes join
    mask = (rng.random((9, 13)) < 0.3).astype(np.uint8)
    return {
        "image_f32": (rng.random((9, 13)).astype(np.float32), torch.float32, False),
        "field_f32": (rng.normal(size=(4, 5, 2)).astype(np.float32), torch.float32, False),
        "counts_stack_f32": (counts, torch.float32, False),
        "gradient_f64": (rng.normal(size=(7, 11)), torch.float64, False),
        "ray_values_f64": (rng.normal(size=23), torch.float64, False),
        "mask_u8": (mask, torch.uint8, True),
    }


SOURCES = sources()
NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8}


@pytest.mark.parametrize("source", list(SOURCES))
def test_each_variant_holds_the_values_and_is_what_it_is_named_for(source, tmp_path):
    a = SOURCES[source][0]
    seen = []
    for name, v in cases.variants(a, tmp_path):
        cases.check_variant(name, v, a)
        seen.append(name)
    assert len(seen) == len(set(seen)) and set(seen) <= set(cases.ALL_VARIANTS)
    assert {"every_second_column", "flipud", "fliplr", "byte_order", "read_only", "memmap", "nested_list", "torch_cpu",
            "torch_cpu_view"} <= set(seen)
    if a.ndim >= 2:
        assert {"fortran", "crop", "rot90"} <= set(seen)
    if source == "counts_stack_f32":
        assert {"uint8", "uint16", "int32"} <= set(seen)
    for name, v in cases.variants(a, tmp_path, tensors=False):
        if name in cases.NEGATIVE_STRIDE:
            assert any(s < 0 for s in v.strides), name


def state_of(v):
    if isinstance(v, np.ndarray):
        return v.tobytes(), v.flags.writeable, v.strides, v.dtype
    if isinstance(v, torch.Tensor):
        return v.clone().numpy().tobytes(), v.stride(), v.dtype
    return repr(v)


@pytest.mark.parametrize("source", list(SOURCES))
def test_the_helper_on_the_cpu_gives_numpys_bytes_and_writes_nothing(source, tmp_path):
    a, dtype, nonzero = SOURCES[source]
    want = np.ascontiguousarray((a != 0) if nonzero else a, NP_OF[dtype]).tobytes()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for name, v in [("c_contiguous", a.copy()), *cases.variants(a, tmp_path)]:
            before = state_of(v)
            t = library._on_device(v, dtype, "cpu", "im1", a.ndim, nonzero=nonzero)
            assert isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu", name
            assert t.numpy().tobytes() == want, f"{source}, {name}: not the bytes of np.ascontiguousarray(a, target)"
            assert state_of(v) == before, f"{source}, {name}: the caller's object changed"
        if nonzero:
            for name, m in cases.mask_forms(a):
                assert library._on_device(m, dtype, "cpu", "mask", 2, nonzero=True).numpy().tobytes() == want, name


def test_a_conforming_tensor_comes_back_as_the_same_storage():
    for dtype in (torch.float32, torch.float64):
        t = torch.arange(12, dtype=dtype).reshape(3, 4)
        out = library._on_device(t, dtype, "cpu", "im1", 2)
        assert out.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() and out.data_ptr() == t.data_ptr()
        for other in (t.t(), t[:, ::2], t.to(torch.float64 if dtype == torch.float32 else torch.float32), t.to(torch.int32)):
            out = library._on_device(other, dtype, "cpu", "im1", 2)
            assert out.untyped_storage().data_ptr() != other.untyped_storage().data_ptr()
            assert out.is_contiguous() and out.dtype == dtype and torch.equal(out, other.to(dtype))
    assert library._on_device(None, torch.float32, "cpu", "w") is None and library._checked(None, "w") is None


def test_what_the_rule_refuses_names_the_argument():
    a = SOURCES["image_f32"][0]
    for name, bad, error in cases.refused(a):
        with pytest.raises(error, match="im2"):
            library._on_device(bad, torch.float32, "cpu", "im2", 2)
        with pytest.raises(error, match="im2"):
            library._checked(bad, "im2")
    with pytest.raises(TypeError, match="predictor"):
        library._checked(torch.zeros((2, 2, 2), dtype=torch.complex64), "predictor", 3)
    with pytest.raises(TypeError, match="im1"):
        library._checked(np.array([["a", "b"]]), "im1", 2)
    for bad in (a[0], a[None], a.tolist()[0], torch.from_numpy(a.copy())[None]):
        with pytest.raises(ValueError, match="im1 must have 2 dimensions"):
            library._on_device(bad, torch.float32, "cpu", "im1", 2)
    with pytest.raises(ValueError, match="frames1"):
        library._checked([[1.0, 2.0], [3.0]], "frames1", 3)                          # ragged: numpy makes no array of it
    with pytest.raises(ValueError, match=r"one shape, not \(9, 13\) and \(8, 13\)"):
        library._checked_pair(a, a[:-1])
    with pytest.raises(ValueError, match="a mask of shape .* does not cover"):
        library._checked_pair(a, a, mask=np.zeros((9, 12), bool))
    with pytest.raises(ValueError, match="does not cover"):
        library._checked_pair(a, a, mask=(np.zeros((9, 13), bool), np.zeros((8, 13), np.uint8)))
    with pytest.raises(TypeError, match="mask"):
        library._checked_pair(a, a, mask=np.zeros((9, 13), complex))
    with pytest.raises(TypeError, match="weighting"):
        library._checked_weighting(np.zeros((32, 32), complex))
    assert library._checked_weighting("gaussian") == "gaussian" and library._checked_weighting(("gaussian", 7.0)) == ("gaussian", 7.0)


def test_numpys_conversion_round_to_nearest():
    """The device tensor holds np.asarray(x).astype(target): f64 -> f32 to the nearest even, large integers likewise."""
    x = np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -40, 65535.0, 16777217.0])
    for v in (x, x.tolist(), torch.from_numpy(x.copy()), x.astype(x.dtype.newbyteorder(cases.SWAPPED))):
        assert library._on_device(v, torch.float32, "cpu").numpy().tobytes() == x.astype(np.float32).tobytes()
    big = np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 40 + 2 ** 16 + 1], np.uint64)
    assert library._on_device(big, torch.float32, "cpu").numpy().tobytes() == big.astype(np.float32).tobytes()
    bf = torch.tensor([[1.0, 0.3], [-2.5, 65280.0]], dtype=torch.bfloat16)         # numpy has no bfloat16: through f32, exactly
    assert torch.equal(library._on_device(bf, torch.float32, "cpu", "im1", 2), bf.to(torch.float32))
    u16 = np.array([0, 1, 61000, 65535], np.uint16)
    assert library._on_device(u16, torch.float32, "cpu").tolist() == [0.0, 1.0, 61000.0, 65535.0]


# ---- the lint: one place makes tensors of callers' arrays -----------------------------------------------------------------------
# The lint is textual: it reads the lines of photon_amd/*.py, so a listed statement that is reformatted has to be listed again,
# and a spelling it does not know (an alias of torch) passes it; it guards against the ordinary slip, not against intent.
# internal uses of torch.from_numpy / torch.as_tensor that remain: (file, what the line holds) -> why it is no caller's array
INTERNAL_TENSORS = {
    ("library.py", "return torch.from_numpy(c).to(device=dev)"): "the helper itself: c is its own native, C-contiguous, writable copy",
    ("library.py", "d_off = torch.from_numpy(offsets).to(dev)"): "pass 2's integer window offsets, an int32 table piv_correlation.predictor just made",
}


def test_tensors_of_callers_arrays_are_made_in_the_helper_alone():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "photon_amd", "*.py"))):
        for no, line in enumerate(open(path, encoding="utf-8"), 1):
            code = line.split("#", 1)[0]
            if re.search(r"\b(as_tensor|from_numpy|from_dlpack|frombuffer|asarray)\s*\(", code) and "torch" in code \
                    or re.search(r"\btorch\.tensor\s*\(", code):
                found.setdefault((os.path.basename(path), code.strip()), []).append(no)
    unlisted = {k: v for k, v in found.items() if k not in INTERNAL_TENSORS}
    assert not unlisted, f"tensors made outside library._on_device (lines by statement): {unlisted}"
    assert not [k for k in INTERNAL_TENSORS if k not in found], "INTERNAL_TENSORS lists statements that are gone"
    assert len(found[("library.py", "d_off = torch.from_numpy(offsets).to(dev)")]) == 1          # once, in the shared two-pass helper
    text = open(os.path.join(ROOT, "photon_amd", "library.py"), encoding="utf-8").read()
    assert "d_off = torch.from_numpy(offsets).to(dev)" in text[text.index("def _two_passes("):text.index("def _replace_masked(")]
    body = text[text.index("def _on_device("):text.index("def _device_and_stream(")]
    assert "torch.from_numpy(c)" in body                                                     # the listed statement is the helper's
    assert len(re.findall(r"\b_on_device\(", text)) >= 20                                   # the lint has something to guard


# ---- the inventory -------------------------------------------------------------------------------------------------------------
def test_every_array_argument_of_every_driver_has_a_row():
    """A public method of PhotonLibrary with an array parameter cannot ship without a line in cases.DRIVERS (or in
    HOST_ARRAY_METHODS, with the reason there), and every argument DRIVERS lists is one that a row of the GPU module runs the
    variants on."""
    cls = library.PhotonLibrary
    public = {name for name, _ in inspect.getmembers(cls, inspect.isfunction) if not name.startswith("_")}
    assert not [m for m in (*cases.DRIVERS, *cases.HOST_ARRAY_METHODS) if m not in public], "listed methods that do not exist"
    assert not set(cases.DRIVERS) & set(cases.HOST_ARRAY_METHODS)
    for method, params in cases.DRIVERS.items():
        have = inspect.signature(getattr(cls, method)).parameters
        assert not [p for p in params if p not in have], (method, list(have))
    # a method that takes one of the drivers' argument names is a driver, or is listed with the host-array methods
    for method, hit in cases.methods_with_array_parameters(cls).items():
        assert method in cases.DRIVERS or method in cases.HOST_ARRAY_METHODS, f"{method}{hit}: no row in driver_input_cases.DRIVERS"
        if method in cases.DRIVERS:
            assert sorted(hit) == sorted(cases.DRIVERS[method]), (method, hit)
    # a method whose docstring promises numpy arrays or torch tensors in is one of the two lists as well
    for name in public:
        doc = inspect.getdoc(getattr(cls, name)) or ""
        if re.search(r"numpy arrays or torch|torch tensors on the device or numpy|torch device tensors or\s+numpy", doc):
            assert name in cases.DRIVERS, f"{name} takes arrays by its docstring and has no row in driver_input_cases.DRIVERS"
    covered = cases.covered_arguments()
    missing = [(m, p) for m, params in cases.DRIVERS.items() for p in params if (m, p) not in covered]
    assert not missing, f"no row of driver_input_cases.rows() runs the variants on {missing}"
    assert not [mp for mp in covered if mp[1] not in cases.DRIVERS.get(mp[0], {})], "rows for arguments DRIVERS does not list"


def test_the_inventory_fails_without_a_row(monkeypatch):
    rows = dict(cases.rows())
    del rows["correlate_weighting"]
    monkeypatch.setattr(cases, "rows", lambda: rows)
    with pytest.raises(AssertionError, match="weighting"):
        test_every_array_argument_of_every_driver_has_a_row()


def test_the_rows_reuse_the_stream_pipelines():
    import test_streams_gpu as ts
    rows = cases.rows()
    assert len(ts.PIPELINES) == 14 and all(name in rows and rows[name].run is ts.PIPELINES[name][2] for name in ts.PIPELINES)
    for name in ("tomo_reconstruct_deflections", "correlate_mask", "correlate_weighting", "preprocess_series_background"):
        assert name in rows


# ---- camera counts: the f64 model keeps its own caps on them ---------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(cases.CAMERA_SETTINGS))
@pytest.mark.parametrize("index", range(3))
def test_the_direct_correlators_model_on_camera_counts_keeps_its_clear_windows(index, setting):
    """What assert_close_to_the_host_model leaves out stays rare on counts: more than half of the live windows keep a peak
    that stands clear of its runner-up by 1e-3, as test_piv_correlation_gpu asks of the unscaled images; and the model's
    vectors on the counts are those on the unscaled images to within the quantisation (printed; 8 bit moves them most)."""
    import test_piv_correlation_gpu as tg
    from photon_amd import piv_correlation as pc
    c1, c2, win, step, R, off, want = cases.direct_correlator_counts(index, setting)
    gain, pedestal, dtype = cases.CAMERA_SETTINGS[setting]
    assert c1.dtype == dtype and c1.min() >= pedestal and c1.max() > pedestal + 0.25 * gain
    assert (c1 == np.iinfo(dtype).max).mean() < 0.01                                 # saturation stays the exception
    live = (want[1] & pc.FLAG_FLAT) == 0
    planes = want[2][live].reshape(int(live.sum()), -1)
    srt = np.sort(planes, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-3 * srt[:, -1]
    assert clear.mean() > 0.5
    w, r, s, shape, shift, _ = cases.direct_correlator_cases()[index]
    im1, im2 = tg.particle_pair(shape, shift, seed=w * 100 + r + s)
    unscaled = pc.correlate_model(im1, im2, win, step, R, offset=off)
    assert np.array_equal(unscaled[1], want[1])                                       # the same flags: the pedestal makes no window flat
    moved = np.abs(unscaled[0][live][clear, :2] - want[0][live][clear, :2])
    print(f"win {win}, {setting}: {clear.mean():.3f} of the live windows clear; counts move the model's vectors by {np.median(moved):.2e} px "
          f"(median), {moved.max():.2e} px (max)")
    # rounding adds noise of 0.29 counts rms, 1.4e-3 of the 8-bit gain: a quarter of the 5.8e-3 rms the images carry already, so the
    # typical vector moves by a small part of its own random error (0.05 px for a good PIV vector)
    assert np.median(moved) <= 0.01


# ---- camera counts: every other model keeps its module's caps on the counts images -------------------------------------------------
SETTINGS = list(cases.CAMERA_SETTINGS)


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_ensemble_model_on_camera_counts_keeps_its_clear_windows(setting):
    from photon_amd import piv_correlation as pc
    import piv_ensemble_cases as ec
    want_v, want_f, want_c, want_p = cases.ensemble_counts(setting)[4]
    assert np.array_equal(want_f, cases.ensemble_counts(None)[4][1]) and (want_c == ec.PARTICLE_PAIRS).all()
    live = (want_f & pc.FLAG_FLAT) == 0
    srt = np.sort(want_p[live].reshape(int(live.sum()), -1), axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-3 * srt[:, -1]
    moved = np.abs(want_v[live][clear, :2] - cases.ensemble_counts(None)[4][0][live][clear, :2])
    print(f"ensemble, {setting}: {clear.mean():.3f} of the live windows clear; counts move the vectors by {np.median(moved):.2e} px (median)")
    assert clear.mean() > 0.5 and np.median(moved) <= 0.01


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_deformation_and_multigrid_models_on_camera_counts_stay_within_their_bar_of_the_unscaled_ones(setting):
    """|RMS - RMS of the model| <= 0.02 px is the bar the device is held to: rounding to counts moves the models' own RMS
    against the truth by less than that."""
    for name, model in (("correlate_deform", cases.deform_model), ("correlate_multigrid phase", cases.phase_multigrid_model)):
        rms, unscaled = cases.uniform_rms(model(setting)[0], cases.PAIR_SHIFT), cases.uniform_rms(model(None)[0], cases.PAIR_SHIFT)
        print(f"{name}, {setting}: model RMS on counts {rms:.4f} px, on the unscaled pair {unscaled:.4f} px")
        assert abs(rms - unscaled) <= 0.02 and np.isfinite(model(setting)[0][1:-1, 1:-1, :2]).all()


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_uncertainty_model_on_camera_counts_flags_what_it_flagged(setting):
    c1, c2, (sigma, flags, stats, T) = cases.uncertainty_counts(setting)
    _, _, (sigma0, flags0, _, _) = cases.uncertainty_counts(None)
    keep = (flags == 0) & (flags0 == 0)
    ratio = sigma[keep] / sigma0[keep]
    print(f"uncertainty, {setting}: {int((flags != flags0).sum())} of {flags.size} flags differ; sigma on counts / unscaled: median {np.median(ratio):.3f}")
    assert keep.mean() > 0.5 and (flags != flags0).mean() <= 0.05           # V < 0 (bit 32) sits on the noise: a few windows may cross
    assert 0.8 <= np.median(ratio) <= 1.25                                   # sigma is in pixels: it does not scale with the gain


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_flow_model_on_camera_counts_follows_the_unscaled_one(setting):
    _, _, grid, flow = cases.flow_counts(setting)
    _, _, grid0, flow0 = cases.flow_counts(None)
    moved = np.abs(flow - flow0)
    print(f"optical flow, {setting}: counts move the model's field by {np.median(moved):.2e} px (median), {moved.max():.2e} px (max)")
    assert np.isfinite(flow).all() and np.median(moved) <= 0.01


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_dots_model_on_camera_counts_finds_the_same_dots_within_its_edge_cap(setting):
    """With background -> gain background + pedestal and the relative threshold that cuts the same intensity, the model
    finds on the counts the dots it finds on the unscaled frame, and none of them sits on the 1 px line that compare_fit
    leaves out (MAX_EDGE_SHARE).  With the threshold left at 0.25 of a maximum that carries the pedestal it would admit the
    noise: 346 maxima against 17 at a pedestal of 61000."""
    import test_dot_tracking_gpu as td
    frame, thr, bg, peaks, want = cases.dots_counts(setting)
    _, _, _, peaks0, want0 = cases.dots_counts(None)
    assert np.array_equal(peaks, peaks0) and want["count1"] == want0["count1"] == 17
    assert np.array_equal(want["status1"], want0["status1"])
    moved = np.abs(want["dots1"][:, :2] - want0["dots1"][:, :2])
    pk = np.asarray(peaks, np.int64)
    dist = np.stack([np.abs(want["dots1"][:, 0] - pk % frame.shape[1]), np.abs(want["dots1"][:, 1] - pk // frame.shape[1])], axis=1)
    edge = (np.abs(dist - 1.0) <= td.POS_TOL).any(axis=1)
    print(f"dots, {setting}: threshold {thr:.4f}, background {bg:g}: positions move by at most {np.nanmax(moved):.2e} px, {int(edge.sum())} on the edge")
    assert edge.sum() <= td.MAX_EDGE_SHARE * len(peaks)
    assert np.nanmax(moved) <= 0.05


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_preprocess_models_on_camera_counts_agree(setting):
    frames, floor, want32, want64 = cases.preprocess_counts(setting)
    assert frames.dtype == cases.CAMERA_SETTINGS[setting][2] and np.isfinite(want32).all()
    assert np.abs(want32 - want64).max() <= 4 * 2.0 ** -24 * max(1.0, float(np.abs(want64).max()))      # a few f32 roundings of the result


# ---- exact scale: the f32 models themselves take im 2^k --------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.SCALE_EXPONENTS)
def test_the_f32_models_are_exact_under_a_power_of_two(k):
    """No model carries a constant in intensity units: on im 2^k (floor 2^k, alpha2 4^k) the pre-processing returns its
    result times 2^k where it returns intensities, the terms Ix, Iy, c times 2^k and w over 4^k, the sweeps the same field, and the phase correlator the
    same vectors, flags and planes, all bit for bit.  So all three drivers are in the device's exact-scale test."""
    import optical_flow_cases as oc
    import piv_phase_cases as phc
    from photon_amd import optical_flow as of
    from photon_amd import piv_preprocess as pp
    s = np.float32(2.0 ** k)
    frames, bg, floor, got = cases.preprocess_scaled(k)
    base = pp.preprocess_model_f32(frames / s, bg / s, cases.PREPROCESS["radius"], cases.PREPROCESS["floor"])
    assert np.isfinite(got).all() and (got.tobytes() == base.tobytes() or got.tobytes() == (base * s).tobytes())
    w1, w2, u0, gain, alpha2, terms = cases.terms_scaled(k)
    base = of.terms_model(w1 / s, w2 / s, u0, gain, oc.ALPHA2)
    assert np.isfinite(terms).all()
    assert terms[..., :3].tobytes() == (base[..., :3] * s).tobytes() and terms[..., 3].tobytes() == (base[..., 3] / (s * s)).tobytes()
    swept = cases.sweeps_scaled(k)                      # the sweeps: the field is in pixels, the same bits from scaled and unscaled terms
    assert np.isfinite(swept).all() and swept.tobytes() == of.iterate_model(base, u0, cases.SCALED_SWEEPS).tobytes()
    for index in cases.PHASE_SCALE_CASES:
        _, _, _, want = cases.phase_scaled(index, k)
        _, _, _, base = phc.device_case(index)
        assert np.array_equal(want[1], base[1]) and np.array_equal(want[0], base[0], equal_nan=True)
        assert np.array_equal(want[2], base[2], equal_nan=True)
