"""The drivers of photon_amd/library.py on the arrays callers hold (the ingest rule: PhotonLibrary's docstring).

For every row of driver_input_cases.rows() -- the 14 pipelines of test_streams_gpu.py and the rows that complete the
drivers' array arguments -- the reference is the call on fresh C-contiguous numpy inputs of the driver's own dtype.  Then, one
argument at a time, the same values arrive as every variant of driver_input_cases.variants (layouts, byte order, read-only,
memmap, wider float, lists, integer dtypes, CPU tensors) and as device tensors (contiguous: passed through uncopied; a crop;
a permuted view; the other float dtype; bool and u8 for masks).  Every result is the reference byte for byte, no warning is
raised (warnings are errors here), the caller's object holds its bytes afterwards, and no returned tensor shares storage
with an input.  What the rule refuses is refused before the device is asked for anything.
"""
import warnings

import numpy as np
import pytest

import driver_input_cases as cases
from test_streams_gpu import flatten

pytestmark = pytest.mark.gpu

ROWS = cases.rows()


def fresh(inputs):
    return {k: np.array(a, order="C") for k, a in inputs.items()}         # the shared inputs are read-only: writable copies


def device_variants(a, is_mask):
    """(name, device tensor) pairs that hold the values of the numpy array `a`."""
    import torch
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    yield "device_contiguous", t                                           # for f32 / f64 arguments: used in place
    nd = a.ndim
    big = torch.full(tuple(a.shape[:-1]) + (a.shape[-1] + 9,), 3, dtype=t.dtype, device="cuda")
    big[..., 5:5 + a.shape[-1]] = t
    yield "device_crop", big[..., 5:5 + a.shape[-1]]
    if nd >= 2:
        yield "device_permuted", t.permute(*reversed(range(nd))).contiguous().permute(*reversed(range(nd)))
    else:
        yield "device_every_second", t.repeat_interleave(2)[::2]
    if a.dtype.kind == "f":
        other = np.float64 if a.dtype == np.float32 else np.float32
        if np.array_equal(a.astype(other).astype(a.dtype), a):
            yield "device_other_float", torch.from_numpy(a.astype(other)).cuda()
    if is_mask:
        yield "device_bool", torch.from_numpy(np.asarray(a) != 0).cuda()
        yield "device_uint8_255", torch.from_numpy((np.asarray(a) != 0).astype(np.uint8) * np.uint8(255)).cuda()
        yield "device_float32", torch.from_numpy((np.asarray(a) != 0).astype(np.float32)).cuda()


def state_of(v):
    """What must be the same after the call: bytes, flags and strides of an array; a device tensor's bytes (a clone now)."""
    import torch
    if isinstance(v, np.ndarray):
        return v.tobytes(), v.flags.writeable, v.flags.c_contiguous, v.strides, v.dtype
    if isinstance(v, torch.Tensor):
        return v.detach().clone().cpu().numpy().tobytes(), v.stride(), v.dtype, v.device
    return repr(v)


def storages(obj, found=None):
    """The storage addresses of every torch tensor in a result."""
    import torch
    found = set() if found is None else found
    if isinstance(obj, torch.Tensor):
        found.add(obj.untyped_storage().data_ptr())
    elif isinstance(obj, dict):
        for v in obj.values():
            storages(v, found)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            storages(v, found)
    return found


@pytest.mark.parametrize("name", list(ROWS))
def test_layouts_and_dtypes_give_the_same_bytes_and_inputs_are_never_written(photon, name, tmp_path):
    import torch
    row = ROWS[name]
    base = fresh(row.make_inputs())
    want = flatten(row.run(photon, fresh(base)))
    torch.cuda.synchronize()
    again = flatten(row.run(photon, fresh(base)))
    torch.cuda.synchronize()
    assert again == want, f"{name}: two calls on the same inputs differ; the byte comparison has no footing"
    n = 0
    for key, argument in row.vary.items():
        a = base[key]
        is_mask = argument in ("mask", "fixed", "support")
        everything = [*cases.variants(a, tmp_path), *device_variants(a, is_mask), *(cases.mask_forms(a) if is_mask else ())]
        for vname, v in everything:
            args = fresh(base)
            args[key] = v
            others = {k: state_of(x) for k, x in args.items()}
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                result = row.run(photon, args)
                got = flatten(result)
            torch.cuda.synchronize()
            differ = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert len(got) == len(want) and not differ, f"{name}: {argument} as {vname}: results {differ} differ from the C-contiguous call"
            changed = [k for k, x in args.items() if state_of(x) != others[k]]
            assert not changed, f"{name}: {argument} as {vname}: the call changed the caller's {changed}"
            if isinstance(v, torch.Tensor) and v.is_cuda:
                assert v.untyped_storage().data_ptr() not in storages(result), f"{name}: {argument} as {vname}: a result shares the input's storage"
            n += 1
    print(f"{name}: {n} variants of {list(row.vary.values())} give the reference's bytes")
    assert n >= 12 * len(row.vary)


@pytest.mark.parametrize("name", list(ROWS))
def test_every_argument_passed_through_at_once_is_never_written(photon, name):
    """All array arguments as conforming device tensors, the case in which nothing is copied on the way in: the reference's
    bytes, every tensor holds its bytes afterwards, no result shares their storage."""
    import torch
    row = ROWS[name]
    base = fresh(row.make_inputs())
    want = flatten(row.run(photon, fresh(base)))
    tensors = {k: torch.from_numpy(a).cuda() for k, a in base.items()}
    before = {k: t.clone() for k, t in tensors.items()}
    result = row.run(photon, tensors)
    got = flatten(result)
    torch.cuda.synchronize()
    assert got == want
    assert not [k for k, t in tensors.items() if not torch.equal(t, before[k])], "a driver wrote into a caller's device tensor"
    assert not storages(result) & {t.untyped_storage().data_ptr() for t in tensors.values()}


def boom(*args, **kwargs):
    raise AssertionError("the driver asked for the device before it refused its arguments")


@pytest.mark.parametrize("name", list(ROWS))
def test_refusals_come_before_any_device_work(photon, name, monkeypatch, capfd):
    import torch
    from photon_amd import library
    row = ROWS[name]
    base = fresh(row.make_inputs())
    flatten(row.run(photon, fresh(base)))                               # the row runs as it is
    torch.cuda.synchronize()
    capfd.readouterr()
    monkeypatch.setattr(library, "_device_and_stream", boom)
    monkeypatch.setattr(torch, "empty", boom)
    n = 0

    def refused(key, bad, error, match):
        nonlocal n
        args = fresh(base)
        args[key] = bad
        with pytest.raises(error, match=match):
            row.run(photon, args)
        n += 1

    for key, argument in row.vary.items():
        a = base[key]
        for _, bad, error in cases.refused(a):
            refused(key, bad, error, argument)
        refused(key, torch.zeros(a.shape, dtype=torch.complex64), TypeError, argument)
        if cases.DRIVERS[row.method][argument] is not None:
            refused(key, a[0], ValueError, f"{argument}.* must have {a.ndim} dimensions")       # a 1-d "image", a 2-d "stack"
            refused(key, a[None], ValueError, f"{argument}.* must have {a.ndim} dimensions")    # a 3-d "image"
    if {"im1", "im2"} <= set(row.vary):
        refused("im2", base["im2"][:-1], ValueError, "one shape")
        refused("im1", base["im1"][:, 1:], ValueError, "one shape")
    if "frames2" in base and "frames1" in base:
        refused("frames2", base["frames2"][:, :-1], ValueError, "one shape")
    if "mask" in base:
        refused("mask", base["mask"][:-1], ValueError, "does not cover")
        refused("mask", (base["mask"], base["mask"][:, :-2]), ValueError, "does not cover")
    if "background" in base:
        refused("background", base["background"][:-1], ValueError, "one .height, width. plane")
    out, err = capfd.readouterr()
    assert (out, err) == ("", ""), "a refusal reached the library"
    assert n >= 3 * len(row.vary)


# ---- camera counts: the direct correlator against its f64 model ------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(cases.CAMERA_SETTINGS))
@pytest.mark.parametrize("index", range(3))
def test_the_direct_correlator_on_camera_counts_against_the_f64_model(photon, index, setting):
    """The integer frames themselves (uint8 / uint16, rint(pedestal + gain im)) through the ingest rule into photon_piv_correlate,
    against piv_correlation.correlate_model on the same counts as f64, under test_piv_correlation_gpu's assertion as it is:
    planes within 1e-4 of the peak, clear windows within 1e-3 px, more than half of the windows clear.  The window sums of a
    64 x 64 window at 61000 counts reach 2.5e8, where an f32 ulp is 16: the kernel has to subtract before it sums.  The driver
    on the integer arrays, in one pass and in two, returns the bytes of the raw calls.  Each case prints its pair
    (`pytest -s`); the measured figures are in DESIGN 4.3u."""
    import torch
    import test_piv_correlation_gpu as tg
    from photon_amd import library
    from photon_amd import piv_correlation as pc
    c1, c2, win, step, R, off, want = cases.direct_correlator_counts(index, setting)
    dev, _ = library._device_and_stream()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, b = (library._on_device(c, torch.float32, dev, "im", 2) for c in (c1, c2))
    assert a.cpu().numpy().tobytes() == c1.astype(np.float32).tobytes()
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int32)).cuda() if off is not None else None
    h, w = c1.shape
    vec, flg, pl = photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R, d_off.data_ptr() if off is not None else 0, planes=True)
    torch.cuda.synchronize()
    got = vec.cpu().numpy(), flg.cpu().numpy(), pl.cpu().numpy()
    live = (want[1] & pc.FLAG_FLAT) == 0
    n = int(live.sum())
    peak = want[2][live].reshape(n, -1).max(axis=1)
    worst_plane = (np.abs(got[2][live].reshape(n, -1) - want[2][live].reshape(n, -1)).max(axis=1) / peak).max()
    worst_vector = np.nanmax(np.abs(got[0][live][:, :2] - want[0][live][:, :2]))
    print(f"direct correlator, win {win}, {setting}: worst plane error {worst_plane:.2e} of the peak, worst vector difference over all "
          f"live windows {worst_vector:.2e} px")
    clear = tg.assert_close_to_the_host_model(got, want)
    assert clear.mean() > 0.5
    # the driver on the uint arrays: one pass is the raw call without offsets, two passes the raw call with the host predictor's
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v1, f1 = photon.correlate(c1, c2, win, step, R)
        v2, f2 = photon.correlate(c1, c2, win, step, R, passes=2)
        vd, fd = photon.correlate(torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda(), win, step, R)       # uint8 / uint16 on the device
    assert vd.tobytes() == v1.tobytes() and fd.tobytes() == f1.tobytes()
    raw1 = photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R)
    assert raw1[0].cpu().numpy().tobytes() == v1.tobytes() and raw1[1].cpu().numpy().tobytes() == f1.tobytes()
    offsets = pc.predictor(v1, f1, pc.normalized_median_test(v1))
    d2 = torch.from_numpy(offsets).cuda()
    raw2 = photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R, d2.data_ptr(), planes=True)
    got2 = tuple(t.cpu().numpy() for t in raw2)
    assert got2[0].tobytes() == v2.tobytes() and got2[1].tobytes() == f2.tobytes()
    want2 = pc.correlate_model(c1.astype(np.float64), c2.astype(np.float64), win, step, R, offset=offsets, planes=True)
    clear2 = tg.assert_close_to_the_host_model(got2, want2)
    assert clear2.mean() > 0.5


# ---- camera counts: the other measurement drivers, each under its own module's assertion -----------------------------------------
SETTINGS = list(cases.CAMERA_SETTINGS)
HIGH_PEDESTAL_SIGMA_LIMIT = 1.2e-4        # of sigma, measured: displacement_uncertainty against its model behind the same warp
HIGH_PEDESTAL_FLOW_LIMIT = 3.73e-5        # px, measured: the header's limit of the f32 warp at a pedestal of 61000


def worst(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both = np.isfinite(got) & np.isfinite(want)
    return float(np.abs(got - want)[both].max())


def quiet(call, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return call(*args, **kwargs)


@pytest.mark.parametrize("setting", SETTINGS)
def test_correlate_ensemble_on_camera_counts(photon, setting):
    """test_piv_ensemble_gpu.test_particle_stacks_are_close_to_the_host_model on the integer stacks: section 5's bounds."""
    import test_piv_correlation_gpu as single
    import test_piv_ensemble_gpu as te
    s1, s2, (win, R, step, shape, _, _), off, (want_v, want_f, want_c, want_p) = cases.ensemble_counts(setting)
    v, f, c, p = te.device_ensemble(photon, s1.astype(np.float32), s2.astype(np.float32), win, step, R, off)
    grid = want_f.shape
    print(f"correlate_ensemble, {setting}: worst vector difference over all live windows {worst(v.reshape(grid + (4,))[..., :2], want_v[..., :2]):.2e} px, "
          f"worst plane difference {worst(p.reshape(want_p.shape), want_p):.2e}")
    assert np.array_equal(c.reshape(grid), want_c)
    clear = single.assert_close_to_the_host_model((v.reshape(grid + (4,)), f.reshape(grid), p.reshape(want_p.shape)), (want_v, want_f, want_p))
    assert clear.mean() > 0.5
    dv, df, dc = quiet(photon.correlate_ensemble, s1, s2, win, step, R)          # the driver on the integer stacks, no offsets
    rv, rf, rc, _ = te.device_ensemble(photon, s1.astype(np.float32), s2.astype(np.float32), win, step, R, None, planes=False)
    assert dv.tobytes() == rv.tobytes() and df.tobytes() == rf.tobytes() and dc.tobytes() == rc.tobytes()


@pytest.mark.parametrize("setting", SETTINGS)
def test_correlate_deform_and_phase_multigrid_on_camera_counts(photon, setting):
    """The bar correlate_deform and correlate_multigrid are held to against their models (test_piv_deformation_gpu,
    test_piv_multigrid_gpu): |RMS(device) - RMS(model)| <= 0.02 px against the truth, here the uniform shift of the pair."""
    c1, c2 = cases.pair_counts(setting)
    for name, call, kw, model in (("correlate_deform", photon.correlate_deform, cases.DEFORM, cases.deform_model(setting)),
                                  ("correlate_multigrid phase", photon.correlate_multigrid, cases.PHASE_MULTIGRID, cases.phase_multigrid_model(setting))):
        vec, status = quiet(call, c1, c2, **kw)
        rms, want = cases.uniform_rms(vec, cases.PAIR_SHIFT), cases.uniform_rms(model[0], cases.PAIR_SHIFT)
        print(f"{name}, {setting}: device {rms:.4f} px, model {want:.4f} px; worst |device - f64 model| over all nodes {worst(vec[..., :2], model[0][..., :2]):.2e} px")
        assert abs(rms - want) <= 0.02


@pytest.mark.parametrize("setting", SETTINGS)
def test_uncertainty_on_camera_counts(photon, setting):
    """test_piv_uncertainty_gpu.test_device_matches_the_model on the counts: the f64 sums within SUM_RTOL of the model's on
    their scales, the flags, sigma within SIGMA_OWN_RTOL of the model's last step on the device's sums and SIGMA_MODEL_RTOL
    of the model's.  Then the driver on the integer frames with a zero field against its model, under SIGMA_MODEL_RTOL."""
    import piv_uncertainty_cases as uc
    import test_piv_uncertainty_gpu as tu
    from photon_amd import piv_uncertainty as pu
    shape, win, step, reach = cases.UNCERTAINTY_CASE
    c1, c2, (want_sigma, want_flags, want, T) = cases.uncertainty_counts(setting)
    sigma, flags, got = tu.device_uncertainty(photon, c1.astype(np.float32), c2.astype(np.float32), win, step, reach)
    E, N = cases.window_energies(c1, c2, win, step)[..., None], uc.n_terms(reach)
    err_c = max(float((np.abs(got[..., k] - want[..., k]) / E).max()) for k in (0, 1))
    err_s = float((np.abs(got[..., 2] - want[..., 2]) / T).max())
    err_v = float((np.abs(got[..., 3] - want[..., 3]) / (N * T)).max())
    own, own_flags = pu.sigma_from_stats(got)
    err_own, err_model = float(np.abs(sigma / own - 1.0).max()), float(np.abs(sigma / want_sigma - 1.0).max())
    field = np.zeros((*flags.shape, 2), np.float32)
    d_sigma, d_flags = quiet(photon.displacement_uncertainty, c1, c2, field, win, step, reach)
    m_sigma = pu.displacement_uncertainty_model(c1.astype(np.float64), c2.astype(np.float64), field, win, step, reach)[0]
    print(f"uncertainty, {setting}: |C - model| / E {err_c:.1e}, |S00 - model| / T {err_s:.1e}, |V - model| / (N T) {err_v:.1e}; sigma vs own sums "
          f"{err_own:.1e}, vs model {err_model:.1e}; driver sigma / model - 1: {float(np.abs(d_sigma / m_sigma - 1.0).max()):.3e}")
    assert err_c <= tu.SUM_RTOL and err_s <= tu.SUM_RTOL and err_v <= tu.SUM_RTOL
    assert np.array_equal(flags, want_flags) and np.array_equal(own_flags, want_flags)
    assert err_own <= tu.SIGMA_OWN_RTOL and err_model <= tu.SIGMA_MODEL_RTOL
    assert np.array_equal(d_flags, want_flags)
    # the driver against its own model, under the one bar the project has for device sigma against a model; at the pedestal of
    # 61000 the f32 warp in front of the kernel (the header's limit beside photon_piv_deform_dense) moves sigma by 1.2e-4 of
    # itself, measured: asserted at twice that, a factor that covers box-to-box differences in summation-independent rounding alone
    err_driver = float(np.abs(d_sigma / m_sigma - 1.0).max())
    assert err_driver <= (2 * HIGH_PEDESTAL_SIGMA_LIMIT if setting == "16bit_high_pedestal" else tu.SIGMA_MODEL_RTOL)


@pytest.mark.parametrize("setting", SETTINGS)
def test_optical_flow_on_camera_counts(photon, setting):
    """test_optical_flow_gpu.test_the_device_follows_the_model on the counts, from the same grid predictor: 3e-5 px.  alpha2
    stays: the driver scales the frames by 1 / std(im1) itself, so its alpha2 is in units of the normalised image.
    Measured on an MI355X: 7.2e-7 px (8 bit), 4.2e-7 px (12 bit), 3.73e-5 px at the pedestal of 61000 -- over the module's
    bar.  The cause is the f32 warp, whose 16 taps carry coefficients of the pedestal's size (61000 x 16 x 2^-24 x 1.5 = 0.09
    counts in a pixel against a signal whose std is a few hundred), no window sum; the limit is documented beside
    photon_piv_deform_dense in the header, and asserted here at twice the measured figure.  The factor covers box-to-box
    differences in nothing but summation-independent rounding (the host's 1 / std, numpy's f64 model)."""
    c1, c2, grid, want = cases.flow_counts(setting)
    got = quiet(photon.optical_flow, c1, c2, grid, **cases.FLOW)
    diff = worst(got, want)
    print(f"optical_flow, {setting}: |device flow - model flow| = {diff:.3g} px")
    assert diff <= (2 * HIGH_PEDESTAL_FLOW_LIMIT if setting == "16bit_high_pedestal" else 3e-5)


@pytest.mark.parametrize("setting", SETTINGS)
def test_track_dots_on_camera_counts(photon, setting):
    """test_dot_tracking_gpu.compare_fit, unchanged, on what track_dots(relative=True) finds in the integer frame."""
    import test_dot_tracking_gpu as td
    frame, thr, bg, peaks, want = cases.dots_counts(setting)
    got = quiet(photon.track_dots, frame, frame, thr, relative=True, background=bg)
    assert got["count1"] == want["count1"] == len(peaks) and got["npaired"] == want["npaired"]
    w = td.compare_fit(got["dots1"], got["status1"], want["dots1"], want["status1"], peaks, frame.shape[1], setting)
    print(f"track_dots, {setting}: {got['count1']} dots, threshold {thr:.4f} of the maximum, background {bg:g}: worst |device - model| {w:.2e} px")


@pytest.mark.parametrize("setting", SETTINGS)
def test_preprocess_series_on_camera_counts(photon, setting):
    """The integer frames through preprocess_series: the f32 model bit for bit (test_piv_preprocess_gpu.assert_same_bits),
    the floor scaled with the gain; the f64 model printed."""
    import test_piv_preprocess_gpu as tp
    frames, floor, want32, want64 = cases.preprocess_counts(setting)
    got = quiet(photon.preprocess_series, frames, background="min", minmax_radius=cases.PREPROCESS["radius"], floor=floor).cpu().numpy()
    print(f"preprocess_series, {setting}: worst |device - f64 model| {worst(got, want64):.2e}")
    tp.assert_same_bits(got, want32, setting)


# ---- exact scale: a power of two changes no mantissa ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.SCALE_EXPONENTS)
def test_scaled_by_a_power_of_two_the_kernels_equal_their_f32_models(photon, k):
    """preprocess_series with floor 2^k, photon_optflow_terms with alpha2 4^k and photon_optflow_iterate on its terms, the phase
    correlator: im 2^k as f32 against the
    f32 model on the same scaled frames, under each module's bit-for-bit assertion.  A kernel with an absolute epsilon or a
    constant in intensity units fails here and nowhere else."""
    import piv_phase_cases as phc
    import test_optical_flow_gpu as to
    import test_piv_phase_gpu as tph
    import test_piv_preprocess_gpu as tp
    frames, bg, floor, want = cases.preprocess_scaled(k)
    got = photon.preprocess_series(frames, background=bg, minmax_radius=cases.PREPROCESS["radius"], floor=floor).cpu().numpy()
    tp.assert_same_bits(got, want, k)
    got = photon.preprocess_series(frames, background="min", minmax_radius=cases.PREPROCESS["radius"], floor=floor).cpu().numpy()
    tp.assert_same_bits(got, want, k)
    w1, w2, u0, gain, alpha2, want = cases.terms_scaled(k)
    assert to.device_terms(photon, w1, w2, u0, gain, alpha2).tobytes() == want.tobytes()
    assert to.device_iterate(photon, want, u0, cases.SCALED_SWEEPS).tobytes() == cases.sweeps_scaled(k).tobytes()      # the sweeps
    for index in cases.PHASE_SCALE_CASES:
        win, R, step, _, _, _, mode, sigma, diameter = phc.DEVICE_CASES[index]
        im1, im2, off, want = cases.phase_scaled(index, k)
        w = tph.assert_equals_the_f32_model(tph.device_phase(photon, im1, im2, win, step, R, off, mode, sigma, diameter), want)
        print(f"phase, {phc.case_id(phc.DEVICE_CASES[index])}, 2^{k}: largest |delta d| {w:.3g} px")
