"""Masked correlation on the device (photon_piv_correlate_masked, section 17): section 5's bits where no mask looks, the f64
model of photon_amd/piv_mask.py where one does, and the way up through the drivers and the BOS reconstruction."""
import ctypes

import numpy as np
import pytest

import bos_density_cases as bc
import piv_deformation_cases as dc
import piv_mask_cases as cases
import piv_multigrid_cases as mc
from photon_amd import bos_density as bd
from photon_amd import piv_correlation as pc
from photon_amd import piv_mask as pk

pytestmark = pytest.mark.gpu


def device_masked(photon, im1, im2, m1, m2, win, step, R, min_valid, offset=None, planes=True):
    """piv_correlate_masked on host arrays; m1, m2: bool / u8 planes or None (NULL); one array given twice is one pointer.
    Returns numpy (vectors, flags, planes, valid)."""
    import torch
    a, b = (torch.from_numpy(np.array(x, np.float32)).cuda() for x in (im1, im2))
    d1 = None if m1 is None else torch.from_numpy(np.ascontiguousarray(m1, np.uint8)).cuda()
    d2 = d1 if m2 is m1 else None if m2 is None else torch.from_numpy(np.ascontiguousarray(m2, np.uint8)).cuda()
    off = torch.from_numpy(np.array(offset, np.int32)).cuda() if offset is not None else None
    h, w = im1.shape
    out = photon.piv_correlate_masked(a.data_ptr(), b.data_ptr(), 0 if d1 is None else d1.data_ptr(), 0 if d2 is None else d2.data_ptr(), w, h,
                                      win, step, R, min_valid, off.data_ptr() if off is not None else 0, planes=planes)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def device_plain(photon, im1, im2, win, step, R, offset=None):
    import torch
    a, b = (torch.from_numpy(np.array(x, np.float32)).cuda() for x in (im1, im2))
    off = torch.from_numpy(np.array(offset, np.int32)).cuda() if offset is not None else None
    h, w = im1.shape
    out = photon.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, R, off.data_ptr() if off is not None else 0, planes=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def in_image_count(shape, win, step, offset):
    """n_b of a window no mask touches: the pixels of the zero-shift window of b that lie in the image."""
    h, w = shape
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    off = np.zeros((n_rows, n_cols, 2), np.int64) if offset is None else np.asarray(offset, np.int64)
    y0 = (np.arange(n_rows) * step)[:, None] + off[..., 1]
    x0 = (np.arange(n_cols) * step)[None, :] + off[..., 0]
    return (np.clip(np.minimum(y0 + win, h) - np.maximum(y0, 0), 0, None) * np.clip(np.minimum(x0 + win, w) - np.maximum(x0, 0), 0, None))


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=[cases.case_id(c) for c in cases.CASES])
def test_clear_windows_return_section_5s_bits(photon, i):
    """NULL masks, all-zero masks, and a mask that is nonzero only beyond every window's search region: vectors, flags and
    planes are photon_piv_correlate's, bit for bit, on every plan of the list ((64, 32): K = 1; (16, 1): the smallest)."""
    win, R, step, shape, _, _ = cases.CASES[i]
    im1, im2, off = cases.case_pair(i)
    want = device_plain(photon, im1, im2, win, step, R, off)
    far, _ = cases.far_mask(shape, win, step, R, off)
    zeros = np.zeros(shape, np.uint8)
    n_b = in_image_count(shape, win, step, off)
    for name, m1, m2 in (("null", None, None), ("zeros", zeros, zeros), ("one null", None, zeros), ("far", far, far)):
        for min_valid in (1, win * win // 2):
            got = device_masked(photon, im1, im2, m1, m2, win, step, R, min_valid, off)
            assert (n_b >= win * win // 2).all()                     # (no window of the list loses half of b to the image's edge)
            for g, w, what in zip(got, want, ("vectors", "flags", "planes")):
                assert g.tobytes() == w.tobytes(), (name, min_valid, what)
            assert (got[3][..., 0] == win * win).all() and np.array_equal(got[3][..., 1], n_b), name


@pytest.mark.parametrize("kind", cases.MASK_KINDS)
@pytest.mark.parametrize("i", cases.MODEL_CASES, ids=[cases.case_id(cases.CASES[i]) for i in cases.MODEL_CASES])
def test_device_matches_the_host_model(photon, i, kind):
    """f32 against f64 at the bars of test_piv_correlation_gpu (1e-4 of the peak on planes, 1e-3 px on vectors where the
    model's peak stands clear): a pair count N wrong by one in 500 moves a plane value by 2e-3 of itself."""
    win, R, step, shape, _, _ = cases.CASES[i]
    im1, im2, off = cases.model_case(i)
    m1, m2 = cases.masks_of(kind, cases.CASES[i])
    min_valid = win * win // 2
    want = pk.correlate_masked_model(im1, im2, m1, m2, win, step, R, min_valid, offset=off, planes=True, valid=True)
    f = want[1]
    n_clear, n_partial, n_out = (int(x.sum()) for x in ((f & 48) == 0, (f & pk.FLAG_PARTIAL) != 0, (f & pk.FLAG_MASKED_OUT) != 0))
    if kind == "pixels":
        assert n_partial == f.size                                  # every window takes the normalised path
    else:
        assert n_clear and n_partial and n_out, (n_clear, n_partial, n_out)
    got = device_masked(photon, im1, im2, m1, m2 if kind == "two_masks" else m1, win, step, R, min_valid, off)
    assert np.array_equal(got[3], want[3])
    cases.assert_close_to_the_host_model(got[:3], want[:3])


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf, 1e30], ids=["nan", "inf", "-inf", "1e30"])
def test_what_lies_under_a_mask_changes_no_bit(photon, poison):
    for i in (2, 6, 9):
        win, R, step, shape, _, _ = cases.CASES[i]
        im1, im2, off = cases.model_case(i)
        m1, m2 = cases.masks_of("two_masks", cases.CASES[i])
        want = device_masked(photon, im1, im2, m1, m2, win, step, R, win * win // 2, off)
        p1, p2 = im1.copy(), im2.copy()
        p1[m1], p2[m2] = poison, poison
        got = device_masked(photon, p1, p2, m1, m2, win, step, R, win * win // 2, off)
        assert ((want[1] & pk.FLAG_PARTIAL) != 0).any()
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), i


def test_two_calls_return_identical_bits(photon):
    im1, im2 = cases.particle_pair((512, 512), (3.3, -2.7), seed=5)
    mask = cases.disc((512, 512), (300.0, 220.0), 120.0)
    for win, step, R in ((32, 16, 16), (64, 32, 32), (16, 8, 3)):
        a = device_masked(photon, im1, im2, mask, mask, win, step, R, win * win // 2)
        b = device_masked(photon, im1, im2, mask, mask, win, step, R, win * win // 2)
        assert ((a[1] & pk.FLAG_PARTIAL) != 0).any() and ((a[1] & pk.FLAG_MASKED_OUT) != 0).any() and ((a[1] & 48) == 0).any()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_counts_and_bit_16_at_the_threshold(photon):
    im1, im2 = cases.threshold_pair()
    m1, m2 = cases.threshold_masks()
    args = (cases.T_WIN, cases.T_STEP, cases.T_R, cases.T_MIN_VALID)
    want = pk.correlate_masked_model(im1, im2, m1, m2, *args, planes=True, valid=True)
    got = device_masked(photon, im1, im2, m1, m2, *args)
    vec, flg, pl, val = got
    full, mv = cases.T_WIN ** 2, cases.T_MIN_VALID
    assert tuple(val[cases.T_ALIVE]) == (mv, full) and flg[cases.T_ALIVE] == pk.FLAG_PARTIAL and np.isfinite(vec[cases.T_ALIVE]).all()
    assert tuple(val[cases.T_DEAD_A]) == (mv - 1, full) and flg[cases.T_DEAD_A] == pk.FLAG_MASKED_OUT
    assert tuple(val[cases.T_DEAD_B]) == (full, mv - 1) and flg[cases.T_DEAD_B] == pk.FLAG_MASKED_OUT
    for node in (cases.T_DEAD_A, cases.T_DEAD_B):
        assert np.isnan(vec[node]).all() and np.isnan(pl[node]).all()
    assert np.array_equal(val, want[3])
    cases.assert_close_to_the_host_model(got[:3], want[:3])


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.rand((64, 80), device="cuda")
    msk = torch.zeros((64, 80), dtype=torch.uint8, device="cuda")
    vec = torch.full((64, 4), 7.0, device="cuda")
    flg = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    val = torch.full((64, 2), 7, dtype=torch.int32, device="cuda")
    p, m = ctypes.c_void_p(im.data_ptr()), ctypes.c_void_p(msk.data_ptr())
    pv, pf, pn = (ctypes.c_void_p(t.data_ptr()) for t in (vec, flg, val))
    capfd.readouterr()
    for what, args, outs in (("win 24", (p, p, m, m, 80, 64, 24, 8, 4, 1), (pv, pf, pn)), ("win 128", (p, p, m, m, 80, 64, 128, 8, 4, 1), (pv, pf, pn)),
                             ("R 0", (p, p, m, m, 80, 64, 16, 8, 0, 1), (pv, pf, pn)), ("R > win/2", (p, p, m, m, 80, 64, 16, 8, 9, 1), (pv, pf, pn)),
                             ("step 0", (p, p, m, m, 80, 64, 16, 0, 4, 1), (pv, pf, pn)),
                             ("image too small", (p, p, m, m, 80, 15, 16, 8, 4, 1), (pv, pf, pn)),
                             ("null im1", (None, p, m, m, 80, 64, 16, 8, 4, 1), (pv, pf, pn)),
                             ("null im2", (p, None, m, m, 80, 64, 16, 8, 4, 1), (pv, pf, pn)),
                             ("vectors without flags", (p, p, m, m, 80, 64, 16, 8, 4, 1), (pv, None, pn)),
                             ("min_valid 0", (p, p, m, m, 80, 64, 16, 8, 4, 0), (pv, pf, pn)),
                             ("min_valid win^2 + 1", (p, p, None, None, 80, 64, 16, 8, 4, 257), (pv, pf, pn)),
                             ("valid without vectors", (p, p, m, m, 80, 64, 16, 8, 4, 1), (None, None, pn))):
        r, c = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_correlate_masked(*args, None, *outs, None, ctypes.byref(r), ctypes.byref(c), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc != 0, what
        assert len(err.strip().splitlines()) == 1 and "photon_piv_correlate_masked" in err, (what, err)
        assert r.value == -5 and c.value == -5, what
        assert (vec == 7.0).all().item() and (flg == 7).all().item() and (val == 7).all().item(), what
    r, c = ctypes.c_int(0), ctypes.c_int(0)                     # the size query writes the two ints alone
    assert L.photon_piv_correlate_masked(p, p, m, m, 80, 64, 16, 8, 4, 1, None, None, None, None, None, ctypes.byref(r), ctypes.byref(c),
                                         None) == 0
    torch.cuda.synchronize()
    assert (r.value, c.value) == ((64 - 16) // 8 + 1, (80 - 16) // 8 + 1)
    assert (vec == 7.0).all().item() and (flg == 7).all().item() and (val == 7).all().item()
    assert capfd.readouterr().err == ""


# ---- the drivers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 2])
def test_correlate_with_a_mask_is_the_kernel_calls_composed_by_hand(photon, passes):
    im1, im2, mask = cases.body_pair(1)
    im1, im2 = np.array(im1), np.array(im2)                            # (the shared pair is read-only; torch wants a writable array)
    other = cases.disc(cases.S_SHAPE, (40.0, 90.0), 25.0)
    win, step, R = cases.S_WIN, cases.S_STEP, cases.S_R
    for m, (m1, m2) in ((mask, (mask, mask)), ((mask, other), (mask, other))):
        min_valid = pk.min_valid_for(win, 0.3)
        vec, flg, _, _ = device_masked(photon, im1, im2, m1, m2, win, step, R, min_valid)
        if passes == 2:
            off = pc.predictor(vec, flg, pc.normalized_median_test(vec))
            vec, flg, _, _ = device_masked(photon, im1, im2, m1, m2, win, step, R, min_valid, off)
        got_v, got_f = photon.correlate(im1, im2, win, step, R, passes=passes, mask=m, min_valid_fraction=0.3)
        assert got_v.tobytes() == vec.tobytes() and got_f.tobytes() == flg.tobytes()
        out = (flg & pk.FLAG_MASKED_OUT) != 0
        assert out.any() and np.isnan(got_v[out]).all()
        fill_v, fill_f = photon.correlate(im1, im2, win, step, R, passes=passes, mask=m, min_valid_fraction=0.3, fill_masked=True)
        assert np.array_equal(fill_f, flg) and np.array_equal(fill_v, pk.fill_masked(vec, flg, True).astype(np.float32), equal_nan=True)
        assert np.isfinite(fill_v[out][:, :2]).all()
    import torch
    for m in (torch.from_numpy(np.array(mask)).cuda(), [mask.astype(np.uint8) * 255, torch.from_numpy(np.array(other)).cuda()]):
        want = photon.correlate(im1, im2, win, step, R, passes=passes, mask=(mask, other) if isinstance(m, list) else mask)
        got = photon.correlate(im1, im2, win, step, R, passes=passes, mask=m)       # device tensors, bool or u8, any nonzero value
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        photon.correlate(im1, im2, win, step, passes=passes, method="phase", mask=mask)
    with pytest.raises(ValueError, match="does not cover"):
        photon.correlate(im1, im2, win, step, passes=passes, mask=mask[:-1])


def check_driver(name, got, got_fill, want, want_fill, which, rms):
    """A deformation driver under a mask against its model: bit 16 on the same nodes, the NaN / fill rule, and the RMS error
    over the partial windows `which` within 0.02 px of the model's (the margin of the multigrid device tests)."""
    (gv, gs), (gf, gfs), (wv, ws), (wf, wfs) = got, got_fill, want, want_fill
    assert np.array_equal(wfs, ws) and np.isfinite(wf[..., :2]).all()
    out = (ws & pk.FLAG_MASKED_OUT) != 0
    assert out.any() and np.array_equal((gs & pk.FLAG_MASKED_OUT) != 0, out)
    assert np.isnan(gv[out]).all() and np.isfinite(gv[~out][:, :2]).all()
    assert np.array_equal(gfs, gs) and np.isfinite(gf[..., :2]).all() and np.array_equal(gf[~out], gv[~out], equal_nan=True)
    r_dev, r_model = rms(gv, which), rms(wv, which)
    print(f"{name}: {int(which.sum())} partial windows, device {r_dev:.4f} px, model {r_model:.4f} px")
    assert abs(r_dev - r_model) <= 0.02


def test_correlate_deform_with_a_mask(photon):
    im1, im2, mask = cases.vortex_pair(1)
    im1, im2 = np.array(im1), np.array(im2)                            # (the shared pair is read-only; torch wants a writable array)
    which = cases.interior(cases.partial_windows(mask, dc.WIN, dc.STEP))
    got = photon.correlate_deform(im1, im2, **cases.D_ARGS, mask=mask)
    got_fill = photon.correlate_deform(im1, im2, **cases.D_ARGS, mask=mask, fill_masked=True)
    check_driver("correlate_deform", got, got_fill, cases.model_deform(1, True), cases.model_deform(1, True, True), which,
                 lambda v, w: cases.rms_at_centroids(v, w, mask, dc.vortex, dc.WIN, dc.STEP))
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        photon.correlate_deform(im1, im2, **cases.D_ARGS, method="phase", mask=mask)


def test_correlate_multigrid_with_a_mask(photon):
    im1, im2, mask = cases.multigrid_pair(1)
    im1, im2 = np.array(im1), np.array(im2)                            # (the shared pair is read-only; torch wants a writable array)
    win, step = mc.FINAL
    which = cases.interior(cases.partial_windows(mask, win, step))
    assert which.sum() >= 12
    kw = dict(schedule=mc.SCHEDULE, iterations=mc.ITERATIONS, radius=mc.RADIUS["direct"])
    got = photon.correlate_multigrid(im1, im2, **kw, mask=mask)
    got_fill = photon.correlate_multigrid(im1, im2, **kw, mask=mask, fill_masked=True)
    check_driver("correlate_multigrid", got, got_fill, cases.model_multigrid(1), cases.model_multigrid(1, True), which,
                 lambda v, w: cases.rms_at_centroids(v, w, mask, mc.displacement, win, step))
    with pytest.raises(ValueError, match="iteration counts"):           # check_schedule's refusals come first
        photon.correlate_multigrid(im1, im2, mc.SCHEDULE, (1, 1), method="phase", mask=mask)
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        photon.correlate_multigrid(im1, im2, **kw, method="phase", mask=mask)


def test_without_a_mask_the_drivers_return_the_bits_they_returned(photon):
    im1, im2, _ = cases.multigrid_pair(1)
    im1, im2 = np.array(im1), np.array(im2)                            # (the shared pair is read-only; torch wants a writable array)
    for call, kw in ((photon.correlate, dict(win=32, step=16, passes=2)), (photon.correlate_deform, dict(win=32, step=16, iterations=2)),
                     (photon.correlate_multigrid, dict(schedule=mc.SCHEDULE, iterations=mc.ITERATIONS, radius=mc.RADIUS["direct"]))):
        a, b = call(im1, im2, **kw), call(im1, im2, **kw, mask=None, fill_masked=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    import torch
    a = photon.correlation_predictor(im1, im2)
    b = photon.correlation_predictor(im1, im2, mask=None)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    mask = cases.disc(mc.SHAPE, cases.M_CENTRE, cases.M_RADIUS)
    p = photon.correlation_predictor(im1, im2, mask=mask).cpu().numpy()
    filled = photon.correlation_predictor(im1, im2, mask=mask, fill_masked=True).cpu().numpy()
    count, _, _ = pk.window_valid(mask, 32, 16)
    out = count < pk.min_valid_for(32, 0.5)
    assert out.any() and np.isnan(p[out]).all() and np.isfinite(filled).all() and np.array_equal(p[~out], filled[~out])


def test_reconstruct_with_a_mask(photon, tmp_path):
    """A small BOS pair with one corner block of windows outside the dot pattern: phi is NaN exactly on the nodes the model
    leaves NaN, and within test_bos_density_gpu's margin of integrate_model on the same gradients."""
    n_pix = 128
    c1, c2 = bc.blob_calls(photon, str(tmp_path), False, n_pix=n_pix)
    im1, im2 = (photon.render(c).reshape(n_pix, n_pix).astype(np.float32) for c in (c1, c2))
    mask = np.zeros((n_pix, n_pix), bool)
    mask[:56, :56] = True                                              # windows (0..1, 0..1) wholly, the next ring in part
    args = (c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    vectors, flags = photon.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2, mask=mask)
    out = (flags & pk.FLAG_MASKED_OUT) != 0
    assert out[:2, :2].all() and out.sum() < out.size // 2 and np.isnan(vectors[out]).all()
    gx, gy, w, _, _, h = bd.measured_gradients(vectors, flags, (n_pix, n_pix), *args)
    assert (w[out] == 0).all()
    want, ws = bd.integrate_model(gx, gy, w, hx=h, hy=h, tol=1e-8)
    phi, mid, st = bd.reconstruct(photon, im1, im2, *args, passes=2, mask=mask)
    assert st["converged"] == 1 and ws["converged"] == 1
    assert np.array_equal(np.isnan(phi), np.isnan(want)) and np.isnan(want[1, 1]) and np.isfinite(phi).any()
    assert np.nanmax(np.abs(phi - want)) <= 1e-6 * np.nanmax(np.abs(want))
    g1, g2, w2, _ = bd.deflection_data(photon, im1, im2, *args, passes=2, mask=mask)
    assert np.array_equal(w2, w) and np.array_equal(g1, gx, equal_nan=True) and np.array_equal(g2, gy, equal_nan=True)
