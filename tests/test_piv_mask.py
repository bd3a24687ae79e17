"""Masked correlation, CPU tier: the f64 host model of section 17 (photon_amd/piv_mask.py) against section 5's model where
no mask looks, its indifference to what lies under a mask, the counts and bits at the threshold, and the two studies with
a stationary textured body in the frame (the figures of DESIGN.md section 4.3p)."""
import numpy as np
import pytest

import piv_deformation_cases as dc
import piv_mask_cases as cases
import piv_multigrid_cases as mc
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_mask as pk
from photon_amd import piv_multigrid as pm


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=[cases.case_id(c) for c in cases.CASES])
def test_without_a_masked_pixel_in_sight_the_model_is_section_5s(i):
    win, R, step, shape, _, _ = cases.CASES[i]
    im1, im2, off = cases.case_pair(i)
    want = pc.correlate_model(im1, im2, win, step, R, offset=off, planes=True)
    far, _ = cases.far_mask(shape, win, step, R, off)
    for m1, m2 in ((None, None), (np.zeros(shape, np.uint8), None), (far, far)):
        got = pk.correlate_masked_model(im1, im2, m1, m2, win, step, R, 1, offset=off, planes=True, valid=True)
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)
        assert (got[3][..., 0] == win * win).all()
        assert (got[1] & (pk.FLAG_MASKED_OUT | pk.FLAG_PARTIAL)).max() == 0


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf, 1e30])
def test_what_lies_under_a_mask_changes_no_output(poison):
    i = 4
    win, R, step, shape, _, _ = cases.CASES[i]
    im1, im2, off = cases.case_pair(i)
    m1, m2 = cases.masks_of("two_masks", cases.CASES[i])
    want = pk.correlate_masked_model(im1, im2, m1, m2, win, step, R, win * win // 2, offset=off, planes=True, valid=True)
    p1, p2 = im1.copy(), im2.copy()
    p1[m1], p2[m2] = poison, poison
    with np.errstate(all="raise"):
        got = pk.correlate_masked_model(p1, p2, m1, m2, win, step, R, win * win // 2, offset=off, planes=True, valid=True)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_counts_and_bit_16_at_the_threshold():
    im1, im2 = cases.threshold_pair()
    m1, m2 = cases.threshold_masks()
    vec, flg, val = pk.correlate_masked_model(im1, im2, m1, m2, cases.T_WIN, cases.T_STEP, cases.T_R, cases.T_MIN_VALID, valid=True)
    full, mv = cases.T_WIN ** 2, cases.T_MIN_VALID
    assert tuple(val[cases.T_ALIVE]) == (mv, full) and flg[cases.T_ALIVE] == pk.FLAG_PARTIAL
    assert np.isfinite(vec[cases.T_ALIVE]).all()
    assert tuple(val[cases.T_DEAD_A]) == (mv - 1, full) and flg[cases.T_DEAD_A] == pk.FLAG_MASKED_OUT
    assert tuple(val[cases.T_DEAD_B]) == (full, mv - 1) and flg[cases.T_DEAD_B] == pk.FLAG_MASKED_OUT
    assert np.isnan(vec[cases.T_DEAD_A]).all() and np.isnan(vec[cases.T_DEAD_B]).all()
    assert ((flg & pk.FLAG_MASKED_OUT) != 0).sum() == 2
    # the refusals of min_valid
    for bad in (0, full + 1):
        with pytest.raises(ValueError, match="min_valid"):
            pk.correlate_masked_model(im1, im2, m1, m2, cases.T_WIN, cases.T_STEP, cases.T_R, bad)


@pytest.mark.parametrize("i", [1, 2, 6], ids=[cases.case_id(cases.CASES[i]) for i in (1, 2, 6)])
def test_bit_32_is_set_exactly_where_a_window_looks_at_a_masked_pixel(i):
    """Written from the definition, window by window: mask1 over a's window, mask2 over the in-image part of b's search
    region (offset applied)."""
    win, R, step, shape, _, _ = cases.CASES[i]
    im1, im2, off = cases.model_case(i)
    h, w = shape
    for kind in ("disc", "two_masks"):
        m1, m2 = cases.masks_of(kind, cases.CASES[i])
        _, flg, val = pk.correlate_masked_model(im1, im2, m1, m2, win, step, R, win * win // 2, offset=off, valid=True)
        for r in range(flg.shape[0]):
            for c in range(flg.shape[1]):
                ox, oy = (0, 0) if off is None else off[r, c]
                y0, x0 = r * step, c * step
                seen = m1[y0:y0 + win, x0:x0 + win].any() or \
                    m2[max(y0 + oy - R, 0):max(y0 + oy + win + R, 0), max(x0 + ox - R, 0):max(x0 + ox + win + R, 0)].any()
                out = min(val[r, c]) < win * win // 2
                assert bool(flg[r, c] & pk.FLAG_MASKED_OUT) == out
                assert bool(flg[r, c] & pk.FLAG_PARTIAL) == (seen and not out), (kind, r, c)
                assert not (out and flg[r, c] & pc.FLAG_FLAT)


def test_window_valid_counts_and_centroids():
    mask = np.zeros((40, 56), bool)
    mask[:, 30:] = True                                                # columns 30.. are gone
    count, row, col = pk.window_valid(mask, 16, 8)
    assert count.shape == pc.grid_shape(mask.shape, 16, 8)
    assert count[0].tolist() == [256, 256, 16 * 14, 16 * 6, 0, 0]
    assert np.allclose(row[:, :4], (np.arange(4) * 8 + 7.5)[:, None])
    assert np.allclose(col[0, :4], [7.5, 15.5, (16 + 29) / 2.0, (24 + 29) / 2.0]) and np.isnan(col[0, 4:]).all()


def test_fill_masked():
    v = np.arange(3 * 3 * 4, dtype=np.float64).reshape(3, 3, 4)
    status = np.zeros((3, 3), np.int32)
    status[1, 1], status[0, 0] = pk.FLAG_MASKED_OUT | pd.FLAG_REPLACED, pk.FLAG_MASKED_OUT
    v[0, 0] = np.nan
    blank = pk.fill_masked(v, status)
    assert np.isnan(blank[1, 1]).all() and np.isnan(blank[0, 0]).all() and np.isfinite(blank[status == 0]).all()
    filled = pk.fill_masked(v, status, True)
    assert np.array_equal(filled[1, 1], v[1, 1])                       # the loop's median stays
    assert filled[0, 0, :2].tolist() == [np.median([4.0, 12.0, 16.0]), np.median([5.0, 13.0, 17.0])] and np.isnan(filled[0, 0, 2:]).all()


def test_the_mask_saves_the_windows_a_stationary_body_cuts():
    """Study 1: 128 x 176, uniform shift (3.3, -2.1) px, a bright stationary texture to the right of
    a slanted edge; 32 / 16 windows, R 8, seeds 1 .. 12, over the partially masked windows (bit 32: the body lies in the
    window or in its search region, and at least half of the window is free).  The
    share of vectors more than 1 px from the shift: the masked model at most 5 %, section 5's model at least 50 %."""
    wrong_masked = wrong_plain = total = 0
    for seed in cases.S_SEEDS:
        im1, im2, mask = cases.body_pair(seed)
        vm, fm = pk.correlate_masked_model(im1, im2, mask, mask, cases.S_WIN, cases.S_STEP, cases.S_R, pk.min_valid_for(cases.S_WIN, 0.5))
        which = (fm & pk.FLAG_PARTIAL) != 0
        assert which[cases.partial_windows(mask, cases.S_WIN, cases.S_STEP)].all()
        vp, _ = pc.correlate_model(im1, im2, cases.S_WIN, cases.S_STEP, cases.S_R)
        wrong_masked += cases.off_by_more_than_a_pixel(vm, which)[0]
        bad, n = cases.off_by_more_than_a_pixel(vp, which)
        wrong_plain, total = wrong_plain + bad, total + n
    print(f"masked {wrong_masked} / {total}, section 5 {wrong_plain} / {total}")
    assert total >= 100
    assert wrong_masked <= 0.05 * total
    assert wrong_plain >= 0.5 * total


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_deformation_loop_under_a_mask(seed):
    """Study 2: the vortex pair with a stationary textured disc of radius 30 at (200, 72),
    correlate_deform(32, 16, radius 16, iterations 3), over the interior partially masked windows, against the truth at the
    centroid of each window's free pixels."""
    im1, im2, mask = cases.vortex_pair(seed)
    which = cases.interior(cases.partial_windows(mask, dc.WIN, dc.STEP))
    assert which.sum() >= 12
    vm, sm = cases.model_deform(seed, True)
    vp, _ = cases.model_deform(seed, False)
    rms_m = cases.rms_at_centroids(vm, which, mask, dc.vortex, dc.WIN, dc.STEP)
    rms_p = cases.rms_at_centroids(vp, which, mask, dc.vortex, dc.WIN, dc.STEP)
    print(f"seed {seed}: {int(which.sum())} windows, masked {rms_m:.4f} px, unmasked {rms_p:.4f} px")
    assert rms_m <= 0.1 * rms_p
    assert ((sm[which] & pd.FLAG_REPLACED) != 0).mean() <= 0.1
    out = (sm & pk.FLAG_MASKED_OUT) != 0
    assert out.any() and (sm[out] == (pk.FLAG_MASKED_OUT | pd.FLAG_REPLACED) | (sm[out] & pc.FLAG_OUTSIDE)).all()
    assert np.isnan(vm[out]).all() and np.isfinite(vm[~out][:, :2]).all()
    vf, sf = cases.model_deform(seed, True, True)
    assert np.array_equal(sf, sm) and np.isfinite(vf[..., :2]).all()
    assert np.array_equal(vf[~out], vm[~out], equal_nan=True)


def test_phase_correlation_refuses_a_mask_after_the_schedule_is_checked():
    im1, im2, mask = cases.multigrid_pair(1)
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        pm.correlate_multigrid_model(im1, im2, mc.SCHEDULE, mc.ITERATIONS, method="phase", mask=mask)
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        pd.correlate_deform_model(im1, im2, method="phase", mask=mask)
    with pytest.raises(ValueError, match="phase correlator has no masks"):
        pd.model_correlator("phase", 32, None, None, 2.5, mask=mask)
    with pytest.raises(ValueError, match="iteration counts"):             # check_schedule's refusals come first
        pm.correlate_multigrid_model(im1, im2, mc.SCHEDULE, (1, 1), method="phase", mask=mask)
    with pytest.raises(ValueError, match="does not cover"):
        pd.correlate_deform_model(im1, im2, mask=mask[:-1])
    with pytest.raises(ValueError, match="min_valid_fraction"):
        pd.correlate_deform_model(im1, im2, mask=mask, min_valid_fraction=0.0)
    # without a mask the correlators are the ones the models had
    assert pd.model_correlator("direct", 32, None, None, 2.5)[0] is pc.correlate_model


def test_every_multigrid_level_takes_min_valid_from_its_own_window():
    assert [pk.min_valid_for(w, 0.5) for w in (16, 32, 64)] == [128, 512, 2048]
    assert pk.min_valid_for(16, 0.3) == 77 and pk.min_valid_for(16, 1.0) == 256
    vec, status = cases.model_multigrid(1)
    im1, im2, mask = cases.multigrid_pair(1)
    count, _, _ = pk.window_valid(mask, *mc.FINAL)
    assert np.array_equal((status & pk.FLAG_MASKED_OUT) != 0, count < 128)
    assert np.isnan(vec[count < 128]).all()
