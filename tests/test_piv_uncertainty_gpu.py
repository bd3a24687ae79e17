"""photon_piv_uncertainty on the GPU (include/parallel_ray_tracing.h, section 11): the device's sums, flags and sigma against
the f64 model of photon_amd/piv_uncertainty.py on every case, repeat bits, refusals, the driver against its parts, the
calibration against pairs with a known displacement, and the weights in the BOS loop."""
import ctypes

import numpy as np
import pytest

import bos_density_cases as bc
import piv_deformation_cases as dc
import piv_uncertainty_cases as uc
import test_bos_density_gpu as bos
from photon_amd import bos_density as bd
from photon_amd import piv_correlation as pc
from photon_amd import piv_uncertainty as pu

pytestmark = pytest.mark.gpu

# device vs model, f64 sums of at most 4096 terms in another order: 4.5e-13 of the sum of the absolute terms; the bounds
# keep a factor of 20 over that.  C0, C1 against sqrt(sum A^2 sum B^2), S(0) against T, V against N T, N = 1 + 2 |H_K|.
SUM_RTOL = 1e-11
SIGMA_OWN_RTOL = 1e-6           # sigma against the model's last step on the device's own sums: f32 rounding, ulps of log
SIGMA_MODEL_RTOL = 1e-5         # sigma against the model's


def device_uncertainty(photon, im1, im2, win, step, reach, stats=True):
    import torch
    a, b = torch.from_numpy(np.ascontiguousarray(im1)).cuda(), torch.from_numpy(np.ascontiguousarray(im2)).cuda()
    sigma, flags, st = photon.piv_uncertainty(a.data_ptr(), b.data_ptr(), im1.shape[1], im1.shape[0], win, step, reach, stats=stats)
    torch.cuda.synchronize()
    return sigma.cpu().numpy(), flags.cpu().numpy(), st.cpu().numpy() if stats else None


@pytest.mark.parametrize("case", uc.CASES, ids=uc.case_id)
def test_device_matches_the_model(photon, case):
    shape, win, step, reach = case
    want_sigma, want_flags, want, T = uc.model(case)
    sigma, flags, got = device_uncertainty(photon, *uc.matched_pair(shape), win, step, reach)
    assert got.shape == want.shape and sigma.shape == want_sigma.shape and sigma.dtype == np.float32
    E, N = uc.energies(case)[..., None], uc.n_terms(reach)
    err_c = max(float((np.abs(got[..., k] - want[..., k]) / E).max()) for k in (0, 1))
    err_s = float((np.abs(got[..., 2] - want[..., 2]) / T).max())
    err_v = float((np.abs(got[..., 3] - want[..., 3]) / (N * T)).max())
    own, own_flags = pu.sigma_from_stats(got)
    err_own = float(np.abs(sigma / own - 1.0).max())
    err_model = float(np.abs(sigma / want_sigma - 1.0).max())
    print(f"{uc.case_id(case)}: {flags.size} windows, {int((flags & 32).astype(bool).sum())} with V < 0; |C - model| / E {err_c:.1e}, "
          f"|S00 - model| / T {err_s:.1e}, |V - model| / (N T) {err_v:.1e}; sigma vs own sums {err_own:.1e}, vs model {err_model:.1e}")
    assert err_c <= SUM_RTOL and err_s <= SUM_RTOL and err_v <= SUM_RTOL
    assert np.array_equal(flags, want_flags) and np.array_equal(own_flags, want_flags)
    assert err_own <= SIGMA_OWN_RTOL and err_model <= SIGMA_MODEL_RTOL


def test_two_calls_return_identical_bits_with_and_without_stats(photon):
    im1, im2 = uc.matched_pair((130, 97))
    a = device_uncertainty(photon, im1, im2, 16, 5, 4)
    b = device_uncertainty(photon, im1, im2, 16, 5, 4)
    c = device_uncertainty(photon, im1, im2, 16, 5, 4, stats=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
    assert (a[1] & 32).any()                                # the case holds windows that took the fallback


def test_identical_frames_give_zero_sigma(photon):
    im = uc.matched_pair((97, 130))[0]
    odd = [(win, step, reach) for win, step in ((16, 8), (32, 16), (64, 32)) for reach in (1, 3)]       # every kernel of an odd reach
    for win, step, reach in [(16, 8, 4), (32, 16, 2), (64, 32, 0)] + odd:
        sigma, flags, stats = device_uncertainty(photon, im, im, win, step, reach)
        assert sigma.shape == (*pc.grid_shape(im.shape, win, step), 2), (win, step, reach)
        assert (sigma == 0.0).all() and (flags == 0).all() and (stats[..., 2:] == 0.0).all(), (win, step, reach)


def check_a_constant_window(photon, which, shape, win, step, reach):
    """Window (1, 2) of the grid, and only that one, constant in frame `which`."""
    ims = [im.copy() for im in uc.matched_pair(shape)]
    ims[which][step:step + win, 2 * step:2 * step + win] = 0.37
    sigma, flags, stats = device_uncertainty(photon, *ims, win, step, reach)
    want_sigma, want_flags, _, _ = pu.uncertainty_model(*ims, win, step, reach)
    assert flags[1, 2] == pu.FLAG_FLAT and np.isnan(sigma[1, 2]).all() and np.isnan(stats[1, 2]).all()
    assert int((flags & pu.FLAG_FLAT).astype(bool).sum()) == 1
    assert np.array_equal(flags, want_flags) and np.array_equal(np.isnan(sigma), np.isnan(want_sigma))
    np.testing.assert_allclose(sigma, want_sigma, rtol=SIGMA_MODEL_RTOL)


@pytest.mark.parametrize("which", [0, 1])
def test_a_constant_window_is_flat(photon, which):
    check_a_constant_window(photon, which, (64, 64), 16, 8, 2)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("reach", [1, 3])
@pytest.mark.parametrize("shape,win,step", [((64, 64), 16, 8), ((64, 64), 32, 8), ((130, 192), 64, 32)],
                         ids=["win16", "win32", "win64"])
def test_a_constant_window_is_flat_at_an_odd_reach(photon, shape, win, step, reach, which):
    check_a_constant_window(photon, which, shape, win, step, reach)


def test_refusals_and_the_size_query_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    im = torch.from_numpy(uc.matched_pair((64, 64))[0]).cuda()
    sigma = torch.full((49, 2), -77.0, dtype=torch.float32, device="cuda")
    flags = torch.full((49,), -77, dtype=torch.int32, device="cuda")
    stats = torch.full((49, 8), -77.0, dtype=torch.float64, device="cuda")
    p, s, f, st = (ctypes.c_void_p(t.data_ptr()) for t in (im, sigma, flags, stats))

    def untouched():
        torch.cuda.synchronize()
        return (sigma == -77.0).all().item() and (flags == -77).all().item() and (stats == -77.0).all().item()

    capfd.readouterr()
    for what, args in (("win 24", (p, p, 64, 64, 24, 8, 2, s, f, st)), ("win 0", (p, p, 64, 64, 0, 8, 2, s, f, st)),
                       ("step 0", (p, p, 64, 64, 16, 0, 2, s, f, st)), ("reach -1", (p, p, 64, 64, 16, 8, -1, s, f, st)),
                       ("reach 5", (p, p, 64, 64, 16, 8, 5, s, f, st)), ("narrow image", (p, p, 15, 64, 16, 8, 2, s, f, st)),
                       ("low image", (p, p, 64, 31, 32, 8, 2, s, f, st)), ("null im1", (None, p, 64, 64, 16, 8, 2, s, f, st)),
                       ("null im2", (p, None, 64, 64, 16, 8, 2, s, f, st)), ("sigma without flags", (p, p, 64, 64, 16, 8, 2, s, None, st))):
        rows, cols = ctypes.c_int(-5), ctypes.c_int(-5)
        rc = L.photon_piv_uncertainty(*args, ctypes.byref(rows), ctypes.byref(cols), None)
        err = capfd.readouterr().err
        assert rc == 1, what
        assert len(err.strip().splitlines()) == 1 and "photon: photon_piv_uncertainty:" in err, (what, err)
        assert rows.value == -5 and cols.value == -5 and untouched(), what
    # the size query: the grid, and nothing launched even with flags and stats given
    rows, cols = ctypes.c_int(-5), ctypes.c_int(-5)
    assert L.photon_piv_uncertainty(p, p, 64, 64, 16, 8, 2, None, f, st, ctypes.byref(rows), ctypes.byref(cols), None) == 0
    assert (rows.value, cols.value) == (7, 7) == pc.grid_shape((64, 64), 16, 8) and untouched()
    # an accepted call is silent and fills every window
    assert L.photon_piv_uncertainty(p, p, 64, 64, 16, 8, 2, s, f, st, None, None, None) == 0
    torch.cuda.synchronize()
    assert capfd.readouterr().err == "" and (sigma == 0.0).all().item() and (flags == 0).all().item() and (stats != -77.0).all().item()


# ---- the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy-field", "device-field"])
def test_driver_equals_its_parts_bit_for_bit(photon, as_tensor):
    import torch
    shape, win, step, reach = (97, 130), 32, 16, 2
    im1, im2 = uc.matched_pair(shape)
    r, c = pc.grid_shape(shape, win, step)
    rng = np.random.default_rng(5)
    field = np.zeros((r, c, 3 if as_tensor else 4), np.float32)            # 3: the driver must cut it to the two components
    field[..., :2] = rng.uniform(-1.5, 1.5, (r, c, 2))
    field[1, 2, 0] = np.nan                                                 # reads as (0, 0)
    arg = torch.from_numpy(field).cuda() if as_tensor else field
    sigma, flags, w1, w2 = photon.displacement_uncertainty(im1, im2, arg, win, step, reach, return_warped=True)
    assert sigma.shape == (r, c, 2) and flags.shape == (r, c)
    two = torch.from_numpy(np.ascontiguousarray(field[..., :2])).cuda()
    h, w = shape
    for im, scale, got in ((im1, -0.5, w1), (im2, 0.5, w2)):
        a = torch.from_numpy(im).cuda()
        coef, out = torch.empty_like(a), torch.empty_like(a)
        photon.bspline_coefficients(a.data_ptr(), w, h, coef.data_ptr())
        photon.piv_deform(coef.data_ptr(), w, h, two.data_ptr(), 2, r, c, win, step, scale, out.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out, got) and not torch.equal(out, a)
    s2, f2, _ = photon.piv_uncertainty(w1.data_ptr(), w2.data_ptr(), w, h, win, step, reach)
    torch.cuda.synchronize()
    assert s2.cpu().numpy().tobytes() == sigma.tobytes() and f2.cpu().numpy().tobytes() == flags.tobytes()
    for bad in (field[:-1], field[..., :1]):
        with pytest.raises(ValueError):
            photon.displacement_uncertainty(im1, im2, bad, win, step, reach)


def test_sigma_is_calibrated_on_the_device(photon):
    """The uniform pairs at image noise 0.05: correlate_deform, then displacement_uncertainty, under the bound of the CPU
    tier (measured there with the model: 0.86 / 0.75)."""
    errors, sigmas = [], []
    for seed in uc.CAL_SEEDS:
        im1, im2 = uc.noisy_pair("uniform", seed, 0.05)
        vec, _ = photon.correlate_deform(im1, im2, dc.WIN, dc.STEP, iterations=3)
        sigma, flags = photon.displacement_uncertainty(im1, im2, vec, dc.WIN, dc.STEP, reach=2)
        assert not (flags[1:-1, 1:-1] & (pu.FLAG_FLAT | pu.FLAG_NO_PEAK)).any()
        errors.append(uc.interior_error(vec, "uniform"))
        sigmas.append(sigma[1:-1, 1:-1].reshape(-1, 2).astype(np.float64))
    ratio, cover = uc.calibration(errors, sigmas)
    print(f"uniform, noise 0.05, device: rms sigma / std(error) = {ratio[0]:.3f} (x) {ratio[1]:.3f} (y); |error| <= sigma on "
          f"{100 * cover[0]:.0f} % / {100 * cover[1]:.0f} % of the nodes")
    assert (ratio >= uc.CAL_BOUND[0]).all() and (ratio <= uc.CAL_BOUND[1]).all(), ratio


# ---- the weights in the BOS loop -----------------------------------------------------------------------------------------
def test_reconstruct_with_uncertainty_weights(photon, tmp_path):
    """The rendered blob of the section 6 tests (4-pixel splat): phi with weights="uncertainty" is finite wherever it is with
    "median" and meets the bound the "median" test holds phi to."""
    c1, c2 = bc.blob_calls(photon, str(tmp_path), False)
    im1, im2 = (photon.render(c).reshape(bc.N_PIX, bc.N_PIX).astype(np.float32) for c in (c1, c2))
    args = (photon, im1, im2, c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    med, _, st_med = bd.reconstruct(*args, passes=2, weights="median")
    unc, _, st_unc = bd.reconstruct(*args, passes=2, weights="uncertainty")
    assert st_med["converged"] == 1 and st_unc["converged"] == 1
    e_med = bos.check("median weights, 4-pixel", med, c2, bos.BOUND_CORRELATED)
    assert np.isfinite(unc[np.isfinite(med)]).all()
    e_unc = bos.check("uncertainty weights, 4-pixel", unc, c2, bos.BOUND_CORRELATED)
    print(f"rel L2 error: median weights {e_med:.4f}, uncertainty weights {e_unc:.4f}")
