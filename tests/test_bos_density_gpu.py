"""photon_integrate_gradient on the GPU (include/parallel_ray_tracing.h, section 6): the device against the f64 host model
of photon_amd/bos_density.py, bit-identical repeats, the refusals, exact biquadratic fields, and the end-to-end BOS loop:
an off-centre Gaussian blob rendered, its dot shifts measured and integrated, against the blob's chief-ray projection."""
import ctypes

import numpy as np
import pytest

import bos_density_cases as bc
from photon_amd import bos_density as bd
from photon_amd import deflections as dfl
from photon_amd import piv_correlation as pc
from photon_amd.library import photon_integrate_stats_t

pytestmark = pytest.mark.gpu

# device vs model with tol = 0 and a fixed iteration count: the two differ only in the order of the dot products' sums.
# Measured on MI355X: at most 6.5e-15 of max |phi| over these cases (193 x 257, 300 iterations); the bound keeps 150x.
PARITY_RTOL = 1e-12


def scale(a):
    return max(float(np.nanmax(np.abs(a))), 1e-300) if np.isfinite(a).any() else 1.0


CASES = [  # (name, ny, nx, case kwargs, hx, hy, max_iter)
    ("2x2", 2, 2, dict(fixed_frac=None), 1.0, 1.0, 8),
    ("one_unknown", 3, 3, dict(fixed_frac=None, nan_frac=0.0, zero_frac=0.0), 0.5, 2.0, 8),
    ("193x257", 193, 257, dict(fixed_frac=None), 0.7, 1.1, 300),
    ("random_fixed", 61, 47, dict(fixed_frac=0.02), 1.0, 0.8, 200),
    ("dense_fixed_nan", 40, 90, dict(fixed_frac=0.3, nan_frac=0.2, zero_frac=0.2), 1.3, 0.4, 120),
    ("1024sq", 1024, 1024, dict(fixed_frac=None, nan_frac=0.01, zero_frac=0.01), 1.0, 1.0, 40),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_matches_the_host_model(photon, case):
    name, ny, nx, kw, hx, hy, max_iter = case
    c = bc.random_case(len(name) + ny, ny, nx, **kw)
    if name == "dense_fixed_nan":
        c["value"][np.random.default_rng(1).random((ny, nx)) < 0.05] = np.nan
    want, ws = bd.integrate_model(**c, hx=hx, hy=hy, tol=0.0, max_iter=max_iter)
    got, gs = photon.integrate_gradient(**c, hx=hx, hy=hy, tol=0.0, max_iter=max_iter)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for k in ("iterations", "converged", "unknowns", "unreachable"):
        assert gs[k] == ws[k], (k, gs, ws)
    err = float(np.nanmax(np.abs(got - want))) / scale(want) if np.isfinite(want).any() else 0.0
    print(f"{name}: {gs['unknowns']} unknowns, {gs['unreachable']} unreachable, {gs['iterations']} iterations, "
          f"max |device - model| / max |phi| = {err:.2e}")
    assert err <= PARITY_RTOL, err
    np.testing.assert_allclose(gs["residual"], ws["residual"], rtol=1e-6, atol=1e-14)


@pytest.mark.parametrize("n", [64, 256])
def test_iteration_counts_agree_within_one_check(photon, n):
    P, gx, gy, h = bc.gaussian_case(n)
    want, ws = bd.integrate_model(gx, gy, None, None, P, h, h, tol=1e-8)
    got, gs = photon.integrate_gradient(gx, gy, None, None, P, h, h, tol=1e-8)
    print(f"{n}^2: device {gs['iterations']} iterations, model {ws['iterations']}; residual {gs['residual']:.2e}")
    assert gs["converged"] == 1 and ws["converged"] == 1
    assert abs(gs["iterations"] - ws["iterations"]) <= bd.CHECK_EVERY
    assert np.abs(got - want).max() <= 1e-6 * np.abs(P).max()


def test_two_calls_return_identical_bits(photon):
    c = bc.random_case(7, 300, 420, fixed_frac=0.01)
    a, sa = photon.integrate_gradient(**c, tol=1e-9)
    b, sb = photon.integrate_gradient(**c, tol=1e-9)
    assert a.tobytes() == b.tobytes() and sa == sb


@pytest.mark.parametrize("shape,h", [((9, 7), (1.0, 1.0)), ((130, 170), (0.05, 0.04))])
def test_biquadratic_fields_are_exact_on_the_device(photon, shape, h):
    phi, gx, gy = bc.biquadratic(*shape, *h)
    w = np.random.default_rng(3).uniform(0.05, 5.0, shape)
    got, st = photon.integrate_gradient(gx, gy, w, None, phi, h[0], h[1], tol=1e-14, max_iter=100 * max(shape))
    err = float(np.abs(got - phi).max() / np.abs(phi).max())
    print(f"biquadratic {shape}: {st['iterations']} iterations, rel err {err:.2e}")
    assert err <= 1e-10, err


def test_refusals_print_one_line_and_write_nothing(photon, capfd):
    import torch
    L = photon.lib
    g = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    out = torch.full((16, 16), 7.0, dtype=torch.float64, device="cuda")
    p, o = ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(out.data_ptr())
    nan, inf = float("nan"), float("inf")
    capfd.readouterr()
    for what, args in (("nx 1", (p, p, 1, 16, 1.0, 1.0, 1e-8, 10, o)), ("ny 1", (p, p, 16, 1, 1.0, 1.0, 1e-8, 10, o)),
                       ("too many nodes", (p, p, 50000, 50000, 1.0, 1.0, 1e-8, 10, o)),
                       ("hx 0", (p, p, 16, 16, 0.0, 1.0, 1e-8, 10, o)), ("hy < 0", (p, p, 16, 16, 1.0, -1.0, 1e-8, 10, o)),
                       ("hx nan", (p, p, 16, 16, nan, 1.0, 1e-8, 10, o)), ("hy inf", (p, p, 16, 16, 1.0, inf, 1e-8, 10, o)),
                       ("tol < 0", (p, p, 16, 16, 1.0, 1.0, -1.0, 10, o)), ("tol nan", (p, p, 16, 16, 1.0, 1.0, nan, 10, o)),
                       ("max_iter < 0", (p, p, 16, 16, 1.0, 1.0, 1e-8, -1, o)), ("null gx", (None, p, 16, 16, 1.0, 1.0, 1e-8, 10, o)),
                       ("null gy", (p, None, 16, 16, 1.0, 1.0, 1e-8, 10, o)), ("null phi", (p, p, 16, 16, 1.0, 1.0, 1e-8, 10, None))):
        gx, gy, nx, ny, hx, hy, tol, it, phi = args
        st = photon_integrate_stats_t(-5, -5, -5, -5, -5.0)
        rc = L.photon_integrate_gradient(gx, gy, None, None, None, nx, ny, hx, hy, tol, it, phi, ctypes.byref(st), None)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert rc == 1, what
        assert len(err.strip().splitlines()) == 1 and "photon: photon_integrate_gradient:" in err, (what, err)
        assert list(st.as_dict().values()) == [-5, -5, -5, -5, -5.0], what
        assert (out == 7.0).all().item(), what
    phi, st = photon.integrate_gradient(np.zeros((16, 16)), np.zeros((16, 16)))          # an accepted call is silent
    assert capfd.readouterr().err == "" and st["iterations"] == 0 and (phi == 0).all()


def test_raw_pointer_form(photon):
    import torch
    P, gx, gy, h = bc.gaussian_case(48)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (("gx", gx), ("gy", gy), ("value", P))}
    fixed = torch.zeros((48, 48), dtype=torch.uint8, device="cuda")
    fixed[0, :] = fixed[-1, :] = fixed[:, 0] = fixed[:, -1] = 1
    phi = torch.empty((48, 48), dtype=torch.float64, device="cuda")
    st = photon.integrate_gradient_ptr(d["gx"].data_ptr(), d["gy"].data_ptr(), 48, 48, phi.data_ptr(), d_fixed_ptr=fixed.data_ptr(),
                                       d_value_ptr=d["value"].data_ptr(), hx=h, hy=h, tol=1e-10)
    want, ws = bd.integrate_model(gx, gy, None, None, P, h, h, tol=1e-10)
    assert st["converged"] == 1 and abs(st["iterations"] - ws["iterations"]) <= bd.CHECK_EVERY
    assert np.abs(phi.cpu().numpy() - want).max() <= 1e-8 * np.abs(P).max()


# ---- end to end: a rendered BOS pair of an off-centre blob --------------------------------------------------------------
# Bounds on the relative L2 error over the nodes above 10 % of the peak.  Measured on MI355X:
# 0.034 from the true shifts and 0.033 from a two-pass correlation, both splats; the bounds keep about 1.5x.
BOUND_TRUE_SHIFTS = 0.05
BOUND_CORRELATED = 0.05
MAX_HOLES = 0.1                 # share of those nodes a rejected vector may leave NaN


@pytest.fixture(scope="module")
def blob_pairs(photon, tmp_path_factory):
    """Both splats: (call_with, im1, im2, records 1, records 2) per diffraction setting."""
    wd = str(tmp_path_factory.mktemp("blob"))
    out = {}
    for diffraction in (False, True):
        c1, c2 = bc.blob_calls(photon, wd, diffraction)
        im1, r1 = photon.render_moments(c1)
        im2, r2 = photon.render_moments(c2)
        out[diffraction] = (c2, im1.reshape(bc.N_PIX, bc.N_PIX).astype(np.float32), im2.reshape(bc.N_PIX, bc.N_PIX).astype(np.float32),
                            r1, r2)
    return out


def check(name, phi, call, bound):
    P, mid, h = bc.truth(call)
    rel, off, holes = bc.errors(phi, P, mid, h)
    print(f"{name}: rel L2 error {rel:.4f} (bound {bound}), argmax offset ({off[0]:+.2f}, {off[1]:+.2f}) grid steps, "
          f"{100 * holes:.1f} % of the nodes NaN")
    assert abs(off[0]) <= 1.0 and abs(off[1]) <= 1.0, off
    assert holes <= MAX_HOLES, holes
    assert rel <= bound, rel
    return rel


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_true_shifts_integrate_to_the_projection(photon, blob_pairs, diffraction):
    call, im1, im2, r1, r2 = blob_pairs[diffraction]
    d = dfl.dot_deflections(r1, r2, call.camera, call.lightray_number_per_particle, group=bc.DOT_POINTS)
    mean, _ = pc.window_truth(pc.image_positions(d.pos1, call.camera), -d.d_pos, (bc.N_PIX, bc.N_PIX), bc.WIN, bc.STEP, 3)
    F = bd.displacement_factor(call, bc.ORIGIN_Z, bc.EXTENT)
    gx, gy = bd.gradients_from_displacements(mean, call.camera, F)
    _, _, h = bd.node_geometry((bc.N_PIX, bc.N_PIX), bc.WIN, bc.STEP, call, bc.ORIGIN_Z, bc.EXTENT)
    w = np.isfinite(mean).all(axis=-1).astype(np.float64)
    assert w.mean() > 0.95
    phi, st = photon.integrate_gradient(gx, gy, w, hx=h, hy=h)
    assert st["converged"] == 1
    check(f"true shifts, {'erf' if diffraction else '4-pixel'}", phi, call, BOUND_TRUE_SHIFTS)


@pytest.mark.parametrize("diffraction", [False, True], ids=["4-pixel", "erf"])
def test_correlated_pair_integrates_to_the_projection(photon, blob_pairs, diffraction):
    call, im1, im2, _, _ = blob_pairs[diffraction]
    phi, mid, st = bd.reconstruct(photon, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, passes=2)
    assert st["converged"] == 1
    check(f"correlated, {'erf' if diffraction else '4-pixel'}", phi, call, BOUND_CORRELATED)


def test_median_test_weights_reject_outliers(photon, blob_pairs):
    call, im1, im2, _, _ = blob_pairs[False]
    vectors, flags = photon.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    args = ((bc.N_PIX, bc.N_PIX), call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    clean, _, _ = bd.integrate_vectors(photon, vectors, flags, *args, weights="median")
    rng = np.random.default_rng(5)
    bad = rng.random(flags.shape) < 0.05
    noisy = vectors.copy()
    noisy[bad, :2] = rng.uniform(-6.0, 6.0, (int(bad.sum()), 2))
    med, _, _ = bd.integrate_vectors(photon, noisy, flags, *args, weights="median")
    unit, _, _ = bd.integrate_vectors(photon, noisy, flags, *args, weights="unit")
    P, mid, h = bc.truth(call)
    e_clean, _, _ = bc.errors(clean, P, mid, h)
    e_med, off, holes = bc.errors(med, P, mid, h)
    e_unit, _, unit_holes = bc.errors(unit, P, mid, h)
    print(f"{int(bad.sum())} outliers: rel L2 error clean {e_clean:.4f}, median-test weights {e_med:.4f} "
          f"({100 * holes:.1f} % NaN), unit weights {e_unit:.4f}")
    assert unit_holes == 0.0 and holes <= MAX_HOLES
    assert e_med <= e_unit
    assert e_med <= max(1.5 * e_clean, e_clean + 0.02), (e_med, e_clean)
    assert abs(off[0]) <= 1.0 and abs(off[1]) <= 1.0, off
