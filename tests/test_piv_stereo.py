"""Stereo PIV on the host (photon_amd/piv_stereo.py): the camera model, its folding onto a plane, the two dewarp models against
each other, and the reconstruction model against constructions whose answer is known.  No GPU."""
import numpy as np
import pytest

import piv_stereo_cases as cases
from photon_amd import piv_deformation as pd
from photon_amd import piv_stereo as ps


@pytest.mark.parametrize("kind", list(cases.ANGLES))
def test_the_polynomial_fits_a_pinhole_at_thirty_degrees(kind):
    """9 x 9 x 3 target (Z = -1, 0, 1 mm), 300 mm, 5 px/mm: what a cubic leaves of a perspective view stays below 1e-2 px."""
    for (theta, phi), (_, cam, rms, worst) in zip(cases.ANGLES[kind], cases.calibrated(kind)):
        print(f"{kind} theta {theta} phi {phi}: rms {rms:.2e} px, max {worst:.2e} px")
        assert rms <= worst <= 1e-2
        assert cam["cx"].shape == cam["cy"].shape == (19,) and cam["cx"].dtype == np.float64


def test_fit_camera_refuses_a_flat_target():
    target = ps.calibration_target(cases.PLANE, 9, (0.0,))
    with pytest.raises(ValueError, match="terms"):
        ps.fit_camera(target, cases.calibrated("symmetric")[0][0].project(target))


def test_the_jacobian_is_the_derivative_of_the_map():
    """Central differences with h = 1e-4 mm: truncation h^2 / 6 times a third derivative of order 1 px/mm^3 is 2e-9, rounding
    2e-16 x 250 px / h = 5e-10; the bound is 1e-7 px/mm against entries of order 5."""
    cam = cases.cameras("asymmetric")[0]
    P = ps.plane_points(cases.PLANE, [0.0, 3.5, 80.0, 159.0], [0.0, 10.0, 100.25, 191.0]) + np.array([0.0, 0.0, 0.4])
    J, h = ps.jacobian(cam, P), 1e-4
    assert J.shape == (4, 4, 2, 3) and np.abs(J).max() > 1.0
    for axis in range(3):
        d = np.zeros(3)
        d[axis] = h
        num = (ps.map_points(cam, P + d) - ps.map_points(cam, P - d)) / (2 * h)
        assert np.abs(num - J[..., axis]).max() <= 1e-7


@pytest.mark.parametrize("z", [0.0, 0.7])
def test_the_folded_cubics_are_the_camera_on_the_plane(z):
    cam = cases.cameras("asymmetric")[1]
    pl = dict(cases.PLANE, z=z)
    poly, grid = ps.plane_coefficients(cam, pl)
    x, y = ps.folded_points(poly, grid, (pl["height"], pl["width"]))
    want = ps.map_points(cam, ps.plane_points(pl))
    err = max(np.abs(x - want[..., 0]).max(), np.abs(y - want[..., 1]).max())
    print(f"z = {z}: folded against map_points {err:.2e} px")
    assert err <= 1e-12 * max(cases.SENSOR)


def test_the_f32_dewarp_model_against_the_f64_model():
    """The warp's bound of tests/test_piv_deformation_gpu.py: 1e-4 of max |im|.  Measured 1.5e-7: the
    fraction is taken in f64, so what is left is the f32 rounding of coefficients, weights and sums."""
    im = cases.image(cases.SRC, 21, n=2)
    coef = np.stack([pd.bspline_coefficients_model(f) for f in im]).astype(np.float32)
    worst = 0.0
    for out in cases.OUTS:
        for name, (poly, grid) in cases.dewarp_cameras(cases.SRC, out).items():
            got, mask32 = ps.dewarp_model_f32(coef, poly, grid, out)
            want, mask64 = ps.dewarp_model(im, poly, grid, out)
            assert got.dtype == np.float32 and got.shape == want.shape == (2,) + out and np.array_equal(mask32, mask64)
            assert (got[:, mask32 == 1] == 0).all()
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"dewarp_model_f32 against dewarp_model: {worst / np.abs(im).max():.2e} of max |im|")
    assert worst <= 1e-4 * np.abs(im).max()


def test_the_dewarp_cases_cover_what_they_claim():
    for out in cases.OUTS:
        cams = cases.dewarp_cameras(cases.SRC, out)
        masks = {name: ps.outside_mask(poly, grid, out, cases.SRC) for name, (poly, grid) in cams.items()}
        assert not masks["fit"][:-1, :-1].any() and masks["all_outside"].all()
        assert masks["partly_outside"].any() and not masks["partly_outside"].all()
        assert masks["full"].mean() < 0.5
        x, _ = ps.folded_points(*cams["overflow"], out)
        assert masks["overflow"].any() and not masks["overflow"].all() and np.isinf(x).any()
    x, _ = ps.folded_points(*cases.dewarp_cameras(cases.SRC, cases.OUTS[0])["overflow"], cases.OUTS[0])
    assert np.isnan(x).any()
    x, y = ps.folded_points(*cases.dewarp_cameras(cases.SRC, cases.OUTS[0])["rotated"], cases.OUTS[0])
    assert (x[:, 0] != x[:, -1]).sum() == 0 and (y[0] != y[-1]).sum() == 0           # x depends on the row alone, y on the column


def test_the_identity_camera_dewarps_an_image_onto_itself():
    im = cases.image((20, 31), 5)[0]
    coef = pd.bspline_coefficients_model(im)
    got, mask = ps.dewarp_model_f32(coef.astype(np.float32), *ps.plane_coefficients(ps.identity_camera(), ps.plane(0, 0, 1, 0, 31, 20)), (20, 31))
    assert not mask.any() and np.abs(got - im).max() <= 1e-5


# ---- reconstruction ----------------------------------------------------------------------------------------------------------
def _synthesised(delta, cams, pl, extra=None):
    """The two cameras' (dx, dy) [r, c, 2] in f64 that see the world displacement delta [r, c, 3] exactly: J_c delta = J_c[:, :2]
    pitch d_c; extra: per camera an image-space vector [r, c, 2] added to the right-hand side."""
    P = ps.window_centres(pl, cases.WIN, cases.STEP)
    out = []
    for c, cam in enumerate(cams):
        J = ps.jacobian(cam, P)
        rhs = np.einsum("...ij,...j->...i", J, delta) + (0.0 if extra is None else extra[c])
        out.append(np.linalg.solve(J[..., :2], rhs[..., None])[..., 0] / pl["pitch"])
    return out


def _true_delta(pl):
    P = ps.window_centres(pl, cases.WIN, cases.STEP)
    return np.stack([0.5 + 0.01 * P[..., 0], -0.3 + 0.02 * P[..., 1], 0.4 - 0.01 * P[..., 0] * P[..., 1] / 10.0], axis=-1)


@pytest.mark.parametrize("kind", list(cases.ANGLES))
def test_the_reconstruction_returns_a_consistent_displacement_exactly(kind):
    cams, pl = cases.cameras(kind), cases.PLANE
    delta = _true_delta(pl)
    d1, d2 = _synthesised(delta, cams, pl)
    out, flags = ps.reconstruct_model(d1, d2, cams, pl, cases.WIN, cases.STEP)
    assert out.shape == (9, 11, 8) and not flags.any()
    print(f"{kind}: delta off by {np.abs(out[..., :3] - delta).max():.2e}, residual {out[..., 3].max():.2e}, pivot ratio {out[..., 7].min():.3f}")
    assert np.abs(out[..., :3] - delta).max() <= 1e-10 and out[..., 3].max() <= 1e-10
    assert np.isnan(out[..., 4:7]).all() and (out[..., 7] > 0.01).all()


def test_the_residual_is_the_inconsistency_of_the_four_equations():
    """A right-hand side moved by r0 times a unit vector of the null space of A^T leaves delta where it was and has
    residual r0."""
    cams, pl = cases.cameras("asymmetric"), cases.PLANE
    delta, P = _true_delta(pl), ps.window_centres(pl, cases.WIN, cases.STEP)
    A = np.concatenate([ps.jacobian(c, P) for c in cams], axis=-2)                  # [r, c, 4, 3]
    null = np.linalg.svd(A, full_matrices=True)[0][..., :, 3]                       # unit vectors with A^T e = 0
    r0 = 0.37
    d1, d2 = _synthesised(delta, cams, pl, extra=[r0 * null[..., :2], r0 * null[..., 2:]])
    out, _ = ps.reconstruct_model(d1, d2, cams, pl, cases.WIN, cases.STEP)
    assert np.abs(out[..., :3] - delta).max() <= 1e-10 and np.abs(out[..., 3] - r0).max() <= 1e-10


def test_the_propagated_sigmas_against_a_monte_carlo_of_the_linear_map():
    """20 000 samples: the standard deviation of a sample standard deviation is 1 / sqrt(2 N) = 0.5 %; the bound is 3 %."""
    cams, pl = cases.cameras("asymmetric"), ps.centred_plane(32, 32, 0.2)
    rng = np.random.default_rng(31)
    sig = [np.array([[[0.05, 0.08]]]), np.array([[[0.11, 0.03]]])]
    d = [np.array([[[1.0, -2.0]]]), np.array([[[0.5, 0.7]]])]
    out, _ = ps.reconstruct_model(d[0], d[1], cams, pl, 32, 16, sigma1=sig[0], sigma2=sig[1])
    P = ps.window_centres(pl, 32, 16)[0, 0]
    J = [ps.jacobian(c, P) for c in cams]
    A = np.concatenate(J, axis=0)
    n = 20000
    noise = [rng.normal(0.0, 1.0, (n, 2)) * s[0, 0] + v[0, 0] for s, v in zip(sig, d)]
    b = np.concatenate([pl["pitch"] * x @ Jc[:, :2].T for x, Jc in zip(noise, J)], axis=1)      # [n, 4]
    samples = b @ np.linalg.pinv(A).T
    got, want = out[0, 0, 4:7], samples.std(axis=0)
    print(f"sigma model {got}, Monte Carlo {want}")
    assert np.abs(got / want - 1.0).max() <= 0.03
    assert np.abs(samples.mean(axis=0) - out[0, 0, :3]).max() <= 4 * want.max() / np.sqrt(n)


def test_two_identical_cameras_are_degenerate():
    cam, pl = cases.cameras("symmetric")[0], cases.PLANE
    d = np.ones((9, 11, 2))
    out, flags = ps.reconstruct_model(d, d, (cam, cam), pl, cases.WIN, cases.STEP, flags1=np.full((9, 11), 4))
    assert (flags == (4 | ps.FLAG_DEGENERATE)).all() and np.isnan(out).all()


def test_a_vector_that_is_not_finite_keeps_the_pivot_ratio_alone():
    cams, pl = cases.cameras("symmetric"), cases.PLANE
    d1, d2 = np.ones((9, 11, 2)), np.ones((9, 11, 2))
    d2[3, 4, 1] = np.nan
    out, flags = ps.reconstruct_model(d1, d2, cams, pl, cases.WIN, cases.STEP)
    assert flags[3, 4] == ps.FLAG_NOT_FINITE and flags.sum() == ps.FLAG_NOT_FINITE
    assert np.isnan(out[3, 4, :7]).all() and out[3, 4, 7] > 0 and np.isfinite(out[..., :4]).sum() == 4 * (99 - 1)


def test_the_model_chain_measures_three_components():
    """The issue's two conditions on the model alone: the stereo dX is at most 0.2 of what camera 1 alone reads wrong, and
    the median stereo residual is below 0.1 px."""
    for name in cases.ACCURACY:
        rms, alone, median, worst = cases.model_figures(name)
        print(f"{name}: rms dX dY dZ {rms.round(4)} px, camera 1 alone {alone:.3f} px, ratio {rms[0] / alone:.3f}, residual median {median:.3f} "
              f"max {worst:.3f} px")
        assert rms[0] <= 0.2 * alone and median < 0.1
