"""Gradient-field integration on the host (photon_amd/bos_density.py, include/parallel_ray_tracing.h section 6): the
PCG model against a dense least-squares solve, exactness on biquadratic fields, second-order convergence, unreachable
islands, the paraxial conversion and the argument checks.  No GPU needed."""
import math

import numpy as np
import pytest

from bos_density_cases import biquadratic, gaussian_case, random_case
from photon_amd import bos_density as bd


def rel_err(a, b):
    ok = np.isfinite(b)
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), 1e-300)) if ok.any() else 0.0


@pytest.mark.parametrize("seed", range(12))
def test_model_matches_the_direct_solve(seed):
    rng = np.random.default_rng(100 + seed)
    ny, nx = (int(v) for v in rng.integers(2, 41, 2))
    case = random_case(seed, ny, nx, fixed_frac=(None, 0.05, 0.2)[seed % 3])
    if seed == 4:                                            # a single pinned node anchors everything
        case["fixed"] = np.zeros((ny, nx), np.uint8)
        case["fixed"][ny // 2, nx // 2] = 1
    hx, hy = rng.uniform(0.2, 2.0, 2)
    phi, st = bd.integrate_model(**case, hx=hx, hy=hy, tol=1e-12, max_iter=50 * max(nx, ny))
    ref = bd.solve_direct(**case, hx=hx, hy=hy)
    assert np.array_equal(np.isnan(phi), np.isnan(ref))
    assert st["converged"] == 1
    assert rel_err(phi, ref) <= 1e-8, rel_err(phi, ref)
    fixed = case["fixed"] if case["fixed"] is not None else None
    n_fixed = int((fixed != 0).sum()) if fixed is not None else 2 * (nx + ny) - 4
    assert st["unknowns"] + st["unreachable"] == nx * ny - n_fixed


@pytest.mark.parametrize("shape,h", [((7, 9), (1.0, 1.0)), ((30, 41), (0.3, 0.2)), ((64, 17), (2.0, 0.5))])
def test_biquadratic_fields_are_exact_for_any_weights(shape, h):
    ny, nx = shape
    phi, gx, gy = biquadratic(ny, nx, *h)
    w = np.random.default_rng(nx).uniform(0.05, 5.0, shape)
    got, st = bd.integrate_model(gx, gy, w, None, phi, h[0], h[1], tol=1e-14, max_iter=100 * max(shape))
    assert rel_err(got, phi) <= 1e-10, rel_err(got, phi)
    assert st["unreachable"] == 0


def test_gaussian_projection_converges_at_second_order():
    errs = []
    for n in (32, 64, 128):
        P, gx, gy, h = gaussian_case(n)
        phi, st = bd.integrate_model(gx, gy, None, None, P, h, h, tol=1e-11)
        assert st["converged"] == 1
        errs.append(np.linalg.norm(phi - P) / np.linalg.norm(P))
    ratios = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
    assert all(3.5 <= r <= 4.5 for r in ratios), (errs, ratios)


def test_an_island_behind_a_wall_of_zero_weights_is_nan_and_unreachable():
    ny, nx = 20, 24
    P, gx, gy, h = gaussian_case(24)
    P, gx, gy = P[:ny], gx[:ny], gy[:ny]
    w = np.ones((ny, nx))
    w[5:15, 6] = w[5:15, 16] = w[5, 6:17] = w[14, 6:17] = 0.0            # a closed ring of zero weights
    phi, st = bd.integrate_model(gx, gy, w, None, P, h, h, tol=1e-12)
    inside = np.zeros((ny, nx), bool)
    inside[6:14, 7:16] = True
    ring = (w == 0)
    assert np.isnan(phi[inside]).all()
    assert np.isnan(phi[ring]).all()                         # no live edge at all
    assert st["unreachable"] == int(inside.sum() + ring.sum())
    assert np.isfinite(phi[~inside & ~ring]).all()
    ref = bd.solve_direct(gx, gy, w, None, P, h, h)
    assert np.array_equal(np.isnan(ref), np.isnan(phi)) and rel_err(phi, ref) <= 1e-9


def test_fixed_nodes_keep_their_values_and_a_nan_value_anchors_nothing():
    case = random_case(3, 12, 15)
    fixed = np.zeros((12, 15), np.uint8)
    fixed[0, 0] = fixed[11, 14] = 1
    value = np.zeros((12, 15))
    value[0, 0], value[11, 14] = 2.5, np.nan
    phi, st = bd.integrate_model(case["gx"], case["gy"], case["w"], fixed, value, tol=1e-12)
    assert phi[0, 0] == 2.5 and np.isnan(phi[11, 14])
    ref = bd.solve_direct(case["gx"], case["gy"], case["w"], fixed, value)
    assert np.array_equal(np.isnan(ref), np.isnan(phi)) and rel_err(phi, ref) <= 1e-8
    # only the NaN anchor: nothing is reachable
    fixed[0, 0] = 0
    phi, st = bd.integrate_model(case["gx"], case["gy"], case["w"], fixed, value, tol=1e-12)
    assert st["unknowns"] == 0 and st["iterations"] == 0 and st["converged"] == 1
    assert st["unreachable"] == 12 * 15 - 1 and np.isnan(phi).all()


def test_iteration_rules():
    P, gx, gy, h = gaussian_case(40)
    _, st = bd.integrate_model(gx, gy, None, None, P, h, h, tol=0.0, max_iter=13)
    assert st["iterations"] == 13
    _, st = bd.integrate_model(gx, gy, None, None, P, h, h, tol=1e-6)
    assert st["converged"] == 1 and st["iterations"] % bd.CHECK_EVERY == 0 and st["residual"] <= 1e-6
    _, st = bd.integrate_model(np.zeros((9, 9)), np.zeros((9, 9)), tol=1e-8)           # b = 0
    assert st["iterations"] == 0 and st["converged"] == 1 and st["residual"] == 0.0
    phi, st = bd.integrate_model(gx, gy, None, None, P, h, h, tol=1e-3, max_iter=0)
    assert st["iterations"] == 0 and st["residual"] == 1.0 and (phi[1:-1, 1:-1] == 0).all()


def test_the_conversion_reproduces_the_paraxial_relation(tmp_path):
    from conftest import bos_displacement_case
    from photon_amd import scenes
    c1, c2, predicted = bos_displacement_case(str(tmp_path))
    rho, spacing, origin = scenes.read_nrrd(c2.density_grad_filename)
    extent = spacing[2] * (rho.shape[0] - 1)
    rho_grad = (float(rho[0, 0, -1]) - float(rho[0, 0, 0])) / (spacing[0] * (rho.shape[2] - 1))   # per micron along x
    F = bd.displacement_factor(c2, origin[2], extent)
    # forward: d = F dP/dx with P = int (rho - rho_0) dz, dP/dx = rho_grad extent
    assert math.isclose(F * rho_grad * extent, predicted, rel_tol=1e-4), (F * rho_grad * extent, predicted)
    # backward: the predicted shift along +x (to_pixels) is dP/dx; the erf splat's columns run along +x, rows along -y
    gx, gy = bd.gradients_from_displacements(np.array([predicted, 0.0]), c2.camera, F)
    assert math.isclose(gx, rho_grad * extent, rel_tol=1e-4) and gy == 0.0
    cam4 = dict(c2.camera, implement_diffraction=False)
    gx4, _ = bd.gradients_from_displacements(np.array([predicted, 0.0]), cam4, F)
    assert gx4 == -gx
    _, gy = bd.gradients_from_displacements(np.array([0.0, predicted]), c2.camera, F)
    assert math.isclose(gy, -rho_grad * extent, rel_tol=1e-4)


def test_node_geometry_follows_the_splat_axes():
    from photon_amd import scenes
    call = scenes.bos_scene(n_dots=2, points_per_dot=3, n_pixels=256)
    for diffraction, sx in ((False, -1.0), (True, 1.0)):
        call.camera["implement_diffraction"] = diffraction
        target, mid, h = bd.node_geometry((256, 256), 32, 16, call, 300000.0, 66300.0)
        s = (300000.0 + 33150.0) / call.object_distance
        M = call.image_distance / call.object_distance
        assert math.isclose(h, s * 16 * 17.0 / M, rel_tol=1e-12)
        np.testing.assert_allclose(np.diff(mid[0], axis=1), sx * h, rtol=1e-9)
        np.testing.assert_allclose(np.diff(mid[1], axis=0), -h, rtol=1e-9)
        np.testing.assert_allclose(mid[0], s * target[0], rtol=1e-12)
        assert abs(mid[0].mean()) < h and abs(mid[1].mean()) < h                   # the grid is centred on the axis


def test_weights_from_correlation():
    from photon_amd import piv_correlation as pc
    v = np.ones((3, 4, 4))
    v[0, 1, 0] = np.nan
    flags = np.zeros((3, 4), np.int32)
    flags[2, 3] = pc.FLAG_FLAT
    out = np.zeros((3, 4), bool)
    out[1, 2] = True
    w = bd.weights_from_correlation(v, flags, out)
    want = np.ones((3, 4))
    want[0, 1] = want[2, 3] = want[1, 2] = 0.0
    assert np.array_equal(w, want)


def test_chief_ray_projection_of_a_gaussian_blob():
    A, s, L = 2.0, 2500.0, 700000.0
    zc = 333150.0
    target = (np.array([[0.0, 4000.0]]), np.array([[0.0, -3000.0]]))
    P = bd.chief_ray_projection(lambda x, y, z: bd.RHO_0 + A * np.exp(-(x * x + y * y + (z - zc) ** 2) / (2 * s * s)),
                                target, L, (zc - 33150.0, zc + 33150.0))
    assert math.isclose(P[0, 0], bd.gaussian_projection(0.0, A, s), rel_tol=1e-6)
    r2 = (zc / L) ** 2 * (4000.0 ** 2 + 3000.0 ** 2)                                   # the ray crosses z = zc at (zc/L) X_t
    assert math.isclose(P[0, 1], bd.gaussian_projection(r2, A, s), rel_tol=1e-3)


@pytest.mark.parametrize("args", [(1, 5, 1.0, 1.0, 1e-8, 10), (5, 1, 1.0, 1.0, 1e-8, 10), (5, 5, 0.0, 1.0, 1e-8, 10),
                                  (5, 5, 1.0, -1.0, 1e-8, 10), (5, 5, float("nan"), 1.0, 1e-8, 10),
                                  (5, 5, 1.0, float("inf"), 1e-8, 10), (5, 5, 1.0, 1.0, -1e-3, 10),
                                  (5, 5, 1.0, 1.0, float("nan"), 10), (5, 5, 1.0, 1.0, 1e-8, -1),
                                  (50000, 50000, 1.0, 1.0, 1e-8, 10)])
def test_argument_checks(args):
    with pytest.raises(ValueError):
        bd.check_arguments(*args)


def test_argument_checks_accept_the_edges_of_the_range():
    bd.check_arguments(2, 2, 1e-300, 1e300, 0.0, 0)
    phi, st = bd.integrate_model(np.zeros((2, 2)), np.zeros((2, 2)), value=np.arange(4.0).reshape(2, 2), tol=0.0, max_iter=0)
    assert np.array_equal(phi, np.arange(4.0).reshape(2, 2)) and st["unknowns"] == 0
