"""photon_amd/piv_pairs.py without a GPU: the host model of the PIV field against the CPU oracle, the advection against
exact solutions, the grid fillers against their closed forms, and image_displacements on hand-made records."""
import math

import numpy as np
import pytest

from photon_amd import piv_pairs as pp

BOX_LO, BOX_HI = (-3.0e4, -2.0e4, -7.5e3), (3.0e4, 2.0e4, 7.5e3)
Z_OBJ = 823668.35


def ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def test_philox_known_answer():
    """Random123's known-answer vector for Philox4x32-10 with counter 0 and key 0."""
    words = pp.philox4x32_10(0, np.zeros(1, np.uint64), draw=0, stream=0)
    assert [int(w[0]) for w in words] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("with_cdf", [False, True])
def test_piv_field_is_the_oracles_field(oracle, with_cdf):
    n = 50_001
    cdf = np.cumsum(np.full(27, 1.0 / 27.0)) if with_cdf else None
    got = pp.piv_field(1234, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, cdf)
    want = oracle.sources_piv(1234, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, cdf)
    for key in ("x", "y", "z", "diameter_index"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    # the oracle evaluates photon_det_exp, the model numpy's exp
    assert ulps(got["radiance"], want["radiance"]).max() <= pp.RADIANCE_ULP
    assert np.array_equal(got["world"][:, 0].astype(np.float32), got["x"])
    if with_cdf:
        assert len(np.unique(got["diameter_index"])) == 27
    prefix = pp.piv_field(1234, 1000, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, cdf)          # counter-based
    assert np.array_equal(prefix["world"], got["world"][:1000])


def _assert_same_frame(a, b):
    for key in ("x", "y", "z", "radiance", "diameter_index", "world"):
        assert np.array_equal(a[key], b[key]), key


def test_advect_by_zero_time_or_through_zero_field_is_frame_one():
    n = 3000
    frame1 = pp.piv_field(7, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0)
    vortex = pp.lamb_oseen_vortex(5e6, 4e3, (0.0, 0.0), (-4e4, -4e4, -8e3), (4e4, 4e4, 8e3), 33)
    _assert_same_frame(pp.advect(7, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, flow=vortex, t=0.0), frame1)
    _assert_same_frame(pp.advect(7, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, flow=None, t=0.0, steps=3), frame1)
    still = pp.uniform_flow((0.0, 0.0, 0.0), (-4e4, -4e4, -8e3), (4e4, 4e4, 8e3), 5)
    _assert_same_frame(pp.advect(7, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, flow=still, t=12.5, steps=7), frame1)
    for bad in (dict(steps=0, flow=vortex, t=1.0), dict(flow=vortex, t=float("nan")), dict(flow=None, t=1.0)):
        with pytest.raises(ValueError):
            pp.advect(7, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, **bad)


def test_uniform_flow_moves_every_particle_by_u_t():
    n, t, steps = 20_000, 2.5, 16
    vel = (120.5, -73.25, 9.0)
    flow = pp.uniform_flow(vel, (-1e3, -1e3, -1e3), (1e3, 1e3, 1e3), 3)   # particles outside the grid: clamped to its edge
    start = pp.piv_field(11, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0)["world"]
    got = pp.advect(11, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0, flow=flow, t=t, steps=steps)
    want = start + np.asarray(vel) * t
    # one rounding per step of the sum p + (h/6) (6 u), plus the few roundings of (h/6) (6 u) itself
    h = t / steps
    eps = np.finfo(np.float64).eps
    tol = steps * (np.spacing(np.abs(want).max(axis=0) + np.abs(vel) * t) + 4 * eps * np.abs(vel) * h) + np.spacing(np.abs(want))
    assert (np.abs(got["world"] - want) <= tol).all()
    assert (got["world"] != start).all()
    sheet = pp.piv_field(11, n, BOX_LO, BOX_HI, Z_OBJ, 730.0, 500.0)
    assert np.array_equal(got["diameter_index"], sheet["diameter_index"])


def test_solid_body_rotation_matches_the_exact_rotation():
    n, omega, t, steps = 20_000, 0.4, 2.5, 8                    # omega t = 1 rad in 8 steps: omega h = 1/8
    cx, cy = 1500.0, -800.0
    lo, hi = (-2.5e4 + cx, -2.5e4 + cy, -8e3), (2.5e4 + cx, 2.5e4 + cy, 8e3)   # every orbit stays inside the grid
    box_lo, box_hi = (-1.5e4, -1.5e4, -7.5e3), (1.5e4, 1.5e4, 7.5e3)
    flow = pp.solid_body_rotation(omega, lo, hi, 9, centre=(cx, cy))
    start = pp.piv_field(5, n, box_lo, box_hi, Z_OBJ, 730.0, 500.0)["world"]
    got = pp.advect(5, n, box_lo, box_hi, Z_OBJ, 730.0, 500.0, flow=flow, t=t, steps=steps)["world"]
    c, s = math.cos(omega * t), math.sin(omega * t)
    dx, dy = start[:, 0] - cx, start[:, 1] - cy
    exact = np.stack([cx + c * dx - s * dy, cy + s * dx + c * dy, start[:, 2]], 1)
    r = np.hypot(dx, dy)
    # RK4 on x' = A x with A a rotation generator: one step is the degree-4 Taylor polynomial of exp(hA), off by at most
    # (omega h)^5 / 5! of |x - c| per step, and a step never amplifies (|R(i omega h)| <= 1): steps (omega h)^5 / 120 r.
    wh = omega * t / steps
    truncation = steps * wh ** 5 / 120.0 * r
    # the nodes hold the field in f32: the sampled velocity is off by <= 2^-24 of the largest node speed, for the time t
    f32 = t * omega * math.hypot(2.5e4, 2.5e4) * 2.0 ** -24 * 2
    err = np.hypot(got[:, 0] - exact[:, 0], got[:, 1] - exact[:, 1])
    assert (err <= truncation + f32 + 1e-9).all(), (err - truncation - f32).max()
    assert err.max() > 0.25 * truncation.max()                  # the bound is the RK4 error, not slack (measured ~0.8 of it)
    assert np.array_equal(got[:, 2], start[:, 2])                # w = 0: Z is untouched


def test_lamb_oseen_vortex_at_the_nodes():
    gamma, rc, centre = 4.0e6, 3.0e3, (1200.0, -700.0)
    u, v, w, spacing, origin = pp.lamb_oseen_vortex(gamma, rc, centre, (-2e4, -2e4, -5e3), (2e4, 2e4, 5e3), (41, 33, 3))
    assert u.shape == (3, 33, 41) and u.dtype == np.float32 and not w.any()
    x = origin[0] + spacing[0] * np.arange(41)
    y = origin[1] + spacing[1] * np.arange(33)
    X, Y = np.meshgrid(x, y)
    r = np.hypot(X - centre[0], Y - centre[1])
    theta = np.arctan2(Y - centre[1], X - centre[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        ut = np.where(r > 0, gamma / (2 * np.pi * r) * (1 - np.exp(-r ** 2 / rc ** 2)), 0.0)
    peak = pp.lamb_oseen_peak_speed(gamma, rc)
    for k in range(3):
        np.testing.assert_allclose(u[k], -ut * np.sin(theta), rtol=0, atol=1e-6 * peak)
        np.testing.assert_allclose(v[k], ut * np.cos(theta), rtol=0, atol=1e-6 * peak)
    rr = np.linspace(0.01, 5, 20001) * rc
    assert abs(peak - (gamma / (2 * np.pi * rr) * (1 - np.exp(-rr ** 2 / rc ** 2))).max()) < 1e-6 * peak


def test_sample_flow_reproduces_an_affine_field_and_clamps_to_the_edge():
    flow = pp.solid_body_rotation(0.25, (-1e3, -1e3, 0.0), (1e3, 1e3, 50.0), (5, 3, 2))
    pts = np.array([[10.0, 20.0, 5.0], [-999.0, 700.0, 49.0], [5e3, 0.0, 25.0], [0.0, -4e3, -100.0]])
    got = pp.sample_flow(flow, pts)
    want = np.stack([-0.25 * np.clip(pts[:, 1], -1e3, 1e3), 0.25 * np.clip(pts[:, 0], -1e3, 1e3), 0 * pts[:, 0]], 1)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)


def test_image_displacements_give_nan_for_a_particle_in_one_frame_only():
    cam = dict(pixel_pitch=17.0, x_pixel_number=1024, y_pixel_number=1024)
    rps = 10

    def rec(n, x, y):
        return [n, n * x, n * y, 0.0, 0.0, 0.0, 0.0, n * (x * x + y * y)]
    r1 = np.array([rec(10, 100.0, -50.0), rec(0, 0, 0), rec(4, 300.0, 300.0), rec(0, 0, 0)])
    r2 = np.array([rec(7, 134.0, -84.0), rec(5, 1.0, 1.0), rec(0, 0, 0), rec(0, 0, 0)])
    d = pp.image_displacements(r1, r2, cam, rps)
    assert d.shape == (4, 2)
    np.testing.assert_allclose(d[0], [34.0 / 17.0, -34.0 / 17.0], rtol=1e-12)
    assert np.isnan(d[1:]).all()
