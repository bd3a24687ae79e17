"""Multigrid window refinement, CPU tier: the host models of photon_amd/piv_multigrid.py -- the f32 regrid against its
independent f64 definition and against its properties, the argument rules, and the driver's model against
correlate_deform_model and against analytic truth."""
import numpy as np
import pytest

import piv_multigrid_cases as mc
from photon_amd import piv_correlation as pc
from photon_amd import piv_deformation as pd
from photon_amd import piv_multigrid as pm


# ---- 1. regrid_model against regrid_model_f64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.REGRID_CASES + mc.THIN_CASES, ids=mc.case_id)
def test_regrid_model_matches_the_f64_definition(case):
    shape, src, dst = case
    field = mc.random_field(shape, src, seed=shape[0] + src[1] + dst[1])
    got, want = pm.regrid_model(field, shape, src, dst), pm.regrid_model_f64(field, shape, src, dst)
    assert got.dtype == np.float32 and got.shape == (*pc.grid_shape(shape, *dst), 2) == want.shape
    err = float(np.abs(got - want).max())
    print(f"regrid {mc.case_id(case)}: max |f32 - f64| = {err:.2e} px (bound {mc.BOUND:.2e})")
    assert err <= mc.BOUND


# ---- 2. properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("grid", [(64, 32), (32, 16), (16, 8), (16, 5), (32, 7)], ids=lambda g: f"{g[0]}-{g[1]}")
def test_the_same_grid_returns_the_field(shape, grid):
    field = mc.random_field(shape, grid, seed=7, stride=4)
    assert np.array_equal(pm.regrid_model(field, shape, grid, grid), field[..., :2])


@pytest.mark.parametrize("case", mc.REGRID_CASES + mc.THIN_CASES, ids=mc.case_id)
def test_a_constant_field_stays_constant_bit_for_bit(case):
    shape, src, dst = case
    value = np.array([7.3, -4.6], np.float32)
    field = np.broadcast_to(value, (*pc.grid_shape(shape, *src), 2))
    got = pm.regrid_model(field, shape, src, dst)
    assert got.tobytes() == np.broadcast_to(value, got.shape).astype(np.float32).tobytes()


@pytest.mark.parametrize("case", mc.REGRID_CASES, ids=mc.case_id)
def test_a_linear_field_is_reproduced_inside_the_hull_and_clamped_outside(case):
    """Linear in the centre coordinates with dyadic slopes, so that every source node is an f32 and |v| <= M on these images:
    bilinear interpolation reproduces it inside the hull of the source centres (within the f32 bound); a destination centre
    outside takes the value at the nearest edge of the hull."""
    shape, src, dst = case

    def linear(r, q):
        r, q = np.meshgrid(r, q, indexing="ij")
        return np.stack([(q - r) / 16.0, (r + q) / 32.0 - 4.0], axis=-1)

    (sr, sq), (dr, dq) = mc.centres(shape, src), mc.centres(shape, dst)
    nodes = linear(sr, sq)
    assert np.array_equal(nodes.astype(np.float32), nodes) and np.abs(nodes).max() <= mc.M
    got = pm.regrid_model(nodes.astype(np.float32), shape, src, dst)
    assert np.abs(got - linear(np.clip(dr, sr[0], sr[-1]), np.clip(dq, sq[0], sq[-1]))).max() <= mc.BOUND
    if src == (64, 32) and dst == (16, 8):
        assert (dr[:3] < sr[0]).all() and dr[3] == sr[0]        # centres 7.5, 15.5, 23.5 lie before the first source centre, 31.5
        assert np.array_equal(got[:3], np.broadcast_to(got[3], got[:3].shape))
        assert np.array_equal(got[:, :3], np.broadcast_to(got[:, 3:4], got[:, :3].shape))


def test_nodes_that_are_not_finite_read_as_zeros():
    shape, src, dst = (200, 136), (32, 16), (16, 8)
    field = mc.random_field(shape, src, seed=3, stride=4, bad=0.15)
    bad = ~np.isfinite(field[..., :2]).all(axis=-1)
    assert bad.sum() >= 5
    clean = field.copy()
    clean[bad, :2] = 0.0
    got = pm.regrid_model(field, shape, src, dst)
    assert np.isfinite(got).all() and got.tobytes() == pm.regrid_model(clean, shape, src, dst).tobytes()
    assert np.abs(got - pm.regrid_model_f64(field, shape, src, dst)).max() <= mc.BOUND


def test_a_one_node_source_fills_the_destination():
    field = np.array([[[3.25, -1.5, np.nan, 9.0]]], np.float32)
    for dst in ((16, 8), (32, 16), (64, 64), (16, 5)):
        got = pm.regrid_model(field, (64, 64), (64, 32), dst)
        assert got.shape == (*pc.grid_shape((64, 64), *dst), 2) and (got == field[0, 0, :2]).all()


def test_regrid_model_refuses_what_the_device_refuses():
    shape = (97, 130)
    field = np.zeros((*pc.grid_shape(shape, 32, 16), 2), np.float32)
    for args in ((field, shape, (24, 16), (16, 8)),                                 # a bad win
                 (field, shape, (32, 16), (16, 0)),                                 # a step of 0
                 (field[:-1], shape, (32, 16), (16, 8)),                            # not the source grid
                 (field[..., :1], shape, (32, 16), (16, 8)),                        # one component
                 (np.zeros((1, 1, 2), np.float32), (40, 40), (32, 16), (64, 32)),   # an image smaller than a window
                 (np.zeros((1, 1, 2), np.float32), (64, 2 ** 22 + 1), (64, 2 ** 23), (64, 2 ** 23))):   # a side above 2^22
        for model in (pm.regrid_model, pm.regrid_model_f64):
            with pytest.raises(ValueError):
                model(*args)


# ---- 3. check_schedule -----------------------------------------------------------------------------------------------------
OK = dict(shape=(192, 192), schedule=mc.SCHEDULE, iterations=mc.ITERATIONS, radius=24, residual_radius=4, method="direct")
REFUSED = [("empty schedule", dict(schedule=(), iterations=())), ("lengths differ", dict(iterations=(1, 1))),
           ("no iteration on a later level", dict(iterations=(1, 0, 2))), ("negative iterations on level 0", dict(iterations=(-1, 1, 2))),
           ("radius beyond win / 2", dict(radius=33)), ("radius 0", dict(radius=0)),
           ("phase radius win / 2 on a later pass", dict(method="phase", radius=None, residual_radius=8)),
           ("phase radius beyond win / 2 - 1", dict(method="phase", radius=33)),
           ("residual radius beyond the smallest window's", dict(residual_radius=9)), ("residual radius 0", dict(residual_radius=0)),
           ("image smaller than the largest window", dict(shape=(192, 60))),
           ("image smaller than a later window", dict(shape=(20, 192), schedule=((16, 8), (32, 16)), iterations=(1, 1), radius=8)),
           ("bad win", dict(schedule=((64, 32), (24, 12), (16, 8)))), ("step 0", dict(schedule=((64, 32), (32, 0), (16, 8)))),
           ("unknown method", dict(method="fft"))]


@pytest.mark.parametrize("what,change", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_check_schedule_refuses(what, change):
    with pytest.raises(ValueError):
        pm.check_schedule(**{**OK, **change})


def test_check_schedule_accepts_any_sequence_of_valid_levels():
    assert pm.check_schedule(**OK) == (mc.SCHEDULE, mc.ITERATIONS)
    assert pm.check_schedule(**{**OK, "method": "phase", "radius": None}) == (mc.SCHEDULE, mc.ITERATIONS)
    # lists, levels that do not halve, a change of step alone, a coarser level after a finer one, no iteration on level 0
    got = pm.check_schedule((192, 192), [[32, 16], [32, 8], [16, 5], [64, 7]], [0, 1, 3, 1], None, 4, "direct")
    assert got == (((32, 16), (32, 8), (16, 5), (64, 7)), (0, 1, 3, 1))
    assert pm.check_schedule((64, 64), ((64, 64),), (0,), 32, 99, "direct") == (((64, 64),), (0,))     # no iteration: no residual radius


# ---- 4. correlate_multigrid_model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", mc.METHODS)
def test_a_one_level_schedule_is_correlate_deform_model(method):
    im1, im2 = (im[:128, :160] for im in mc.pair(2))
    for win, step, iterations, smooth in ((64, 32, 2, True), (32, 16, 0, True), (64, 24, 1, False)):
        radius = None if method == "phase" else win // 2
        want = pd.correlate_deform_model(im1, im2, win, step, radius, iterations=iterations, smooth=smooth, method=method, history=True)
        got = pm.correlate_multigrid_model(im1, im2, ((win, step),), (iterations,), radius=radius, smooth=smooth, method=method, history=True)
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
        assert len(got[2]) == len(want[2]) == 1 + iterations and all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))


def test_history_holds_every_field_on_its_level_s_grid():
    im1, im2 = mc.pair(1)
    schedule, iterations = ((64, 32), (32, 16), (32, 8), (16, 8)), (0, 2, 1, 2)
    vectors, status, fields = pm.correlate_multigrid_model(im1, im2, schedule, iterations, radius=24, history=True)
    want = [schedule[0]] + [g for g, n in zip(schedule, iterations) for _ in range(n)]
    assert [f.shape for f in fields] == [(*pc.grid_shape(mc.SHAPE, *g), 2) for g in want]
    assert all(f.dtype == np.float32 for f in fields)
    assert vectors.shape == (*pc.grid_shape(mc.SHAPE, 16, 8), 4) and status.shape == vectors.shape[:2]
    assert np.array_equal(vectors[..., :2], fields[-1])


# ---- 5. accuracy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("seed", mc.SEEDS)
def test_multigrid_halves_the_error_of_the_32_pixel_grid(seed, method):
    """Halving the window twice at least halves the gradient error: interior RMS on the final 16 / 8 grid against that of
    correlate_deform_model(32, 16, iterations=3), code the library had before.  Measured, seeds 1 / 2 / 3:
    direct 0.115 / 0.130 / 0.129 px against 0.470 / 0.451 / 0.593 px; phase 0.055 / 0.061 / 0.057 px against 11.0 / 14.1 /
    14.7 px (the phase baseline's radius is 15 and the x component of the shift reaches 20 px: it fails outright)."""
    vectors, status = mc.model_multigrid(seed, method)
    rms, base = mc.interior_rms(vectors, mc.FINAL), mc.interior_rms(mc.model_baseline(seed, method)[0], (32, 16))
    share = mc.replaced_share(status)
    print(f"{method} seed {seed}: multigrid {rms:.4f} px on {status.shape[0]} x {status.shape[1]} nodes, {100 * share:.1f} % replaced; "
          f"correlate_deform_model(32, 16, iterations=3) {base:.4f} px; ratio {rms / base:.3f}")
    assert vectors.shape == (*pc.grid_shape(mc.SHAPE, *mc.FINAL), 4)
    assert rms <= 0.5 * base
    assert share <= 0.05


def test_the_small_window_alone_cannot_find_the_shift():
    """Why the case needs the feature: |uniform shift| = 16.3 px, the radius of a 16-pixel window is 8."""
    vectors, _ = pd.correlate_deform_model(*mc.pair(1), 16, 8, 8, iterations=3)
    rms = mc.interior_rms(vectors, (16, 8))
    print(f"correlate_deform_model(16, 8, 8, iterations=3), seed 1: {rms:.2f} px")
    assert rms > 5.0
