"""MART particle volumes without a GPU (photon_amd/piv_mart.py): the exact re-projection, the pairing of gather and scatter
(a volume's own images leave it unchanged, bit for bit), zeros, unseen and masked voxels, the threshold, the host's
decisions, the f32 model against the f64 one, and the accuracy of the model chain on piv_mart.CASES."""
import numpy as np
import pytest

import piv_mart_cases as cases
from photon_amd import piv_correlation as pc
from photon_amd import piv_mart as pm
from photon_amd import piv_tomo as pt

SHAPE = pt.shape_of(cases.VOLUME)


# ---- project_model -----------------------------------------------------------------------------------------------------------------
def test_one_voxel_adds_its_four_llrint_values():
    poly, grids, seen = cases.geometry()
    k, i, j = np.argwhere(seen.all(axis=0))[17]
    E, s = np.float32(0.7314), 12
    v = np.zeros(SHAPE, np.float32)
    v[k, i, j] = E
    acc = pm.project_model(v, poly, grids, cases.SENSORS, s)
    for c, (h, w) in enumerate(cases.SENSORS):
        inside, index, weights = pm.footprint(poly[c][k], grids[c], SHAPE[1:], (h, w))
        assert inside[i, j] and len(set(index[:, i, j])) == 4
        y, x = index[:, i, j] // w, index[:, i, j] % w
        assert (y[1], x[1]) == (y[0], x[0] + 1) and (y[2], x[2]) == (y[0] + 1, x[0]) and (y[3], x[3]) == (y[0] + 1, x[0] + 1)
        want = np.zeros(h * w, np.int64)
        for t in range(4):
            product = np.float32(weights[t, i, j] * E)                                  # in f32
            want[index[t, i, j]] += int(np.rint(np.float64(product) * 2.0 ** s))
        assert np.array_equal(acc[c].reshape(-1), want) and (want > 0).sum() == 4
        assert abs(float(weights[:, i, j].sum()) - 1.0) < 1e-6


def test_the_total_is_the_total_of_the_contributions_in_any_order():
    poly, grids, seen = cases.geometry()
    v = cases.volumes(2)
    acc = pm.project_model(v, poly, grids, cases.SENSORS, cases.PROJECT_SCALE)
    rng = np.random.default_rng(1)
    shuffled = pm.project_model(v, poly, grids, cases.SENSORS, cases.PROJECT_SCALE, order=rng.permutation)
    for c, sensor in enumerate(cases.SENSORS):
        inside, index, weights = pm.volume_footprint(poly[c], grids[c], SHAPE, sensor)
        assert np.array_equal(inside, seen[c])
        for f in range(2):
            live = (v[f] > 0) & inside
            total = sum(int(pm.quantise(weights[t][live] * v[f][live], cases.PROJECT_SCALE).sum()) for t in range(4))
            assert int(acc[c][f].sum()) == total > 0
        assert acc[c].dtype == np.int64 and np.array_equal(acc[c], shuffled[c])
    assert not seen[cases.OFF_CAMERA].all() and seen[cases.OFF_CAMERA].any() and seen[0].all()


def test_the_cap_is_reached_and_the_sum_does_not_wrap():
    poly, grids = cases.patch_geometry()
    v = cases.capped_volume()
    acc = pm.project_model(v, poly, grids, cases.PATCH_SENSORS, 20)
    for c in range(2):
        inside, index, weights = pm.volume_footprint(poly[c], grids[c], SHAPE, cases.PATCH_SENSORS[c])
        live = (v > 0) & inside
        assert inside.all()
        taps = sum(int((weights[t][live] > 0).sum()) for t in range(4))
        assert int(acc[c].sum()) == taps * 2 ** 31 and acc[c].max() > 2 ** 38 and (acc[c] >= 0).all()
    assert pm.quantise(np.float32(np.inf), 0) == 2 ** 31 and pm.quantise(np.float32(np.nan), 0) == 0 and pm.quantise(np.float32(-1), 0) == 0
    assert pm.quantise(np.float32(0.5), 0) == 0 and pm.quantise(np.float32(1.5), 0) == 2 and pm.quantise(np.float32(2.5), 0) == 2      # llrint: ties to even
    with np.errstate(over="ignore"):
        assert pm.images_of(np.int64(2 ** 62), -126) == np.inf and pm.images_of(np.int64(3), 1) == np.float32(1.5)


# ---- the pairing of gather and scatter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu_roots", [0, 1, 2])
def test_a_volumes_own_images_leave_it_unchanged_bit_for_bit(mu_roots):
    """frames := the f32 images of the volume's exact re-projection: I_bar and P_bar are the same operations on the same
    values, r = 1, and with threshold 0 the volume comes back bit for bit -- only if the update gathers where, and with the
    weights, the projection scattered."""
    poly, grids, seen = cases.geometry()
    v = np.where(seen.all(axis=0), np.where(cases.volumes(2) > 0, cases.volumes(2), np.float32(0)), np.float32(0))
    s = 24
    frames = [pm.images_of(a, s) for a in pm.project_model(v, poly, grids, cases.SENSORS, s)]
    got = pm.mart_model_f32(frames, v, poly, grids, 2, mu_roots, 0.0, s)
    assert (v > 0).sum() > 500 and got.tobytes() == v.tobytes()
    moved = [np.roll(f, 1, axis=2) for f in frames]                                     # the control: frames one pixel off are not a fixed point
    assert pm.mart_model_f32(moved, v, poly, grids, 2, mu_roots, 0.0, s).tobytes() != v.tobytes()


# ---- zeros, unseen and masked voxels, the threshold --------------------------------------------------------------------------------
def test_zeros_stay_zero_and_unseen_voxels_go_to_zero():
    poly, grids, seen = cases.geometry()
    v, frames = cases.volumes(2), cases.frames(2)
    s = cases.scale(2)
    got = pm.mart_model_f32(frames, v, poly, grids, 1, 1, 0.0, s)
    dead = ~(v > 0)
    assert got[dead].tobytes() == v[dead].tobytes()                                     # zeros, negatives, NaN: as they were
    unseen = ~seen.all(axis=0)
    assert unseen.any() and (got[:, unseen][v[:, unseen] > 0] == 0).all()
    # a voxel a camera does not see contributes nothing to that camera
    only = np.zeros(SHAPE, np.float32)
    k, i, j = np.argwhere(~seen[cases.OFF_CAMERA])[0]
    only[k, i, j] = 1.0
    acc = pm.project_model(only, poly, grids, cases.SENSORS, s)
    assert acc[cases.OFF_CAMERA].sum() == 0 and acc[0].sum() > 0


def test_a_footprint_on_a_dark_frame_ends_the_voxel_at_that_camera():
    poly, grids, seen = cases.geometry()
    v = np.where(cases.volumes(1)[0] > 0, cases.volumes(1)[0], np.float32(0))
    frames = [np.ones(sensor, np.float32) for sensor in cases.SENSORS]
    k, i, j = np.argwhere(seen.all(axis=0) & (v > 0))[40]
    _, index, _ = pm.footprint(poly[1][k], grids[1], SHAPE[1:], cases.SENSORS[1])
    frames[1].reshape(-1)[index[:, i, j]] = 0.0
    s = pm.scale_log2_for(frames)
    states = {}
    for n_cams in (2, 3):                                                               # after camera 1's step; after the whole iteration
        states[n_cams] = pm.mart_model_f32(frames[:n_cams], v, poly[:n_cams], grids[:n_cams], 1, 1, 0.0, s)
    assert states[2][k, i, j] == 0 and states[3][k, i, j] == 0
    assert pm.mart_model_f32(frames[:1] + frames[2:], v, poly[[0, 2]], grids[[0, 2]], 1, 1, 0.0, s)[k, i, j] > 0


def test_the_mask_and_the_threshold():
    poly, grids, seen = cases.geometry()
    v, frames, mask = cases.volumes(2), cases.frames(2), cases.mask()
    s = cases.scale(2)
    free = pm.mart_model_f32(frames, v, poly, grids, 1, 1, 0.0, s)
    masked = pm.mart_model_f32(frames, v, poly, grids, 1, 1, 0.0, s, mask)
    live = v > 0
    assert (masked[:, mask == 1][live[:, mask == 1]] == 0).all() and (free[:, (mask == 1) & seen.all(axis=0)] > 0).any()
    thr = np.float32(0.05)
    cut = pm.mart_model_f32(frames, v, poly, grids, 1, 1, thr, s, mask)
    assert ((masked > 0) & (masked < thr)).any() and not ((cut > 0) & (cut < thr)).any()
    assert (cut[live] == 0).sum() > (masked[live] == 0).sum() and (cut[live] > 0).any()


def test_the_arguments_that_are_refused():
    poly, grids, _ = cases.geometry()
    v, frames = cases.volumes(1), cases.frames(1)
    good = dict(iterations=1, mu_roots=1, threshold=0.0, scale_log2=10)
    for bad in (dict(iterations=0), dict(mu_roots=-1), dict(mu_roots=4), dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=np.inf),
                dict(scale_log2=-127), dict(scale_log2=63)):
        with pytest.raises(ValueError):
            pm.mart_model_f32(frames, v, poly, grids, **{**good, **bad})
    with pytest.raises(ValueError):
        pm.mart_model_f32(frames[:1], v, poly[:1], grids[:1], **good)
    with pytest.raises(ValueError):
        pm.mart_model_f32(cases.frames(2), v, poly, grids, **good)
    with pytest.raises(ValueError):
        pm.project_model(v, poly, grids, cases.SENSORS, 63)
    for relaxation, roots in ((1, 0), (0.5, 1), (0.25, 2), (0.125, 3)):
        assert pm.mu_roots_of(relaxation) == roots
    for relaxation in (0.3, 2, 0, -0.5, None, "half"):
        with pytest.raises(ValueError):
            pm.mu_roots_of(relaxation)


def test_the_scale_is_the_largest_that_keeps_four_maxima_under_the_cap():
    for m in (1.0, 0.5, 0.7, 1.87, 255.0, 65535.0, 1e-3, 1e30):
        s = pm.scale_log2_for([np.array([[0.0, m]], np.float32), np.array([[-5.0, np.nan, np.inf]], np.float32)])
        m32 = float(np.float32(m))
        assert 4.0 * m32 * 2.0 ** s <= 2.0 ** 31 < 4.0 * m32 * 2.0 ** (s + 1)
    assert pm.scale_log2_for(np.zeros((2, 2))) == 0 and pm.scale_log2_for(np.full((2, 2), 1e-60)) == 62 and pm.scale_log2_for([np.float64(1e60)]) == -126
    assert pm.default_threshold([np.array([0.5, 2.0], np.float32)]) == float(np.float32(2e-4))


# ---- the f32 model against the f64 one ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pm.CASES))
def test_the_f32_model_against_the_f64_model(name):
    """After 5 iterations from one first guess, the largest difference relative to max E: every seed under cases.F32_BAR, twice
    the worst seed measured: rounding differences are multiplied through 5 N updates."""
    worst = 0.0
    for seed in pt.CASE_SEEDS:
        m = cases.chain_model(name, seed)
        poly, grids = pt.los_coefficients(m["cameras"], pt.CASE_VOLUME)
        first = m["first"].astype(np.float32)
        s, thr = pm.scale_log2_for(list(m["frames"])), pm.default_threshold(list(m["frames"]))
        E32 = pm.mart_model_f32(m["frames"], first, poly, grids, cases.ITERATIONS, 1, thr, s, m["mask"])
        E64 = pm.mart_model(m["frames"], first, poly, grids, cases.ITERATIONS, 1, thr, m["mask"])
        rel = float(np.abs(E32 - E64).max() / E64.max())
        print(f"{name}, seed {seed}: scale_log2 {s}, threshold {thr:.3e}, f32 against f64 {rel:.3e} of max E")
        worst = max(worst, rel)
    print(f"{name}: worst seed {worst:.3e}")
    assert worst <= cases.F32_BAR


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------
def check_seed(name, seed):
    m = cases.chain_model(name, seed)
    d, vec, flags, partial = m["result"]
    print(f"{name}, seed {seed}: Q MinLOS {m['q_los'][0]:.3f} (interior {m['q_los'][1]:.3f}), after {cases.ITERATIONS} iterations {m['q_mart'][0]:.3f} "
          f"(interior {m['q_mart'][1]:.3f}); rms dX dY dZ {m['rms'].round(4)} voxels over {m['nodes']} interior nodes; "
          f"{np.mean(m['volumes'][0] == 0):.3f} of the voxels at 0")
    assert m["q_mart"][1] > m["q_los"][1]                                               # the condition: MART improves the interior
    assert m["nodes"] >= 12 and not partial.any() and not (flags[pt.interior(flags.shape)] & ~pc.FLAG_OUTSIDE).any()
    return m["rms"]


@pytest.mark.parametrize("name", list(pm.CASES))
def test_mart_improves_the_interior_on_seed_0(name):
    rms = check_seed(name, 0)
    assert (rms <= np.array(cases.CHAIN_BARS[name])).all()


@pytest.mark.parametrize("name", list(pm.CASES))
def test_the_model_chain_with_mart_on_every_seed(name):
    """mart_model with mu = 1/2 and 5 iterations on every seed of piv_tomo.CASE_SEEDS: the interior Q above MinLOS's, and the
    rms error per component over the interior nodes under the recorded bar (the worst seed x 1.25)."""
    worst = np.zeros(3)
    for seed in pt.CASE_SEEDS:
        worst = np.maximum(worst, check_seed(name, seed))
    print(f"{name}: worst seed {worst.round(4)}, x 1.25 = {(1.25 * worst).round(4)}")
    assert (worst <= np.array(cases.CHAIN_BARS[name])).all() and (worst < 1.0 / 3.0).all()


def test_the_cases_and_the_interior():
    assert list(pm.CASES)[:4] == list(pt.CASES) and pm.CASES["uniform_inside"]["margin"] == 0.0 and len(pt.CASES) == 4
    _, _, vol, (P, _, _) = pm.case_inputs("uniform_inside", 0)
    lo = np.array([vol["x0"], vol["y0"], vol["z0"]])
    hi = lo + vol["pitch"] * (np.array([vol["nx"], vol["ny"], vol["nz"]]) - 1)
    assert (P >= lo).all() and (P <= hi).all()
    E = np.zeros(pt.shape_of(vol))
    E[4:-4, 8:-8, 8:-8] = 1.0
    T = np.ones_like(E)
    assert pm.interior_quality(E, T) == pytest.approx(1.0) and pt.quality(E, T) < 0.8
