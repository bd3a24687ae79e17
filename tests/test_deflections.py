"""photon_amd.deflections (no GPU): the host model of a per-source moments record and the dot shifts built on it, held to
the reference's own dump workflow (python_codes/light_ray_processing.py: calculate_dot_average :243-275,
convert_pos_to_pix :277-300, calculate_sensor_origin :513-531, calculate_lightray_deflections :211-241)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from photon_amd import deflections as dfl


def _reference_dot_average(a, rays_per_dot):
    """calculate_dot_average: f32 np.add.reduceat over consecutive rays / rays."""
    return np.add.reduceat(a, range(0, a.size, rays_per_dot)) / rays_per_dot


def _random_dumps(n_src, rps, seed):
    rng = np.random.default_rng(seed)
    n = n_src * rps
    pos = np.empty((n, 3), np.float32)
    pos[:, 0] = rng.uniform(-9000, 9000, n)
    pos[:, 1] = rng.uniform(-9000, 9000, n)
    pos[:, 2] = rng.uniform(40000, 41000, n)
    d = rng.normal(size=(n, 3))
    dirs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    dead = rng.random(n) < 0.2                              # rays that never reach the sensor: NaN in both dumps,
    dead &= (np.arange(n) // (4 * rps)) % 2 == 1            # in every other group of 4 sources: some dots arrive whole
    pos[dead] = np.nan
    dirs[dead] = np.nan
    return pos, dirs


def _scalar_record(pos, dirs):
    """The record contract written out one ray at a time: 64 lanes, increasing j per lane, then the fold by halves."""
    p = [[0.0] * 8 for _ in range(64)]
    for j in range(pos.shape[0]):
        x, y, z = (float(v) for v in pos[j])
        if np.isnan(x) or np.isnan(y) or np.isnan(z):
            continue
        vals = [1.0, x, y, z] + [float(np.arccos(np.float64(v))) for v in dirs[j]] + [x * x + y * y]
        lane = p[j % 64]
        for f in range(8):
            lane[f] = lane[f] + vals[f]
    off = 32
    while off:
        for lane in range(off):
            p[lane] = [a + b for a, b in zip(p[lane], p[lane + off])]
        off //= 2
    return np.array(p[0])


@pytest.mark.parametrize("rps", [1, 7, 64, 65, 500])
def test_record_order_is_the_contract(rps):
    pos, dirs = _random_dumps(5, rps, seed=rps)
    rec = dfl.moments_from_dumps(pos, dirs, rps)
    assert rec.shape == (5, 8) and rec.dtype == np.float64
    for s in range(5):
        want = _scalar_record(pos[s * rps:(s + 1) * rps], dirs[s * rps:(s + 1) * rps])
        assert np.array_equal(rec[s].view(np.uint64), want.view(np.uint64)), s


@pytest.mark.parametrize("rps", [1, 7, 64, 65, 500])
def test_reference_policy_is_the_reference_dot_average(rps):
    n_src = 40
    pos, dirs = _random_dumps(n_src, rps, seed=100 + rps)
    rec = dfl.moments_from_dumps(pos, dirs, rps)
    ang = np.arccos(dirs)                                   # the reference's reader (light_ray_processing.py:120-140)
    for group in (1, 4):
        m = dfl.dot_means(rec, rps, group=group, policy="reference")
        for axis in range(3):
            want = _reference_dot_average(pos[:, axis], group * rps)
            got = m["pos"][:, axis]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (group, axis)
            ok = ~np.isnan(want)
            assert ok.any()
            np.testing.assert_allclose(got[ok], want[ok], rtol=1e-6, atol=1e-6 * 9000)
            want_a = _reference_dot_average(ang[:, axis], group * rps)
            assert np.array_equal(np.isnan(m["dir"][:, axis]), np.isnan(want_a)), (group, axis)
            np.testing.assert_allclose(m["dir"][ok, axis], want_a[ok], rtol=1e-6)
        arrived = dfl.dot_means(rec, rps, group=group, policy="arrived")
        live = ~np.isnan(pos[:, 0])
        cnt = np.add.reduceat(live.astype(np.float64), range(0, live.size, group * rps))
        assert np.array_equal(arrived["n"], cnt)
        sx = np.add.reduceat(np.where(live, pos[:, 0], 0).astype(np.float64), range(0, live.size, group * rps))
        with np.errstate(invalid="ignore"):
            np.testing.assert_allclose(arrived["pos"][:, 0], sx / cnt, rtol=1e-12)


def test_records_are_additive():
    rps = 65
    pos, dirs = _random_dumps(12, rps, seed=3)
    rec = dfl.moments_from_dumps(pos, dirs, rps)
    m1 = dfl.dot_means(rec, rps, group=3, policy="arrived")
    merged = rec.reshape(4, 3, 8).sum(axis=1)
    m2 = dfl.dot_means(merged, 3 * rps, group=1, policy="arrived")
    np.testing.assert_allclose(m1["pos"], m2["pos"], rtol=1e-14)
    # chunked host model: the same bits
    assert np.array_equal(dfl.moments_from_dumps(pos, dirs, rps, max_rays=200), rec)


def test_to_pixels_and_signs_are_the_reference_s():
    cam = {"pixel_pitch": 17.0, "x_pixel_number": 1024, "y_pixel_number": 1024}
    pos = np.array([[0.0, 0.0, 1.0], [-(1024 / 2 - 1) * 17.0, 170.0, 0.0]])
    px = dfl.to_pixels(pos, cam)
    pos0 = -(1024 / 2 - 1) * 17.0                           # calculate_sensor_origin
    np.testing.assert_allclose(px, (pos[:, :2] - pos0) / 17.0)
    assert px[1, 0] == 0.0
    # a rectangular sensor: each axis its own count
    rect = dict(cam, y_pixel_number=512)
    np.testing.assert_allclose(dfl.to_pixels(pos, rect)[:, 1], (pos[:, 1] + (512 / 2 - 1) * 17.0) / 17.0)
    # d_pos = pos1 - pos2, d_dir = dir2 - dir1 (calculate_lightray_deflections)
    rps = 7
    p1, d1 = _random_dumps(6, rps, seed=9)
    p1[:] = np.nan_to_num(p1, nan=1.0)
    d1[:] = np.nan_to_num(d1, nan=0.5)
    p2, d2 = p1.copy(), d1.copy()
    p2[:, 0] += 34.0                                        # image 2 two pixels further right
    d2[:, 0] = np.cos(np.arccos(d1[:, 0]) + 1e-3).astype(np.float32)
    r1, r2 = dfl.moments_from_dumps(p1, d1, rps), dfl.moments_from_dumps(p2, d2, rps)
    d = dfl.dot_deflections(r1, r2, cam, rps)
    np.testing.assert_allclose(d.d_pos[:, 0], -2.0, rtol=1e-5)
    np.testing.assert_allclose(d.d_pos[:, 1], 0.0, atol=1e-9)
    np.testing.assert_allclose(d.d_dir[:, 0], 1e-3, rtol=1e-2)
    assert d.pos1.shape == (6, 2) and d.dir1.shape == (6, 3) and d.rms1.shape == (6,)
    assert (d.rms1 > 0).all() and np.allclose(d.rms1, d.rms2, rtol=1e-4)
    assert dfl.summary(d).splitlines()[0] == "x: -2.00 to -2.00 pix."


def test_dot_means_rejects_bad_arguments():
    rec = np.zeros((6, 8))
    with pytest.raises(ValueError):
        dfl.dot_means(rec, 5, group=4)
    with pytest.raises(ValueError):
        dfl.dot_means(rec, 5, policy="mean")
    with pytest.raises(ValueError):
        dfl.moments_from_dumps(np.zeros((10, 3), np.float32), np.zeros((10, 3), np.float32), 3)
    m = dfl.dot_means(rec, 5, policy="arrived")             # nothing arrived: NaN, not a division warning turned error
    assert np.isnan(m["pos"]).all() and (m["n"] == 0).all()


def test_dump_pair_against_the_reference_reader(oracle, tmp_path):
    """The oracle renders dump_pair_calls (24 sources x 25 rays per image); the host model over its dumps, averaged per
    source, equals the reference reader's own per-ray arrays (tests/golden/dumps_reference_reader.npz) averaged by
    reduceat, and dot_deflections equals the reduceat of the reader's d_pos / d_dir."""
    from conftest import dump_pair_calls
    calls = dump_pair_calls(str(tmp_path))
    for call in calls:
        oracle.render(call, interpolation=1)
    ref = np.load(os.path.join(GOLDEN, "dumps_reference_reader.npz"))
    rps = int(calls[0].lightray_number_per_particle)
    assert rps == 25
    recs = []
    for im in ("im1", "im2"):
        pos = np.fromfile(tmp_path / "light-ray-positions" / im / "pos_0000.bin", np.float32).reshape(-1, 3)
        dirs = np.fromfile(tmp_path / "light-ray-directions" / im / "dir_0000.bin", np.float32).reshape(-1, 3)
        recs.append(dfl.moments_from_dumps(pos, dirs, rps))
    for k, rec in zip((1, 2), recs):
        m = dfl.dot_means(rec, rps, policy="reference")
        for col, axis in enumerate("xyz"):
            want = _reference_dot_average(ref[f"pos{k}_{axis}"], rps)
            assert np.array_equal(np.isnan(m["pos"][:, col]), np.isnan(want)), (k, axis)
            np.testing.assert_allclose(m["pos"][:, col], want, rtol=1e-6, atol=1e-3, equal_nan=True)
            want_a = _reference_dot_average(ref[f"dir{k}_{axis}"], rps)
            np.testing.assert_allclose(m["dir"][:, col], want_a, rtol=1e-6, equal_nan=True)
    d = dfl.dot_deflections(recs[0], recs[1], calls[0].camera, rps, policy="reference")
    pitch = float(calls[0].camera["pixel_pitch"])
    for col, axis in enumerate("xy"):
        want = _reference_dot_average(ref[f"d_pos_{axis}"], rps) / pitch
        assert np.array_equal(np.isnan(d.d_pos[:, col]), np.isnan(want))
        np.testing.assert_allclose(d.d_pos[:, col], want, rtol=1e-6, atol=1e-6)
    for col, axis in enumerate("xyz"):
        np.testing.assert_allclose(d.d_dir[:, col], _reference_dot_average(ref[f"d_dir_{axis}"], rps), rtol=1e-6, atol=1e-6,
                                   equal_nan=True)
    assert np.count_nonzero(np.abs(np.nan_to_num(d.d_pos[:, 0])) > 0) > 0      # the volume moved some dots
