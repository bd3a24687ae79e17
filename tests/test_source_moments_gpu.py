"""Per-source sensor moments on the GPU (photon_trace_moments, photon_start_ray_tracing_moments; include/parallel_ray_tracing.h):
records bit-exact against the host model over ray dumps, independent of the launch plan, unchanged by the culls, and the
dot shifts they give against the paraxial relation."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import bos_displacement_case, dump_pair_calls, load_fixture_call
from photon_amd import deflections as dfl
from photon_amd import scenes

pytestmark = pytest.mark.gpu

EXACT = [0, 1, 2, 3, 7]          # n, position sums, sum r^2: bit for bit; the acos sums to an ulp of f64 acos per ray


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def assert_records_equal(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    g, w = np.ascontiguousarray(got[:, EXACT]), np.ascontiguousarray(want[:, EXACT])
    bad = g.view(np.uint64) != w.view(np.uint64)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} exact fields differ, first at {np.argwhere(bad)[0]}"
    np.testing.assert_allclose(got[:, 4:7], want[:, 4:7], rtol=1e-13, atol=0, err_msg=what)


def read_dumps(call):
    pos = np.fromfile(os.path.join(call.lightray_position_save_path, "pos_0000.bin"), np.float32).reshape(-1, 3)
    dirs = np.fromfile(os.path.join(call.lightray_direction_save_path, "dir_0000.bin"), np.float32).reshape(-1, 3)
    return pos, dirs


def test_records_bit_exact_against_dumps(photon, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("PHOTON_INTERP", "linear")
    for sub in ("gpu", "cpu"):
        (tmp_path / sub).mkdir()
    gpu_calls = dump_pair_calls(str(tmp_path / "gpu"))
    cpu_calls = dump_pair_calls(str(tmp_path / "cpu"))
    for g, c in zip(gpu_calls, cpu_calls):
        rps = g.lightray_number_per_particle
        img, rec = photon.render_moments(g)
        assert rec.shape == (g.num_sources, 8) and rec[:, 0].sum() > 0
        assert_records_equal(rec, dfl.moments_from_dumps(*read_dumps(g), rps), "GPU dumps")
        oracle.render(c, interpolation=1)
        assert_records_equal(rec, dfl.moments_from_dumps(*read_dumps(c), rps), "oracle dumps")
        plain = photon.render(g)
        assert rel_l2(img, plain) <= 1e-6


@pytest.fixture(scope="module")
def through_volume(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments")
    rho, sp, org = scenes.bos_volume(40)
    nrrd = scenes.write_nrrd(str(d / "moments_40.nrrd"), rho, sp, org)
    return scenes.bos_scene(n_dots=5, points_per_dot=9, rays_per_source=150, density_grad_filename=nrrd, seed=3)


# 1 .. 64: both ends of every group size G = 1, 2, 4, ..., 64 of launch_moments; 65: a second ray in lane 0 of the full wave
GROUP_EDGES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65]


@pytest.mark.parametrize("rps", GROUP_EDGES)
def test_records_bit_exact_at_every_group_size(photon, tmp_path, rps):
    """Image 1 of conftest.dump_pair_calls (a few dots, no volume, every ray dumped) at `rps` rays per source: scene creation
    accepts every count from 1."""
    c = scenes.bos_scene(n_dots=3, points_per_dot=8, rays_per_source=rps, seed=5)
    c.simulate_density_gradients, c.ray_tracing_algorithm = False, 0
    c.save_lightrays, c.num_lightrays_save = True, c.num_rays
    for what in ("position", "direction"):
        d = tmp_path / f"light-ray-{what}s"
        d.mkdir()
        setattr(c, f"lightray_{what}_save_path", str(d))
    assert c.lightray_number_per_particle == rps and c.num_rays == c.num_sources * rps
    _, rec = photon.render_moments(c)
    assert rec.shape == (c.num_sources, 8) and rec[:, 0].sum() > 0
    assert_records_equal(rec, dfl.moments_from_dumps(*read_dumps(c), rps), f"{rps} rays per source")


def assert_launch_plan_changes_no_record(photon, call, algorithm, interp, base, k):
    """Every ray order x skip on / off x segments 1, -1, 4, and the source range split at k in either order: the records of
    photon_trace_moments must equal `base`."""
    import torch
    vol = photon.volume_load_nrrd(call.density_grad_filename, interp)
    vol.set_weight_bits(8)                                  # what start_ray_tracing sets (PHOTON_TEX_WEIGHTS default)
    scene = photon.scene_create(call)
    n = call.num_sources
    h, w = call.image_shape
    img = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    rec = torch.full((n, 8), -1.0, dtype=torch.float64, device="cuda")
    try:
        def trace(*ranges):
            rec.fill_(-1.0)
            for b, e in ranges:
                scene.trace_moments(img.data_ptr(), rec.data_ptr(), vol, algorithm, b, e)
            torch.cuda.synchronize()
            return rec.cpu().numpy()

        for order in (0, 1, 2):
            scene.set_ray_order(order)
            for skip in (True, False):
                scene.set_skip_doomed(skip)
                for seg in (1, -1, 4):
                    scene.set_march_segments(seg)
                    assert_records_equal(trace((0, n)), base, f"order {order} skip {skip} segments {seg}")
        scene.set_ray_order(2)
        scene.set_skip_doomed(True)
        scene.set_march_segments(-1)
        assert 0 < k < n
        assert_records_equal(trace((0, k), (k, n)), base, "split")
        assert_records_equal(trace((k, n), (0, k)), base, "split, reversed")
    finally:
        scene.free()
        vol.free()


@pytest.mark.parametrize("interp", [1, 2])
@pytest.mark.parametrize("algorithm", [1, 2])
def test_records_do_not_depend_on_the_launch_plan(photon, through_volume, monkeypatch, interp, algorithm):
    call = through_volume
    call.ray_tracing_algorithm = algorithm
    monkeypatch.setenv("PHOTON_INTERP", "cubic" if interp == 2 else "linear")
    base_img, base = photon.render_moments(call)
    assert base[:, 0].sum() > 0
    assert_launch_plan_changes_no_record(photon, call, algorithm, interp, base, 17)
    monkeypatch.setenv("PHOTON_DEVICES", "0,0,0")
    img3, rec3 = photon.render_moments(call)
    assert_records_equal(rec3, base, "PHOTON_DEVICES=0,0,0")
    assert rel_l2(img3, base_img) <= 1e-6


def test_records_of_a_small_group_do_not_depend_on_the_launch_plan(photon, through_volume, monkeypatch):
    """12 rays per source through the volume: moments_kernel<16>, four sources to a wave, behind every launch plan."""
    call = scenes.bos_scene(n_dots=5, points_per_dot=9, rays_per_source=12, density_grad_filename=through_volume.density_grad_filename,
                            seed=3)
    call.ray_tracing_algorithm = 2
    monkeypatch.setenv("PHOTON_INTERP", "cubic")
    _, base = photon.render_moments(call)
    assert base[:, 0].sum() > 0
    assert_launch_plan_changes_no_record(photon, call, 2, 2, base, 17)


def test_culls_of_the_volume_free_path_change_no_record(photon, monkeypatch):
    call = scenes.piv_scene(n_particles=1200, rays_per_source=600, mie=True, seed=21)
    scene = photon.scene_create(call)
    kept, live = scene.live_sources(), scene.live_rays()
    scene.free()
    assert kept is not None and kept.size < call.num_sources and live < call.lightray_number_per_particle
    img_on, on = photon.render_moments(call)
    monkeypatch.setenv("PHOTON_SKIP_DOOMED", "0")
    img_off, off = photon.render_moments(call)
    assert_records_equal(on, off, "skip_doomed on / off")
    assert np.array_equal(img_on, img_off)
    culled = np.setdiff1d(np.arange(call.num_sources), kept)
    assert (on[culled] == 0).all() and on[kept, 0].sum() > 0


@pytest.mark.parametrize("interp", [1, 2])
def test_every_dot_shifts_as_the_paraxial_relation_says(photon, oracle, tmp_path, monkeypatch, interp):
    monkeypatch.setenv("PHOTON_INTERP", "cubic" if interp == 2 else "linear")
    c1, c2, predicted = bos_displacement_case(str(tmp_path))
    rps, per_dot = c1.lightray_number_per_particle, 30
    _, r1 = photon.render_moments(c1)
    _, r2 = photon.render_moments(c2)
    d = dfl.dot_deflections(r1, r2, c1.camera, rps, group=per_dot)
    whole = ~np.isnan(d.d_pos[:, 0])
    assert whole.sum() >= 3, whole
    # d_pos = pos1 - pos2: on the sensor the dots of image 2 lie `predicted` pixels further along +x
    assert (np.abs(-d.d_pos[whole, 0] - predicted) < 0.015 * predicted).all(), (d.d_pos[whole, 0], predicted)
    assert (np.abs(d.d_pos[whole, 1]) < 0.01).all(), d.d_pos[whole, 1]
    recs = []
    for k, c in enumerate((c1, c2)):
        c.save_lightrays, c.num_lightrays_save = True, c.num_rays
        c.lightray_position_save_path = c.lightray_direction_save_path = str(tmp_path / f"im{k + 1}")
        os.makedirs(c.lightray_position_save_path, exist_ok=True)
        oracle.render(c, interpolation=interp if k else 1)
        recs.append(dfl.moments_from_dumps(*read_dumps(c), rps))
    o = dfl.dot_deflections(recs[0], recs[1], c1.camera, rps, group=per_dot)
    assert np.array_equal(np.isnan(o.d_pos), np.isnan(d.d_pos))
    assert np.nanmax(np.abs(o.d_pos - d.d_pos)) < 1e-4


def test_sample_bos_pair_at_full_size(photon):
    """Both sample BOS images (120 000 sources x 500 rays each); the sample volume lies outside every ray's path, so no dot moves."""
    recs = []
    for im in ("im1", "im2"):
        call = load_fixture_call(f"bos_full_{im}")
        photon.render_moments(call)                         # warm: volume cache, block cache
        t0 = time.perf_counter()
        _, rec = photon.render_moments(call)
        print(f"bos_full_{im}: {call.num_rays:.3g} rays, render_moments {1e3 * (time.perf_counter() - t0):.1f} ms")
        assert rec[:, 0].sum() > 0
        recs.append(rec)
    d = dfl.dot_deflections(recs[0], recs[1], call.camera, call.lightray_number_per_particle)
    whole = ~np.isnan(d.d_pos).any(axis=1)
    assert whole.sum() > 0.4 * whole.size                   # 56 % of the sources lie outside the view
    assert np.abs(d.d_pos[whole]).max() < 1e-3


def test_bad_arguments_and_records_outside_the_range(photon):
    import torch
    call = scenes.bos_scene(n_dots=3, points_per_dot=8, rays_per_source=40, seed=2)
    n = call.num_sources
    h, w = call.image_shape
    img = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    rec = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda")
    scene = photon.scene_create(call)
    try:
        f = photon.lib.photon_trace_moments
        ptr = ctypes.c_void_p
        assert f(scene.handle, None, 0, 0, n, ptr(img.data_ptr()), None, None) != 0
        assert f(scene.handle, None, 0, 0, n + 1, ptr(img.data_ptr()), ptr(rec.data_ptr()), None) != 0
        assert f(scene.handle, None, 0, 5, 4, ptr(img.data_ptr()), ptr(rec.data_ptr()), None) != 0
        assert f(scene.handle, None, 0, -1, 4, ptr(img.data_ptr()), ptr(rec.data_ptr()), None) != 0
        torch.cuda.synchronize()
        assert (rec == 7.0).all() and (img == 0).all()
        scene.trace_moments(img.data_ptr(), rec.data_ptr(), None, 0, 5, 19)
        torch.cuda.synchronize()
        r = rec.cpu().numpy()
        assert (r[:5] == 7.0).all() and (r[19:] == 7.0).all()
        assert (r[5:19, 0] > 0).any() and (r[5:19, 0] <= 40).all()
    finally:
        scene.free()
    moments = np.zeros((n, 8))
    status = []
    image = call.new_image()
    call.invoke(lambda *a: status.append(photon.start_ray_tracing_moments(*a[:-1], None)), image, extra=(moments.ctypes.data,))
    assert status[0] != 0
