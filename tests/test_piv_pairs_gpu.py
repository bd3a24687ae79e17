"""PIV frame pairs on the GPU (photon_flow_from_grid, photon_sources_piv_advected; include/parallel_ray_tracing.h): the
advected field against the host model of photon_amd/piv_pairs.py bit for bit, the extent it hands the lens-sample cull,
and a traced pair whose image shifts follow the paraxial relation."""
import ctypes
import math

import numpy as np
import pytest

from photon_amd import piv_pairs as pp
from photon_amd import scenes
from photon_amd.ray_tracing import single_lens_camera

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "z", "radiance", "diameter_index")
LO, HI = (-3.0e4, -3.0e4, -7.5e3), (3.0e4, 3.0e4, 7.5e3)
Z_OBJ = 823668.35
CDF = np.cumsum(np.full(27, 1.0 / 27.0))
GEOM = single_lens_camera(lens_model="general", **scenes.SAMPLE_LENS)          # the camera of scenes.piv_scene


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def download(src):
    d = src.download()
    src.free()
    return d


def vortex_plus_uniform():
    lo, hi = (-4.5e4, -4.5e4, -8e3), (4.5e4, 4.5e4, 8e3)
    a = pp.lamb_oseen_vortex(6.0e7, 6.0e3, (2.0e3, -1.0e3), lo, hi, (97, 97, 5))
    b = pp.uniform_flow((150.0, -90.0, 20.0), lo, hi, (97, 97, 5))
    return pp.add_flows(a, b)


@pytest.mark.parametrize("cdf", [None, CDF], ids=["no_cdf", "cdf"])
def test_no_motion_is_photon_sources_piv_bit_for_bit(photon, cdf):
    n = 50_001
    want = download(photon.sources_piv(1234, n, LO, HI, Z_OBJ, 730.0, 500.0, cdf))
    vortex = photon.flow_from_grid(*vortex_plus_uniform())
    still = photon.flow_from_grid(*pp.uniform_flow((0.0, 0.0, 0.0), LO, HI, 3))
    try:
        for what, kw in (("flow None", dict(flow=None, t=0.0)), ("t = 0", dict(flow=vortex, t=0.0)),
                         ("zero field", dict(flow=still, t=3.5, steps=5))):
            src, world = photon.sources_piv_advected(1234, n, LO, HI, Z_OBJ, 730.0, 500.0, cdf, return_world=True, **kw)
            got = download(src)
            for key in FIELDS:
                assert np.array_equal(got[key], want[key]), (what, key)
            assert np.array_equal(world, pp.piv_field(1234, n, LO, HI, Z_OBJ, 730.0, 500.0, cdf)["world"]), what
    finally:
        vortex.free()
        still.free()


def test_vortex_advection_is_the_host_model_bit_for_bit(photon):
    n, t, steps = 100_000, 1.5, 16
    flow_grid = vortex_plus_uniform()
    flow = photon.flow_from_grid(*flow_grid)
    try:
        src, world = photon.sources_piv_advected(99, n, LO, HI, Z_OBJ, 730.0, 500.0, CDF, flow=flow, t=t, steps=steps,
                                                 return_world=True)
        got = download(src)
        small = download(photon.sources_piv_advected(99, 1000, LO, HI, Z_OBJ, 730.0, 500.0, CDF, flow=flow, t=t, steps=steps))
    finally:
        flow.free()
    want = pp.advect(99, n, LO, HI, Z_OBJ, 730.0, 500.0, CDF, flow=flow_grid, t=t, steps=steps)
    assert np.array_equal(world, want["world"])
    for key in ("x", "y", "z", "diameter_index"):
        assert np.array_equal(got[key], want[key]), key
    assert ulps(got["radiance"], want["radiance"]).max() <= pp.RADIANCE_ULP
    start = pp.piv_field(99, n, LO, HI, Z_OBJ, 730.0, 500.0)["world"]
    moved = np.hypot(*(world[:, :2] - start[:, :2]).T)
    assert moved.max() > 1000.0 and np.median(moved) > 100.0 and (moved > 0).all()      # the vortex and the drift act
    for key in FIELDS:                                               # counter-based: a prefix is the smaller call
        assert np.array_equal(small[key], got[key][:1000]), key


def test_extent_follows_the_particles_out_of_the_box(photon):
    """Particles carried far outside the box they were drawn from: the lens-sample cull must see where they are."""
    import torch
    n = 300
    lo, hi = (-2.0e4, -5.0e3, -1.0e3), (2.0e4, 5.0e3, 1.0e3)
    # outward stretching along x, u = k x (affine: trilinear reproduces it): x grows tenfold by t = 1, so the particles near
    # the axis stay in view while the outer ones reach 2e5 um from it
    k = math.log(10.0)
    gx, gy, gz, spacing, origin = pp.grid_nodes((-2.5e5, -2.5e5, -2.0e3), (2.5e5, 2.5e5, 2.0e3), (3, 3, 2))
    u = np.broadcast_to(k * gx[None, None, :], (2, 3, 3)).astype(np.float32)
    zero = np.zeros_like(u)
    flow = photon.flow_from_grid(u, zero, zero, spacing, origin)
    call = scenes.piv_scene(n_particles=n, rays_per_source=1000, mie=True, polydisperse=True, seed=3)
    try:
        adv = photon.sources_piv_advected(77, n, lo, hi, GEOM["z_object"], 730.0, 500.0, CDF, flow=flow, t=1.0)
        frame1 = photon.sources_piv(77, n, lo, hi, GEOM["z_object"], 730.0, 500.0, CDF)
    finally:
        flow.free()
    d = adv.download()
    assert np.abs(d["x"]).max() > 1.5e5                                # they left the box (|x| <= 2e4) ...
    assert (np.abs(d["x"]) < 4.0e4).sum() > 10                          # ... and some of them are in view
    call.src_x, call.src_y, call.src_z = d["x"], d["y"], d["z"]
    call.src_radiance, call.src_diameter_index = d["radiance"], d["diameter_index"]
    host_img = photon.render(call)
    host_scene = photon.scene_create(call)
    gen_scene = photon.scene_create_from_sources(call, adv)
    box_scene = photon.scene_create_from_sources(call, frame1)
    try:
        live_host, live_gen, live_box = host_scene.live_samples(), gen_scene.live_samples(), box_scene.live_samples()
        img = torch.zeros(host_img.size, dtype=torch.float32, device="cuda")
        gen_scene.trace(img.data_ptr())
        torch.cuda.synchronize()
        gen_img = img.cpu().numpy().reshape(host_img.shape)
    finally:
        for s in (host_scene, gen_scene, box_scene):
            s.free()
        adv.free()
        frame1.free()
    assert host_img.any() and rel_l2(gen_img, host_img) <= 1e-6
    # the generated scene keeps every lens sample the host-array scene keeps ...
    assert np.isin(live_host, live_gen).all(), (live_host.size, live_gen.size)
    # ... which the frame-1 box would not have: copying its extent would drop samples that carry light
    assert not np.isin(live_host, live_box).all()


def test_piv_pair_shifts_follow_the_paraxial_relation(photon):
    """A reduced sample camera (2000 particles x 1000 rays, volume-free), a uniform world shift: every particle's image
    moves by -m(Z) delta, m(Z) = s_i / (s_o + Z) of the single-lens principal-plane geometry (the BOS test's relation)."""
    import torch
    n, rays = 2000, 1000
    delta = np.array([300.0, -200.0, 0.0])
    lo, hi = (-1.5e4, -1.5e4, -1.0e3), (1.5e4, 1.5e4, 1.0e3)
    call = scenes.piv_scene(n_particles=n, rays_per_source=rays, mie=False, seed=4)
    geom, z_obj = GEOM, GEOM["z_object"]
    flow = photon.flow_from_grid(*pp.uniform_flow(delta, lo, hi, 2))
    try:
        f1, w1 = photon.sources_piv_advected(21, n, lo, hi, z_obj, 730.0, 1.0e4, flow=None, t=0.0, return_world=True)
        f2, w2 = photon.sources_piv_advected(21, n, lo, hi, z_obj, 730.0, 1.0e4, flow=flow, t=1.0, return_world=True)
    finally:
        flow.free()
    np.testing.assert_allclose(w2 - w1, np.broadcast_to(delta, w1.shape), rtol=0, atol=1e-9)
    recs = []
    h, w = call.image_shape
    for src in (f1, f2):
        scene = photon.scene_create_from_sources(call, src)
        img = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        try:
            scene.trace_moments(img.data_ptr(), rec.data_ptr())
            torch.cuda.synchronize()
        finally:
            scene.free()
            src.free()
        recs.append(rec.cpu().numpy())
    d = pp.image_displacements(recs[0], recs[1], call.camera, rays)
    both = ~np.isnan(d).any(axis=1)
    assert both.sum() > 0.9 * n, both.sum()
    assert np.array_equal(recs[0][both, 0], recs[1][both, 0])           # far from the edges: every ray arrives in both frames
    m = geom["image_distance"] / (geom["object_distance"] + w1[:, 2])
    pitch = float(call.camera["pixel_pitch"])
    predicted = -m[:, None] * delta[None, :2] / pitch
    rel = np.abs(d[both] - predicted[both]) / np.abs(predicted[both])
    assert (rel < 0.015).all(), rel.max(axis=0)
    print(f"PIV pair: {both.sum()} particles in both frames, |measured - predicted| / predicted: median "
          f"{np.median(rel):.2e}, max {rel.max():.2e}")


def test_out_of_plane_motion_moves_z_and_the_sheet_radiance_only(photon):
    n, w0 = 20_000, 450.0
    flow_grid = pp.uniform_flow((0.0, 0.0, w0), LO, HI, 2)
    flow = photon.flow_from_grid(*flow_grid)
    try:
        src, world = photon.sources_piv_advected(8, n, LO, HI, Z_OBJ, 730.0, 500.0, flow=flow, t=1.0, return_world=True)
    finally:
        flow.free()
    got = download(src)
    frame1 = download(photon.sources_piv(8, n, LO, HI, Z_OBJ, 730.0, 500.0))
    assert np.array_equal(got["x"], frame1["x"]) and np.array_equal(got["y"], frame1["y"])
    start = pp.piv_field(8, n, LO, HI, Z_OBJ, 730.0, 500.0)["world"]
    np.testing.assert_allclose(world[:, 2] - start[:, 2], w0, rtol=0, atol=1e-9)
    sigma = 730.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    sheet = 500.0 / (sigma * math.sqrt(2 * math.pi)) * np.exp(-world[:, 2] ** 2 / (2 * sigma ** 2))
    assert ulps(got["radiance"], sheet).max() <= pp.RADIANCE_ULP + 2          # (the test's own exp and products)
    assert not np.array_equal(got["radiance"], frame1["radiance"])


def test_refusals_leave_the_handle_and_print_one_line(photon, capfd):
    L = photon.lib
    lo = np.ascontiguousarray(LO, np.float64)
    hi = np.ascontiguousarray(HI, np.float64)
    flow = photon.flow_from_grid(*pp.uniform_flow((1.0, 0.0, 0.0), LO, HI, 2))
    sentinel = 0x5A5A
    capfd.readouterr()
    try:
        for what, fl, t, steps in (("steps 0", flow.handle, 1.0, 0), ("t nan", flow.handle, float("nan"), 16),
                                   ("no flow", None, 1.0, 16)):
            h = ctypes.c_void_p(sentinel)
            rc = L.photon_sources_piv_advected(1, 100, lo.ctypes.data, hi.ctypes.data, Z_OBJ, 730.0, 500.0, None, 0, fl,
                                               t, steps, None, ctypes.byref(h))
            err = capfd.readouterr().err
            assert rc != 0 and h.value == sentinel, what
            assert len(err.strip().splitlines()) == 1 and "photon_sources_piv_advected" in err, (what, err)
    finally:
        flow.free()
    u = np.zeros((4, 1, 4), np.float32)                                         # ny = 1: a 1-node axis
    sp = np.ones(3)
    og = np.zeros(3)
    h = ctypes.c_void_p(sentinel)
    rc = L.photon_flow_from_grid(u.ctypes.data, u.ctypes.data, u.ctypes.data, 4, 1, 4, sp.ctypes.data, og.ctypes.data,
                                 ctypes.byref(h))
    err = capfd.readouterr().err
    assert rc != 0 and h.value == sentinel
    assert len(err.strip().splitlines()) == 1 and "photon_flow_from_grid" in err, err
