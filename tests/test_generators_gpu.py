"""The kernels that make the inputs and the final picture, on inputs with no symmetry (tests/generator_cases.py; the
conditions those inputs meet are asserted on the CPU in tests/test_generators.py): photon_volume_gaussian and
photon_density_gaussian_write_nrrd on grids whose three sides, spacings, origins and centres all differ; the flow sampler
on a grid with nx != ny != nz that the particles leave through every face, and with a NaN node; the extent of generated
sources from boxes with lo != -hi; photon_postprocess_u16 against its numpy mirror over its whole parameter space."""
import numpy as np
import pytest

import generator_cases as gc
from photon_amd import piv_pairs as pp
from photon_amd import scenes
from photon_amd.ray_tracing import crop_window, postprocess_image

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. Gaussian volume -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.GAUSS_CASES))
def test_gaussian_volume_on_a_grid_with_no_symmetry(photon, oracle, tmp_path, name):
    case = gc.GAUSS_CASES[name]
    args = gc.gauss_args(case)
    nx, ny, nz = case["n"]
    in_place = {}
    for interp in (1, 2):
        g, o = photon.volume_gaussian(*args, interp), oracle.volume_gaussian(*args, interp)
        try:
            gi, oi = g.info(), o.info()
            for coefficients in ((False, True) if interp == 2 else (False,)):
                got, want = g.download(coefficients), o.download(coefficients)
                assert got.shape == (nz, ny, nx, 4)
                assert np.array_equal(bits(got), bits(want)), (interp, coefficients, int((bits(got) != bits(want)).sum()))
            in_place[interp] = g.download()
        finally:
            g.free()
            o.free()
        assert (gi.nx, gi.ny, gi.nz) == (oi.nx, oi.ny, oi.nz) == case["n"]
        assert bits(gi.data_min) == bits(oi.data_min) and bits(gi.step_size) == bits(oi.step_size)
        assert np.array_equal(bits(list(gi.min_bound)), bits(list(oi.min_bound)))
        assert np.array_equal(bits(list(gi.max_bound)), bits(list(oi.max_bound)))
        assert np.array_equal(bits(list(gi.grid_spacing)), bits(np.float32(case["spacing"])))
    # the same field as a file: read back it is the volume built in place, and its rho is the header's formula
    path = photon.density_gaussian_write_nrrd(str(tmp_path / f"gauss_{name}.nrrd"), *args)
    for interp in (1, 2):
        v = photon.volume_load_nrrd(path, interp)
        try:
            assert np.array_equal(bits(v.download()), bits(in_place[interp])), interp
        finally:
            v.free()
    rho_file, sp_file, org_file = scenes.read_nrrd(path)
    assert rho_file.shape == (nz, ny, nx) and rho_file.dtype == np.float32
    assert tuple(float(v) for v in sp_file) == case["spacing"] and tuple(float(v) for v in org_file) == case["origin"]
    np.testing.assert_allclose(rho_file, gc.gauss_rho(case), rtol=3e-7)              # the last ulp of exp
    assert np.array_equal(bits(in_place[1][..., 3]), bits(np.float32(0.225e-3) * rho_file))      # texel w = K rho, one f32 product


# ---- 2. flow sampler --------------------------------------------------------------------------------------------------
def advected(photon, flow_grid, cdf, n=gc.FLOW_N, keep=False):
    flow = photon.flow_from_grid(*flow_grid)
    try:
        src, world = photon.sources_piv_advected(gc.FLOW_SEED, n, gc.BOX_LO, gc.BOX_HI, gc.Z_OBJ, *gc.SHEET, cdf, flow=flow,
                                                 t=gc.FLOW_T, steps=gc.FLOW_STEPS, return_world=True)
    finally:
        flow.free()
    got = src.download()
    got["world"] = world
    if keep:
        return got, src
    src.free()
    return got


def assert_frame_is_the_model(got, want):
    assert np.array_equal(got["world"], want["world"], equal_nan=True)
    for key in ("x", "y", "z"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert np.array_equal(got["diameter_index"], want["diameter_index"])
    ok = ~np.isnan(want["radiance"])
    assert np.array_equal(np.isnan(got["radiance"]), ~ok)
    assert ulps(got["radiance"][ok], want["radiance"][ok]).max() <= pp.RADIANCE_ULP


@pytest.mark.parametrize("cdf", [None, gc.CDF], ids=["no_cdf", "cdf"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 3, 5)], ids=["3x5x7", "2x3x5"])
def test_flow_on_an_asymmetric_grid_left_on_every_side(photon, shape, cdf):
    """(nz, ny, nx) all different, the field different at every node, 16 to 36 % of the particles beyond each face: every
    stride, every cell clamp and every weight clamp of flow_sample decides stored bits."""
    grid = gc.noise_flow(shape)
    assert_frame_is_the_model(advected(photon, grid, cdf), gc.flow_advect(grid, cdf))


def test_flow_with_a_nan_node(photon):
    """The header's NaN rule (a NaN coordinate takes cell 0 and weight 0) on the device, and what follows from it: the
    stored x of those particles is NaN, so the sources' extent is left unset and every lens sample is launched."""
    import torch
    grid = gc.noise_flow(nan_node=gc.NAN_NODE)
    want = gc.flow_advect(grid, gc.CDF)
    got, src = advected(photon, grid, gc.CDF, keep=True)
    rays = 64
    call = scenes.piv_scene(n_particles=gc.FLOW_N, rays_per_source=rays, mie=True, polydisperse=True, seed=3)
    try:
        assert_frame_is_the_model(got, want)
        nan = np.isnan(got["x"])
        assert nan.sum() >= 1 and (~nan).sum() >= gc.FLOW_N // 2
        # (a field of the same box without the NaN does get culled: the all-live answer below is the NaN's doing)
        clean = photon.sources_piv(gc.FLOW_SEED, gc.FLOW_N, gc.BOX_LO, gc.BOX_HI, gc.GEOM["z_object"], *gc.SHEET, gc.CDF)
        clean_scene = photon.scene_create_from_sources(call, clean)
        gen_scene = photon.scene_create_from_sources(call, src)
        try:
            assert clean_scene.live_rays() < rays
            assert np.array_equal(gen_scene.live_samples(), np.arange(rays))
            h, w = call.image_shape
            img = torch.zeros(h * w, dtype=torch.float32, device="cuda")
            gen_scene.trace(img.data_ptr())
            torch.cuda.synchronize()
            gen_img = img.cpu().numpy().reshape(h, w)
        finally:
            clean_scene.free()
            gen_scene.free()
            clean.free()
    finally:
        src.free()

    def host_image(keep):
        call.src_x, call.src_y, call.src_z = got["x"][keep], got["y"][keep], got["z"][keep]
        call.src_radiance, call.src_diameter_index = got["radiance"][keep], got["diameter_index"][keep]
        return photon.render(call)
    host_img = host_image(np.ones(gc.FLOW_N, bool))
    assert host_img.any() and np.isfinite(host_img).all() and np.isfinite(gen_img).all()
    assert rel_l2(gen_img, host_img) <= 1e-6
    assert rel_l2(host_image(~nan), host_img) <= 1e-6                   # the NaN sources add nothing on either path


# ---- 3. extents of generated sources ----------------------------------------------------------------------------------
def assert_extent_keeps_the_light(photon, call, gen, near, axis):
    """`gen`: the handle under test; `near`: a handle whose extent misses the far particles.  The scene made from `gen`
    keeps every lens sample that the host-array scene of the same particles keeps, traces photon.render's image of them,
    and `near`'s extent would not have done."""
    import torch
    d = gen.download()
    coord = np.abs(d["xy"[axis]])
    assert coord.max() > 1.5e5 and (coord < 4.0e4).sum() > 10           # far out on one side, and enough of them in view
    call.src_x, call.src_y, call.src_z = d["x"], d["y"], d["z"]
    call.src_radiance, call.src_diameter_index = d["radiance"], d["diameter_index"]
    host_img = photon.render(call)
    host_scene = photon.scene_create(call)
    gen_scene = photon.scene_create_from_sources(call, gen)
    near_scene = photon.scene_create_from_sources(call, near)
    try:
        live_host, live_gen, live_near = host_scene.live_samples(), gen_scene.live_samples(), near_scene.live_samples()
        img = torch.zeros(host_img.size, dtype=torch.float32, device="cuda")
        gen_scene.trace(img.data_ptr())
        torch.cuda.synchronize()
        gen_img = img.cpu().numpy().reshape(host_img.shape)
    finally:
        for s in (host_scene, gen_scene, near_scene):
            s.free()
    print(f"live lens samples: host {live_host.size}, generated {live_gen.size}, near side {live_near.size}")
    assert live_host.size < call.lightray_number_per_particle          # the cull does bite
    assert np.isin(live_host, live_gen).all(), (live_host.size, live_gen.size)
    assert host_img.any() and rel_l2(gen_img, host_img) <= 1e-6
    assert not np.isin(live_host, live_near).all(), (live_host.size, live_near.size)
    return d


@pytest.mark.parametrize("name", list(gc.EXTENT_BOXES))
def test_extent_of_an_off_centre_box(photon, name):
    """photon_sources_piv: the extent is the larger of |box_min| and |box_max| per axis -- whichever side that is."""
    lo, hi, near_lo, near_hi, axis = gc.EXTENT_BOXES[name]
    z_obj = gc.GEOM["z_object"]
    gen = photon.sources_piv(gc.EXTENT_SEED, gc.EXTENT_N, lo, hi, z_obj, *gc.SHEET, gc.CDF)
    near = photon.sources_piv(gc.EXTENT_SEED, gc.EXTENT_N, near_lo, near_hi, z_obj, *gc.SHEET, gc.CDF)
    try:
        assert_extent_keeps_the_light(photon, gc.extent_call(), gen, near, axis)
    finally:
        gen.free()
        near.free()


@pytest.mark.parametrize("name", ["x_low", "y_high"])
def test_extent_of_a_sheet_carried_towards_the_lens(photon, name):
    """photon_sources_piv_advected: a uniform w carries the sheet 4e5 um towards the lens, from 7.0e5 to 3.0e5 um in front
    of the aim plane.  The nearer the sources, the more lens samples can reach the aperture (the cull's dz rmax / dmin term:
    520 live samples against 506 for this lens and rmax = 2e5), so the z range of the handle has to be that of the stored
    particles, and its |x|, |y| the block reduction's over an off-centre field.  (The radiance is the sheet's profile at the new
    Z: a sheet of the usual 730 um would leave the moved particles dark, so this one is 2e6 um thick.)"""
    lo, hi, _, _, axis = gc.EXTENT_BOXES[name]
    z_obj = gc.GEOM["z_object"]
    shift = -4.0e5
    sheet = (2.0e6, 500.0)
    flow = photon.flow_from_grid(*pp.uniform_flow((0.0, 0.0, shift), lo, hi, 2))
    try:
        gen, world = photon.sources_piv_advected(gc.EXTENT_SEED, gc.EXTENT_N, lo, hi, z_obj, *sheet, gc.CDF, flow=flow, t=1.0,
                                                 steps=2, return_world=True)
    finally:
        flow.free()
    frame1 = photon.sources_piv(gc.EXTENT_SEED, gc.EXTENT_N, lo, hi, z_obj, *sheet, gc.CDF)     # the box, where the sheet was
    try:
        start = frame1.download()
        d = assert_extent_keeps_the_light(photon, gc.extent_call(), gen, frame1, axis)
    finally:
        gen.free()
        frame1.free()
    assert np.array_equal(d["x"], start["x"]) and np.array_equal(d["y"], start["y"])
    assert np.abs((d["z"].astype(np.float64) - start["z"]) - shift).max() < 0.1          # (f32 z of 8e5: 1/16 um steps)


# ---- 4. post-processing -----------------------------------------------------------------------------------------------
class Post:
    """One image on the device and a picture buffer prefilled with a sentinel."""
    SENTINEL = 0x5A5A

    def __init__(self, photon, raw):
        import torch
        self.torch, self.photon = torch, photon
        self.raw = np.ascontiguousarray(raw, np.float32)
        self.h, self.w = self.raw.shape
        self.out = torch.empty(self.h * self.w, dtype=torch.int16, device="cuda")
        self.reload()

    def reload(self):
        self.image = self.torch.from_numpy(self.raw.copy()).cuda()

    def run(self, gain, depth, rescale=True, **kw):
        self.out.fill_(self.SENTINEL)
        rows, cols = self.photon.postprocess_u16(self.image.data_ptr(), self.w, self.h, self.out.data_ptr(), gain, depth, rescale, **kw)
        flat = self.out.cpu().numpy().view(np.uint16)
        assert (flat[rows * cols:] == self.SENTINEL).all()              # nothing written behind the picture
        return flat[:rows * cols].reshape(rows, cols)

    def downloaded(self):
        return self.image.cpu().numpy().reshape(self.h, self.w)


def model(raw, gain, depth, rescale=True):
    with np.errstate(invalid="ignore"):
        return postprocess_image(raw, gain, depth, rescale)


@pytest.mark.parametrize("shape", [gc.POST_SMALL, gc.POST_LARGE], ids=["37x53", "725x725"])
def test_postprocess_equals_the_numpy_mirror_at_every_depth_and_gain(photon, shape):
    raw = gc.post_image(shape)
    p = Post(photon, raw)
    for depth in gc.POST_DEPTHS:
        for gain in gc.POST_GAINS:
            got, want = p.run(gain, depth), model(raw, gain, depth)
            assert got.shape == shape and np.array_equal(got, want), (depth, gain, int((got != want).sum()))
            assert want.max() >= 65534 and 2 <= len(np.unique(want)) <= 2 ** depth     # (the model did quantise)
    assert np.array_equal(bits(p.downloaded()), bits(raw))              # without noise the raw image is only read
    # rescaling off: clip and convert only (finite pixels: the conversion of the others is undefined in C and numpy alike)
    finite = gc.post_finite(raw)
    q = Post(photon, finite)
    got, want = q.run(25.0, 12, False), model(finite, 25.0, 12, False)
    assert np.array_equal(got, want) and np.array_equal(want, np.where(finite > 0, np.trunc(finite), 0).astype(np.uint16))


def test_postprocess_rounds_ties_to_even(photon):
    img, at, k = gc.tie_image()
    got = Post(photon, img).run(0.0, 8)
    assert np.array_equal(got, model(img, 0.0, 8))
    assert np.array_equal(got.reshape(-1)[at], (257 * np.where(k % 2 == 0, k, k + 1)).astype(np.uint16))


def test_postprocess_of_an_image_with_no_positive_pixel(photon):
    dark = gc.dark_image()
    p = Post(photon, dark)
    for depth, gain in ((10, 25.0), (1, -6.0), (16, 0.0)):
        got = p.run(gain, depth)
        assert got.shape == dark.shape and not got.any(), (depth, gain)
    assert not p.run(0.0, 10, False).any()
    assert np.array_equal(bits(p.downloaded()), bits(dark))


def test_postprocess_without_rescaling_wraps_beyond_u16(photon):
    """np.uint16(I) of the reference on values beyond 65535: the kernel's comment (photon_post.hip) promises truncation
    and the low 16 bits, as numpy's cast through int64 gives.  The expectation is written out (generator_cases.wrapped_u16):
    a direct float -> uint16 cast out of range is undefined in C, and numpy's is C's."""
    img = gc.wrap_image()
    got = Post(photon, img).run(0.0, 10, False)
    assert np.array_equal(got, gc.wrapped_u16(img))


@pytest.mark.parametrize("shape", [gc.POST_SMALL, (36, 52)], ids=["37x53", "36x52"])
def test_postprocess_crops(photon, capfd, shape):
    rows, cols = shape
    raw = gc.post_image(shape)
    p = Post(photon, raw)
    full = model(raw, 25.0, 10)
    legal, refused = gc.crop_requests(rows, cols)
    for r, c in legal:
        rs, cs = crop_window(rows, cols, r, c)
        got = p.run(25.0, 10, crop_rows=r, crop_cols=c)
        assert got.shape == (rs.stop - rs.start, cs.stop - cs.start) == (r // 2 * 2 - 1, c // 2 * 2 - 1), (r, c)
        assert np.array_equal(got, full[rs, cs]), (r, c)                # normalised to the brightest pixel of the WHOLE image
    for r, c in ((rows, 0), (0, cols), (5, 0), (0, 7)):                 # one of the two 0: no crop
        assert np.array_equal(p.run(25.0, 10, crop_rows=r, crop_cols=c), full), (r, c)
    capfd.readouterr()
    for r, c in refused:
        p.out.fill_(p.SENTINEL)
        with pytest.raises(Exception):
            photon.postprocess_u16(p.image.data_ptr(), cols, rows, p.out.data_ptr(), 25.0, 10, True, crop_rows=r, crop_cols=c)
        err = capfd.readouterr().err
        assert len(err.strip().splitlines()) == 1 and "photon_postprocess_u16" in err, (r, c, err)
        assert (p.out.cpu().numpy().view(np.uint16) == p.SENTINEL).all(), (r, c)
    assert np.array_equal(bits(p.downloaded()), bits(raw))


@pytest.mark.parametrize("shape", [gc.POST_SMALL, gc.POST_LARGE], ids=["37x53", "725x725"])
def test_postprocess_noise_pixel_by_pixel(photon, oracle, shape):
    """Pixel i gets n0 of Philox(noise_seed, counter i, draw 0, PHOTON_STREAM_IMAGE_NOISE) times 100 image_noise, added to
    the raw image in place; the picture is made of that noisy image.  Tolerance: generator_cases.noise_expectation."""
    seed = 3
    raw = gc.post_image(shape)
    n0 = oracle.normal2(seed, raw.size, draw=0, stream=gc.PHOTON_STREAM_IMAGE_NOISE)[:, 0]
    exact, tol = gc.noise_expectation(raw, n0)
    p = Post(photon, raw)
    picture = p.run(25.0, 10, image_noise=gc.POST_NOISE, noise_seed=seed)
    noisy = p.downloaded()
    finite = np.isfinite(raw)
    assert np.array_equal(np.isnan(noisy), np.isnan(raw)) and np.array_equal(noisy[~finite & ~np.isnan(raw)], raw[~finite & ~np.isnan(raw)])
    err = np.abs(noisy[finite].astype(np.float64) - exact[finite])
    assert (err <= tol[finite]).all(), (int((err > tol[finite]).sum()), float((err / tol[finite]).max()))
    assert (noisy[finite] != raw[finite]).mean() > 0.99
    assert np.array_equal(picture, model(noisy, 25.0, 10))
    if shape != gc.POST_SMALL:
        return
    # one seed, fresh copies: the same bytes; another seed: others; a crop leaves every pixel its own draw
    p.reload()
    again = p.run(25.0, 10, image_noise=gc.POST_NOISE, noise_seed=seed)
    assert np.array_equal(again, picture) and np.array_equal(bits(p.downloaded()), bits(noisy))
    p.reload()
    other = p.run(25.0, 10, image_noise=gc.POST_NOISE, noise_seed=seed + 1)
    assert not np.array_equal(other, picture) and (p.downloaded()[finite] != noisy[finite]).mean() > 0.99
    p.reload()
    rs, cs = crop_window(*shape, 12, 21)
    cropped = p.run(25.0, 10, image_noise=gc.POST_NOISE, noise_seed=seed, crop_rows=12, crop_cols=21)
    assert np.array_equal(bits(p.downloaded()), bits(noisy)) and np.array_equal(cropped, picture[rs, cs])
