"""tests/generator_cases.py without a GPU: that the inputs of tests/test_generators_gpu.py have the properties those tests
rest on -- no axis of the Gaussian cases can stand in for another, the particles of the flow case leave the grid through
every face and each mistake the case is there for moves most of them, the tie pixels are ties -- the models against the
oracle, and the gzip payloads the NRRD parser has to refuse (host code of the library: no device is touched)."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

import generator_cases as gc
from photon_amd import piv_pairs as pp
from photon_amd.ray_tracing import crop_window, postprocess_image


# ---- 1. Gaussian volume -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.GAUSS_CASES))
def test_no_axis_of_the_gaussian_cases_can_stand_in_for_another(name):
    case = gc.GAUSS_CASES[name]
    nx, ny, nz = case["n"]
    rho = gc.gauss_rho(case)
    assert rho.shape == (nz, ny, nx) and rho.dtype == np.float32
    assert len({(n, s) for n, s in zip(case["n"], case["spacing"])}) == 3          # every axis its own (side, spacing)
    for a, n in enumerate(case["n"]):
        node = (case["centre"][a] - case["origin"][a]) / case["spacing"][a]
        assert 0.0 < node < n - 1 and abs(node - round(node)) > 0.15, (a, node)      # inside the grid, on no node
        assert abs(node - (n - 1) / 2.0) > 0.05 * (n - 1), (a, node)                 # and not in the middle
    for axes, other in gc.axis_permutations(rho).items():
        assert other.shape == rho.shape
        assert (other != rho).mean() > 0.5, (axes, float((other != rho).mean()))
    if name == "7x12x9":
        assert 2 * 256 < rho.size < 3 * 256                                          # three blocks, the last one partial


@pytest.mark.parametrize("name", list(gc.GAUSS_CASES))
def test_the_gaussian_model_is_the_oracles_density(oracle, name):
    """The oracle's texel w is K rho with rho rounded to f32 first (loadNRRD's scaling, one f32 product): dividing it out
    again is not exact, so the model goes through the same product and is compared at the last ulp of exp."""
    case = gc.GAUSS_CASES[name]
    v = oracle.volume_gaussian(*gc.gauss_args(case), 1)
    try:
        w = v.download()[..., 3]
        info = v.info()
    finally:
        v.free()
    np.testing.assert_allclose(w, np.float32(0.225e-3) * gc.gauss_rho(case), rtol=3e-7)
    assert (info.nx, info.ny, info.nz) == case["n"]
    assert info.step_size == np.float32(min(case["spacing"]))
    lo = [case["origin"][0], case["origin"][1], case["origin"][2] - 750e3]
    assert list(info.min_bound) == [np.float32(x) for x in lo]
    assert list(info.max_bound) == [np.float32(lo[a] + (case["n"][a] - 1) * case["spacing"][a]) for a in range(3)]


# ---- 2. flow sampler --------------------------------------------------------------------------------------------------
def _positions_changed(a, b):
    return float(((a["x"] != b["x"]) | (a["y"] != b["y"]) | (a["z"] != b["z"])).mean())


def test_the_flow_case_leaves_the_grid_through_every_face_and_sees_each_mistake():
    flow = gc.noise_flow()
    assert flow[0].shape == (3, 5, 7) and len({a.tobytes() for a in flow[:3]}) == 3
    start = pp.piv_field(gc.FLOW_SEED, gc.FLOW_N, gc.BOX_LO, gc.BOX_HI, gc.Z_OBJ, *gc.SHEET)["world"]
    want = gc.flow_advect(flow)
    for world in (start, want["world"]):                                 # at the first sample and at the last
        shares = gc.beyond_faces(world)
        assert min(shares.values()) >= 0.10, shares
    assert np.isfinite(want["world"]).all() and np.isfinite(want["radiance"]).all()
    right = gc.flow_advect(flow, clamp_weight=True, y_stride_is_ny=False)           # the variant code with no mistake in it
    for key in want:
        assert np.array_equal(right[key], want[key]), key
    with np.errstate(over="ignore", invalid="ignore"):                   # (extrapolated velocities run away)
        unclamped = gc.flow_advect(flow, clamp_weight=False)
    assert _positions_changed(unclamped, want) > 0.5
    assert _positions_changed(gc.flow_advect(flow, y_stride_is_ny=True), want) > 0.5
    with_cdf = gc.flow_advect(flow, gc.CDF)
    assert np.array_equal(with_cdf["world"], want["world"]) and len(np.unique(with_cdf["diameter_index"])) == 27


def test_the_nan_node_case_has_nan_particles_and_mostly_finite_ones():
    flow = gc.noise_flow(nan_node=gc.NAN_NODE)
    k, j, i = gc.NAN_NODE
    nz, ny, nx = flow[0].shape
    assert 0 < k < nz - 1 and 0 < j < ny - 1 and 0 < i < nx - 1          # interior
    assert np.isnan(flow[0]).sum() == 1 and not np.isnan(flow[1]).any() and not np.isnan(flow[2]).any()
    got = gc.flow_advect(flow)
    nan = np.isnan(got["world"]).any(axis=1)
    assert nan.sum() >= 1 and (~nan).sum() >= gc.FLOW_N // 2, (int(nan.sum()), int((~nan).sum()))
    assert np.array_equal(np.isnan(got["x"]), nan)                       # the stored x carries it: the extent sees it
    # a particle the NaN never reached moved exactly as in the clean field
    clean = gc.flow_advect(gc.noise_flow())
    assert (~nan & (got["world"] == clean["world"]).all(axis=1)).sum() > gc.FLOW_N // 4


def test_the_model_follows_photon_det_exp_where_it_underflows(oracle):
    """Particles the flow case carries 13e3 um off a sheet of sigma = 310 um: photon_det_exp returns 0 below -708
    (include/photon_det_math.h), numpy's exp not before -745.  The model has the oracle's zeros there and stays within
    RADIANCE_ULP of it everywhere else."""
    n = 40_000
    lo, hi = (-1.0e3, -1.0e3, -1.4e4), (1.0e3, 1.0e3, 1.4e4)
    got = pp.piv_field(5, n, lo, hi, gc.Z_OBJ, *gc.SHEET)
    want = oracle.sources_piv(5, n, lo, hi, gc.Z_OBJ, *gc.SHEET)
    sigma = gc.SHEET[0] / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    arg = -got["world"][:, 2] ** 2 / (2.0 * sigma ** 2)
    between = (arg < -708.0) & (arg > -745.0)
    assert between.sum() > 100 and (np.exp(arg[between]) > 0).all()
    assert not got["radiance"][between].any() and not want["radiance"][between].any()
    assert np.array_equal(got["radiance"] == 0, want["radiance"] == 0)
    lit = want["radiance"] > 0
    assert (np.abs(got["radiance"][lit] - want["radiance"][lit]) / np.spacing(want["radiance"][lit])).max() <= pp.RADIANCE_ULP


def test_the_smallest_grid_has_unequal_sides():
    flow = gc.noise_flow((2, 3, 5))
    assert flow[0].shape == (2, 3, 5)
    got = gc.flow_advect(flow)
    assert np.isfinite(got["world"]).all() and min(gc.beyond_faces(got["world"]).values()) >= 0.10


# ---- 3. extents -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.EXTENT_BOXES))
def test_the_extent_boxes_are_off_centre_and_keep_particles_in_view(name):
    lo, hi, near_lo, near_hi, axis = gc.EXTENT_BOXES[name]
    assert max(abs(lo[axis]), abs(hi[axis])) == 10 * min(abs(lo[axis]), abs(hi[axis]))
    assert max(abs(near_lo[axis]), abs(near_hi[axis])) == min(abs(lo[axis]), abs(hi[axis]))
    other = 1 - axis
    assert lo[other] == -hi[other] and lo[2] == -hi[2]
    w = pp.piv_field(gc.EXTENT_SEED, gc.EXTENT_N, lo, hi, gc.GEOM["z_object"], *gc.SHEET, gc.CDF)["world"]
    assert np.abs(w[:, axis]).max() > 1.5e5 and (np.abs(w[:, axis]) < 4.0e4).sum() > 10


# ---- 4. post-processing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [gc.POST_SMALL, gc.POST_LARGE])
def test_the_post_images_hold_every_pixel_class(shape):
    img = gc.post_image(shape)
    flat = img.reshape(-1)
    assert img.shape == shape and img.dtype == np.float32
    assert np.isnan(flat).sum() == 1 and np.isposinf(flat).sum() == 1 and np.isneginf(flat).sum() == 1
    finite = np.isfinite(flat)
    assert 0.03 < (flat[finite] < 0).mean() < 0.07
    pos = flat[finite & (flat > 0)]
    assert pos.min() < 0.02 and pos.max() == 3.0e4 and pos.max() / pos.min() > 1e6
    brightest = int(np.argmax(np.where(finite, flat, -np.inf)))
    assert 0 < brightest < flat.size - 1
    if shape == gc.POST_LARGE:
        assert flat.size > 2048 * 256


def test_the_tie_pixels_are_exact_ties_and_round_to_even():
    img, at, k = gc.tie_image()
    flat = img.reshape(-1)
    assert flat.max() == 255.0 and 0 < int(np.argmax(flat)) < flat.size - 1
    v = flat[at]
    assert np.array_equal((np.float32(255.0) * v) / np.float32(255.0), v) and np.array_equal(v - np.floor(v), np.full(v.size, 0.5, np.float32))
    out = postprocess_image(img, 0.0, 8).reshape(-1)[at]
    assert (out % 257 == 0).all()
    level = out // 257
    even, odd = k % 2 == 0, k % 2 == 1
    assert (level[even] == k[even]).sum() >= 8 and (level[odd] == k[odd] + 1).sum() >= 8
    assert np.array_equal(level, np.where(even, k, k + 1))               # roundf would give k + 1 everywhere


def test_dark_wrap_and_crop_inputs():
    dark = gc.dark_image()
    assert not (dark > 0).any() and (dark < 0).any() and np.signbit(dark[dark == 0]).any() and not postprocess_image(dark, 25.0, 10).any()
    wrap = gc.wrap_image()
    want = gc.wrapped_u16(wrap)
    assert want.reshape(-1)[0] == 0 and want.reshape(-1)[2] == 65535 and len(np.unique(want)) > 1000
    assert np.array_equal(want, (wrap.astype(np.int64) % 65536).astype(np.uint16))       # f32 -> int64 is in range: defined
    for rows, cols in (gc.POST_SMALL, (36, 52)):
        legal, refused = gc.crop_requests(rows, cols)
        sizes = set()
        for r, c in legal:
            rs, cs = crop_window(rows, cols, r, c)
            assert 0 <= rs.start < rs.stop <= rows and 0 <= cs.start < cs.stop <= cols, (r, c)
            assert (rs.stop - rs.start, cs.stop - cs.start) == (r // 2 * 2 - 1, c // 2 * 2 - 1)
            sizes.add((rs.stop - rs.start, cs.stop - cs.start))
        assert (1, 1) in sizes and (2 * (rows // 2) - 1, 2 * (cols // 2) - 1) in sizes
        assert any(r % 2 and c % 2 for r, c in legal) and (rows, cols) in legal
        for r, c in refused:
            rs, cs = crop_window(rows, cols, r, c)
            assert rs.start < 0 or cs.start < 0 or rs.stop <= rs.start or cs.stop <= cs.start, (r, c)


def test_the_noise_expectation_is_exact_and_its_tolerance_is_two_half_ulps(oracle):
    raw = gc.post_image(gc.POST_SMALL)
    n0 = oracle.normal2(3, raw.size, draw=0, stream=gc.PHOTON_STREAM_IMAGE_NOISE)[:, 0]
    exact, tol = gc.noise_expectation(raw, n0)
    finite = np.isfinite(raw)
    assert np.array_equal(np.isfinite(exact), finite) and np.isnan(exact).sum() == 1
    s = np.float32(100.0 * gc.POST_NOISE)
    unfused = (n0.reshape(raw.shape) * s + raw)[finite]                              # numpy: two f32 roundings
    fused = (n0.reshape(raw.shape).astype(np.float64) * float(s) + raw.astype(np.float64)).astype(np.float32)[finite]
    for got in (unfused, fused):
        assert (np.abs(got.astype(np.float64) - exact[finite]) <= tol[finite]).all()
    assert (tol[finite] < 1e-6 * (np.abs(exact[finite]) + np.abs(exact[finite] - raw[finite]))).all()    # nothing but roundings
    delta = exact[finite] - raw[finite]
    assert abs(delta.std() - 6.25) < 0.4 and abs(delta.mean()) < 0.5
    # the draws the mistakes would use instead are other numbers
    other = oracle.normal2(3, raw.size, draw=0, stream=pp.PHOTON_STREAM_SCENE)[:, 0]
    n1 = oracle.normal2(3, raw.size, draw=0, stream=gc.PHOTON_STREAM_IMAGE_NOISE)[:, 1]
    seed = oracle.normal2(4, raw.size, draw=0, stream=gc.PHOTON_STREAM_IMAGE_NOISE)[:, 0]
    for wrong in (other, n1, seed, np.roll(n0, -1)):
        assert (wrong != n0).mean() > 0.99


# ---- 5. gzip payloads that lie ----------------------------------------------------------------------------------------
def test_lying_gzip_payloads_are_refused_by_the_parser(tmp_path, capfd):
    """photon_volume_load_nrrd parses on the host before it touches the device: a refused file returns 2 with one line on
    stderr, here as on a machine with a GPU.  (That the honest gzip, gz and zlib-wrapped files still load to the raw file's
    bits needs the device: tests/test_parity_gpu.py::test_nrrd_payload_encodings.)"""
    from photon_amd import build
    from photon_amd.library import apply_signatures
    lib = apply_signatures(ctypes.CDLL(build.build_library()))
    rng = np.random.default_rng(3)
    n = (12, 10, 14)
    little = (1.2 + 0.1 * rng.random(n)).astype("<f4").tobytes()
    header = (f"NRRD0005\ntype: float\ndimension: 3\nsizes: {n[2]} {n[1]} {n[0]}\nendian: little\nencoding: gzip\n"
              "spacings: 100 110 120\nspace origin: (-500,-400,300000)\n\n").encode()
    payloads = gc.lying_gzip_payloads(little)
    assert len(payloads) == 4
    for name, payload in payloads.items():
        # each of them holds the sizes' worth of the right bytes (the deflate stream behind the 10-byte gzip header, read
        # without its trailer): a reader that stops there and looks no further accepts it
        assert zlib.decompressobj(-15).decompress(payload[10:], len(little)) == little, name
    with pytest.raises(Exception):
        gzip.decompress(payloads["crc_flipped"])
    with pytest.raises(Exception):
        gzip.decompress(payloads["isize_changed"])
    assert len(gzip.decompress(payloads["inflates_beyond_sizes"])) == len(little) + 400
    payloads["zlib_adler_flipped"] = zlib.compress(little)[:-1] + bytes([zlib.compress(little)[-1] ^ 0x10])
    payloads["trailer_cut"] = gzip.compress(little)[:-3]
    capfd.readouterr()
    for name, payload in payloads.items():
        path = tmp_path / f"{name}.nrrd"
        path.write_bytes(header + payload)
        h = ctypes.c_void_p()
        rc = lib.photon_volume_load_nrrd(str(path).encode(), 1, ctypes.byref(h))
        err = capfd.readouterr().err
        assert rc == 2 and not h.value, (name, rc)
        assert len(err.strip().splitlines()) == 1 and "failed to read NRRD" in err and "payload" in err, (name, err)
    # the honest streams get past the parser: whatever comes back is the volume build's answer (0 with a device), never the parser's 2
    for name, payload in (("gzip", gzip.compress(little)), ("zlib_wrapped", zlib.compress(little))):
        path = tmp_path / f"honest_{name}.nrrd"
        path.write_bytes(header + payload)
        h = ctypes.c_void_p()
        rc = lib.photon_volume_load_nrrd(str(path).encode(), 1, ctypes.byref(h))
        err = capfd.readouterr().err
        assert rc != 2 and "failed to read NRRD" not in err, (name, rc, err)
        if h.value:
            lib.photon_volume_free(h)
