"""Host-side logic without a GPU: marshalling mirror, sensor post-processing, scene helpers,
NRRD round trip, source sharding."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from photon_amd import scenes
from photon_amd.ray_tracing import (postprocess_image, read_tiff_u16, save_images, single_lens_camera,
                                    write_tiff_u16)
from photon_amd.sharding import shard_range


@pytest.mark.parametrize("case", ["piv", "bos_im1", "bos_im2"])
def test_postprocess_matches_reference(case):
    """uint16 image the reference's post-processing (perform_ray_tracing_03.py:2190-2247) made of a
    synthetic raw image == ours, pixel for pixel."""
    a = np.load(os.path.join(GOLDEN, f"postprocess_{case}.npz"))
    with open(os.path.join(GOLDEN, f"abi_{case}.json")) as f:
        pp = json.load(f)["postprocess"]
    shape = tuple(int(v) for v in a["shape"])
    raw = np.zeros(shape[0] * shape[1], np.float32)
    raw[a["raw_index"]] = a["raw_value"]
    out = postprocess_image(raw.reshape(shape), pp["pixel_gain"], int(pp["pixel_bit_depth"]),
                            pp["intensity_rescaling"], pp["image_noise"])
    ref = np.zeros(shape[0] * shape[1], np.uint16)
    ref[a["out_u16_index"]] = a["out_u16_value"]
    assert out.dtype == np.uint16 and np.array_equal(out.reshape(-1), ref)


def test_single_lens_camera_matches_reference_numbers():
    """Values the reference derives for its sample lens (captured via its marshalling code)."""
    g = single_lens_camera(105000.0, 8.0, 700000.0, 100000.0)
    with open(os.path.join(GOLDEN, "abi_bos_im1.json")) as f:
        j = json.load(f)
    a = np.load(os.path.join(GOLDEN, "abi_bos_im1.npz"))
    assert g["lens_pitch"] == j["scalars"]["lens_pitch"]
    assert g["image_distance"] == pytest.approx(j["scalars"]["image_distance"], rel=1e-15)
    eg = j["elements"][0]["element_geometry"]
    assert g["element"]["element_geometry"]["vertex_distance"] == pytest.approx(eg["vertex_distance"], rel=1e-14)
    assert g["element"]["element_properties"]["refractive_index"] == pytest.approx(
        j["elements"][0]["element_properties"]["refractive_index"], rel=1e-14)
    assert np.allclose(g["element_center"], a["element_center"], rtol=1e-14)
    assert np.allclose(g["element_plane_parameters"], a["element_plane_parameters"], rtol=1e-14)
    assert np.float32(g["z_offset"]) == np.float32(j["source"]["z_offset"])
    assert np.float32(g["z_object"]) == a["src_z"][0]      # BOS sources sit on the object plane


def test_nrrd_round_trip(tmp_path):
    rho, sp, org = scenes.bos_volume(16)
    p = scenes.write_nrrd(str(tmp_path / "v.nrrd"), rho, sp, org)
    r2, sp2, org2 = scenes.read_nrrd(p)
    assert np.array_equal(rho, r2) and list(sp2) == list(sp) and list(org2) == list(org)
    # the reference's own sample file parses too
    r, sp, org = scenes.read_nrrd(os.path.join(GOLDEN, "sample-density.nrrd"))
    assert r.shape == (64, 64, 64) and sp == [519.5459, 519.5459, 519.5]
    assert org == [-16365.714, -16365.714, 733634.3]


def test_scene_sizes():
    c3 = scenes.bos_scene()
    assert c3.num_sources == 20000 and c3.num_rays == 10_000_000 and c3.camera["implement_diffraction"]
    c2 = scenes.piv_scene()
    assert c2.num_rays == 1_000_000 and c2.scattering_irradiance.shape == (255, 27)
    c0 = scenes.config("C0")
    assert c0.num_rays == 10_000 and c0.scattering_type == "diffuse"


def test_shard_range_partitions_exactly():
    for n in (0, 1, 7, 20000, 1_000_003):
        for w in (1, 2, 3, 8):
            parts = [shard_range(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in parts]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


def test_tiff_and_raw_writers_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    raw = rng.gamma(2.0, 3.0, size=(37, 53)).astype(np.float32)
    u16 = postprocess_image(raw, 25.0, 10)
    tif, binf = str(tmp_path / "a.tif"), str(tmp_path / "a.bin")
    save_images(raw, u16, tif, binf)
    assert np.array_equal(read_tiff_u16(tif), u16)
    assert np.array_equal(np.fromfile(binf, np.float32).reshape(raw.shape), raw)
    # the reference's vendored tifffile is not shipped with the tests; check the header by hand
    with open(tif, "rb") as f:
        assert f.read(4) == b"II*\x00"
    write_tiff_u16(str(tmp_path / "odd.tif"), np.arange(15, dtype=np.uint16).reshape(3, 5))
    assert np.array_equal(read_tiff_u16(str(tmp_path / "odd.tif")), np.arange(15).reshape(3, 5))


def test_march_work_queues_partition_every_launch():
    """The work queues of the persistent march (8 XCDs x 4 sub-queues): for any number of 64-ray groups every group
    below it is handed out by exactly one queue, each queue hands its groups out in increasing order (so the first one
    past the end ends the queue), and the consecutive groups of a chunk (16 groups for the tricubic kernels, 128 for the
    trilinear ones) come from ONE queue (L2 locality).  Host restatement of the kernel's own functions, through the C-ABI; no
    GPU needed."""
    import ctypes
    from photon_amd import build
    from photon_amd.library import apply_signatures
    lib = apply_signatures(ctypes.CDLL(build.build_library(verbose=False)))
    f = lib.photon_march_queue_group
    size = lib.photon_march_queue_size
    subs = lib.photon_march_queue_count() // 8
    assert subs == 4 and lib.photon_march_queue_chunk(2) == 16 and lib.photon_march_queue_chunk(1) == 128
    bad = 0xFFFFFFFF
    assert f(0, 8, 0, 16) == bad and f(0, 0, subs, 16) == bad and size(100, 0, subs, 16) == bad     # out of range: refused, not aliased
    assert f(0, 0, 0, 24) == bad and size(100, 0, 0, 0) == bad                                       # chunks are powers of two
    for C in (16, 128):
        for n_groups in (1, C - 1, C, C + 1, 1023, 8 * C + 5, 32 * C - 1, 32 * C, 64 * C, 64 * C + 1, 19532):
            seen = np.zeros(n_groups, np.int32)
            for x in range(8):
                for sub in range(subs):
                    last, k = -1, 0
                    while True:
                        g = f(k, x, sub, C)
                        assert g > last                    # monotonic: a queue ends at its first group past the launch
                        last = g
                        if g >= n_groups:
                            break
                        seen[g] += 1
                        assert (g // C) % 8 == x and (g // C // 8) % subs == sub
                        k += 1
                    # a segmented launch hands out size x S items per queue (item k = segment k // size of group k % size):
                    # the closed form counts exactly the groups the queue's own enumeration finds below the launch's end
                    assert k == size(n_groups, x, sub, C), (n_groups, x, sub, C)
            assert (seen == 1).all(), (n_groups, C)


def test_march_segments_plan():
    """How many pieces the library cuts a ray's march into (photon_march_segments_plan: pure host arithmetic, the cost model
    of DESIGN.md section 4.1 fitted to tools/segments_sweep.sh).  Pins the plan of the configurations that were measured: the
    measured optima were 4 (equal) / 4-5 (halving) pieces for the C3 job with the tricubic sampler and 12-16 for one GPU's
    eighth of it; with the trilinear sampler (as of the end of round 4) whole marches and 3 pieces; fast kernels and small
    launches march whole."""
    import ctypes
    from photon_amd import build
    from photon_amd.library import apply_signatures
    lib = apply_signatures(ctypes.CDLL(build.build_library(verbose=False)))
    plan = lib.photon_march_segments_plan

    def p(rays, depth, algo, interp, cus=256):
        h = ctypes.c_int(-1)
        return plan(rays, depth, algo, interp, cus, ctypes.byref(h)), h.value

    os.environ.pop("PHOTON_MARCH_SEGMENT_SHAPE", None)
    assert p(10_000_000, 256, 2, 2) in ((4, 1), (5, 1))          # C3 headline: 30.5 chip fills -> halving pieces
    assert p(10_000_000, 256, 2, 1) == (1, 0)                    # the same with the trilinear sampler: whole (measured best, 1 < 2 < 3)
    s, h = p(1_250_000, 256, 2, 2)                               # one GPU's eighth: 3.8 fills -> equal pieces, many
    assert h == 0 and 10 <= s <= 16
    s, h = p(1_250_000, 256, 2, 1)
    assert h == 0 and 3 <= s <= 4                                # measured optimum 3
    assert p(10_000_000, 256, 1, 1) == (1, 0)                    # Euler trilinear: a march of 0.2 ms is not worth a hand-off
    assert p(300_000, 256, 2, 2) == (1, 0)                       # less than 1.25 chip fills: whole marches
    assert p(100_000_000 // 2, 512, 2, 2)[0] >= 2                # one launch of C4
    assert p(10_000_000, 8, 2, 2)[0] <= 2                        # the shortest piece is 4 trips
    assert plan(10_000_000, 256, 3, 2, 256, None) == 0           # integrators 3 / 4 are not segmented: refused


# ---- the plan of a march launch (photon_march_launch_plan: the planner every launch goes through, host arithmetic) ----
_SWEEP_RAYS = [64 * k for k in (1, 100, 5000, 6399, 6400, 6401, 7680, 20000, 156250, 1048576)]
_SWEEP_DEPTHS = (4, 8, 16, 48, 128, 256, 512, 1024)
DUMPS, NOISE, LENS_MAJOR = 1, 2, 4             # flags of photon_march_launch_plan
UNIFORM, HALVING, TAPER = 0, 1, 2


@pytest.fixture()
def march_plan(monkeypatch):
    """f(n_rays, dims, algorithm, interpolation, num_cus=256, scene_segments=-1, flags=0) -> photon_march_plan_t, with
    the two environment variables of the planner unset."""
    import ctypes
    from photon_amd import build
    from photon_amd.library import apply_signatures, bind_march_launch_plan
    monkeypatch.delenv("PHOTON_MARCH_SEGMENTS", raising=False)
    monkeypatch.delenv("PHOTON_MARCH_SEGMENT_SHAPE", raising=False)
    lib = apply_signatures(ctypes.CDLL(build.build_library(verbose=False)))
    plan = bind_march_launch_plan(lib)
    old = lib.photon_march_segments_plan

    def segments_plan(rays, depth, algo, interp, cus):
        h = ctypes.c_int(-1)
        return old(rays, depth, algo, interp, cus, ctypes.byref(h)), h.value
    plan.segments_plan = segments_plan
    return plan


def _boundaries(p):
    return [p.seg_begin[k] for k in range(p.segments + 1)]


def _check_boundaries(p, depth, what):
    b = _boundaries(p)
    assert b[0] == 0 and b[-1] == depth, (what, b)
    if p.segments > 1:
        assert min(np.diff(b)) >= 4, (what, b)
    assert p.segmented == (p.segments > 1), what


def test_march_launch_plan_agrees_with_segments_plan(march_plan):
    """With no scene setting and no environment, the launch plan's pieces are those photon_march_segments_plan reports, over
    launches below, at and above 1.25 chip fills of every kernel's wave count (960 plans); and every plan's boundaries run from
    0 to the depth in pieces of at least 4 trips."""
    for rays in _SWEEP_RAYS:
        for depth in _SWEEP_DEPTHS:
            for algo in (1, 2):
                for interp in (1, 2):
                    for cus in (64, 256, 304):
                        p = march_plan(rays, depth, algo, interp, cus)
                        what = (rays, depth, algo, interp, cus)
                        assert (p.segments, int(p.shape == HALVING)) == march_plan.segments_plan(*what), what
                        _check_boundaries(p, depth, what)


def test_march_launch_plan_forced_counts_keep_their_boundaries(march_plan, monkeypatch):
    for forced in (2, 5, 64):
        monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", f"force:{forced}")
        for rays in _SWEEP_RAYS:
            for depth in _SWEEP_DEPTHS:
                for algo, interp in ((1, 1), (2, 1), (1, 2), (2, 2)):
                    p = march_plan(rays, depth, algo, interp)
                    assert 1 <= p.segments <= forced
                    _check_boundaries(p, depth, (forced, rays, depth, algo, interp))
                    if depth >= 4 * forced and p.shape == UNIFORM:
                        assert p.segments == forced, (forced, rays, depth, algo, interp)


@pytest.mark.parametrize("rays, depth, algo, interp, segments, shape", [
    (10_000_000, 256, 2, 2, 4, HALVING),
    (10_000_000, 256, 2, 1, 1, UNIFORM),
    (1_250_000, 256, 2, 2, 11, UNIFORM),
    (1_250_000, 256, 2, 1, 4, UNIFORM),
    (2_000_000, 128, 2, 2, 6, UNIFORM),
    (50_000_000, 512, 2, 2, 3, HALVING),
    (10_000_000, 256, 1, 2, 3, HALVING),
    (5_000_000, 256, 2, 2, 5, HALVING),
    (5_000_000, 256, 2, 1, 2, HALVING),
    (12_032, 48, 2, 2, 1, UNIFORM),
])
def test_march_launch_plan_pins(march_plan, rays, depth, algo, interp, segments, shape):
    """The plans the library made before the planner was one function (256 compute units, depth^3 texels)."""
    p = march_plan(rays, depth, algo, interp)
    assert (p.segments, p.shape) == (segments, shape)
    assert p.segmented == (segments > 1) and p.save == 0 and p.noise == 0 and p.persistent == 1


def test_march_launch_plan_piece_boundaries(march_plan, monkeypatch):
    assert _boundaries(march_plan(10_000_000, 256, 2, 2)) == [0, 128, 192, 224, 256]       # halving, the last two equal
    monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", "force:3")
    p = march_plan(12_032, 256, 2, 2)
    assert _boundaries(p) == [0, 85, 171, 256] and p.shape == UNIFORM
    monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", "force:5")
    assert _boundaries(march_plan(12_032, 8, 2, 2)) == [0, 4, 8]                             # no piece shorter than 4 trips


def test_march_launch_plan_knobs(march_plan, monkeypatch):
    """The scene's setting beats PHOTON_MARCH_SEGMENTS; force: and an explicit count segment launches of any size;
    PHOTON_MARCH_SEGMENT_SHAPE overrides the shape."""
    monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", "1")
    assert march_plan(10_000_000, 256, 2, 2).segments == 1
    monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", "force:5")
    assert march_plan(12_032, 256, 2, 2).segments == 5
    monkeypatch.setenv("PHOTON_MARCH_SEGMENTS", "force:7")
    assert march_plan(12_032, 256, 2, 2, scene_segments=3).segments == 3
    assert march_plan(12_032, 256, 2, 2, scene_segments=1).segments == 1
    assert march_plan(10_000_000, 256, 2, 2, scene_segments=1).segments == 1
    monkeypatch.delenv("PHOTON_MARCH_SEGMENTS")
    monkeypatch.setenv("PHOTON_MARCH_SEGMENT_SHAPE", "uniform")
    p = march_plan(10_000_000, 256, 2, 2)
    assert p.shape == UNIFORM and p.segments > 1 and len(set(np.diff(_boundaries(p)))) <= 2     # equal up to rounding
    monkeypatch.setenv("PHOTON_MARCH_SEGMENT_SHAPE", "taper:2")
    p = march_plan(10_000_000, 256, 2, 2)
    assert p.shape == TAPER and p.segments > 1
    _check_boundaries(p, 256, "taper:2")


def test_march_launch_plan_exclusions(march_plan):
    """Dumps and gradient noise index a ray's iterations: such launches march whole, even when a count is forced.  (The
    tricubic branches record no intermediate dumps: with them the flag changes nothing, save stays 0.)  The integrators
    other than Euler and RK4 run one thread per ray after a ray-generation kernel."""
    n = 12_032
    for algo in (1, 2):
        p = march_plan(n, 48, algo, 1, scene_segments=5, flags=DUMPS)
        assert (p.segments, p.segmented, p.save, p.noise) == (1, 0, 1, 0)
        for interp in (1, 2):
            p = march_plan(n, 48, algo, interp, scene_segments=5, flags=NOISE)
            assert (p.segments, p.segmented, p.save) == (1, 0, 0) and p.noise == int(algo == 1 and interp == 1)
            p = march_plan(10_000_000, 256, algo, interp, flags=NOISE)
            assert (p.segments, p.segmented) == (1, 0)
            p = march_plan(n, 48, algo, interp, scene_segments=5, flags=DUMPS | NOISE)
            assert (p.segments, p.segmented) == (1, 0)
            assert march_plan(n, 48, algo, interp, scene_segments=5).segments == 5
        p = march_plan(10_000_000, 256, algo, 1, flags=DUMPS)
        assert (p.segments, p.segmented, p.save) == (1, 0, 1)
        assert march_plan(n, 48, algo, 2, scene_segments=5, flags=DUMPS).save == 0
    for algo in (0, 3, 4):
        for interp in (1, 2):
            for rays in (1, 255, 256, 257, n, 10_000_000):
                p = march_plan(rays, 256, algo, interp, scene_segments=5)
                assert (p.persistent, p.grid_blocks, p.block_threads) == (0, (rays + 255) // 256, 256)
                assert (p.segments, p.segmented, p.generates_rays) == (1, 0, 0)


def test_march_launch_plan_grid_and_chunks(march_plan):
    for algo in (1, 2):
        for interp in (1, 2):
            for cus in (64, 256, 304):
                for rays in (1, 256, 257, 12_032, 256 * 8 * cus - 1, 256 * 8 * cus, 256 * 8 * cus + 1, 10_000_000):
                    p = march_plan(rays, 256, algo, interp, cus)
                    assert p.grid_blocks == min((rays + 255) // 256, 8 * cus) and p.block_threads == 256
                    assert p.persistent == 1 and p.generates_rays == 1
        # queue chunks: 16 groups for the tricubic kernels in source-major launches through at most 2^24 texels, else 128
        assert march_plan(10_000_000, 256, algo, 2).groups_per_chunk == 16
        assert march_plan(10_000_000, (128, 256, 512), algo, 2).groups_per_chunk == 16
        assert march_plan(10_000_000, (257, 256, 256), algo, 2).groups_per_chunk == 128
        assert march_plan(10_000_000, 256, algo, 2, flags=LENS_MAJOR).groups_per_chunk == 128
        for dims in (48, 256, (257, 256, 256)):
            for flags in (0, LENS_MAJOR):
                assert march_plan(10_000_000, dims, algo, 1, flags=flags).groups_per_chunk == 128
