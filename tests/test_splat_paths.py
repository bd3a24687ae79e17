"""CPU side of the splat-path tests (tests/test_splat_paths_gpu.py): the counter enum's Python mirror, the debug build's
reader, the scene families of tests/splat_families.py in the oracle -- that they light what they say, that the bars the GPU
tier asserts are met by the oracle against itself across thread counts -- and an independent numpy model of both splats
at the sensor's edges, from the formulas in device_optics.hpp's comments."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import splat_families as sf
from photon_amd import build as _build
from photon_amd import path_stats

F32 = np.float32
THREADS = (1, 5, 16)
# Share of lit pixels of an overlapping 4-pixel family that may differ at all between two summation orders (each by one
# f32 ulp at most).  The oracle against itself gives 0.034 % (1 of 2938).
MAX_DIFFERING_SHARE = 0.005


def ulp_distance(a, b):
    """Distance in f32 steps between same-signed finite values."""
    return np.abs(np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64))


def image_mismatch(fam, got, want, what="image"):
    """None when `got` meets the family's bar against `want`, else the report: how many pixels differ, the first one with its
    row, column and both values.  Erf and isolated 4-pixel families: bit-equal.  Overlapping 4-pixel families: the same
    pixels lit, every pixel within one f32 ulp, at most MAX_DIFFERING_SHARE of the lit pixels differing at all."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if not diff.any():
        return None
    r, c = np.argwhere(diff)[0]
    head = f"{fam.name} {what}: {int(diff.sum())} of {diff.size} pixels differ; first at row {r} column {c}: {got[r, c]!r} vs {want[r, c]!r}"
    if fam.erf or fam.isolated:
        return head
    if ((got != 0) != (want != 0)).any():
        r, c = np.argwhere((got != 0) != (want != 0))[0]
        return f"{head}; lit pixels differ, first at row {r} column {c}: {got[r, c]!r} vs {want[r, c]!r}"
    far = ulp_distance(got, want) > 1
    if far.any():
        r, c = np.argwhere(far)[0]
        return f"{head}; {int(far.sum())} pixels more than one ulp apart, first at row {r} column {c}: {got[r, c]!r} vs {want[r, c]!r}"
    share = diff.sum() / max(1, int((want != 0).sum()))
    if share > MAX_DIFFERING_SHARE:
        return f"{head}; {share:.4%} of the lit pixels differ (cap {MAX_DIFFERING_SHARE:.2%})"
    return None


def test_python_mirror_matches_the_header():
    assert path_stats.header_splat_slots() == path_stats.SPLAT_SLOTS


@pytest.fixture(scope="module")
def rendered(oracle, tmp_path_factory):
    """(families, {name: the oracle's render with every ray dumped})"""
    d = str(tmp_path_factory.mktemp("splat_paths"))
    fams = sf.build_families(oracle, d)
    return fams, {f.name: sf.oracle_render(oracle, f, d) for f in fams}, d


# ---- the numpy model ---------------------------------------------------------------------------------------------------
def erf_spot(call, path, d_x, d_y):
    """One ray's spot from the header's description of the erf splat: (rows, cols) of the pixels rendered and the product of
    the two erf differences there (f64).  Window, image clipping and radius test in f32, as the reference states them."""
    from scipy.special import erf
    cam = call.camera
    nx, ny, D = int(cam["x_pixel_number"]), int(cam["y_pixel_number"]), F32(cam["diffraction_diameter"])
    rfD = F32(sf.RENDER_FRACTION[path]) * D
    X, Y = F32(np.float64(d_x) - 0.5), F32(np.float64(d_y) - 0.5)
    c0, c1 = int(np.floor(X - rfD)), int(np.ceil(X + rfD))
    r0, r1 = int(np.floor(Y - rfD)), int(np.ceil(Y + rfD))
    cols, rows = np.arange(max(c0, 0), min(c1, nx - 1) + 1), np.arange(max(r0, 0), min(r1, ny - 1) + 1)
    C, R = np.meshgrid(cols, rows)
    ex, ey = C.astype(F32) - X, R.astype(F32) - Y                   # f32, like every step to the radius
    rad = np.sqrt(ex * ex + ey * ey)
    assert rad.dtype == F32
    keep = rad <= rfD
    s8 = np.float64(np.sqrt(F32(8.0)))

    def d_erf(e):
        e = e.astype(np.float64)
        return erf(s8 * (e - 0.5) / np.float64(D)) - erf(s8 * (e + 0.5) / np.float64(D))

    return R[keep], C[keep], (d_erf(ex) * d_erf(ey))[keep]


def taps_of_hit(call, x, y):
    """One hit's four taps from the header's description of the 4-pixel splat: (ii, jj, area weight) and the inside flag."""
    cam = call.camera
    nx, ny, pitch = int(cam["x_pixel_number"]), int(cam["y_pixel_number"]), F32(cam["pixel_pitch"])
    p1x, p1y = F32(-float(pitch) * (nx - 1) / 2.0), F32(-float(pitch) * (ny - 1) / 2.0)
    d_x, d_y = (F32(x) - p1x) / pitch, (F32(y) - p1y) / pitch
    inside = not (d_x >= nx or d_y >= ny or d_x < 0 or d_y < 0)
    lx, ly = F32(np.float64(d_x) - 0.5), F32(np.float64(d_y) - 0.5)
    wi, wj = np.float64(np.ceil(ly) - ly), np.float64(np.ceil(lx) - lx)
    ii, jj = int(np.ceil(ly)) - 1, int(np.ceil(lx)) - 1
    return [(ii, jj, wi * wj), (ii, jj + 1, wi * (1 - wj)), (ii + 1, jj, (1 - wi) * wj), (ii + 1, jj + 1, (1 - wi) * (1 - wj))], inside


def tap_index(ii, jj, nx, ny):
    """Where the reference adds tap (ii, jj): flat index (ii-1)*W + jj-1 -- a tap in column 0 lands in the last column of the
    row before -- or None: pixel outside the sensor, or the index before the image."""
    if ii < 0 or ii >= ny or jj < 0 or jj >= nx:
        return None
    k = (ii - 1) * nx + jj - 1
    return k if k >= 0 else None


def test_families_do_what_they_say(oracle, rendered):
    fams, out, _ = rendered
    assert any(f.call.camera["x_pixel_number"] != f.call.camera["y_pixel_number"] for f in fams)
    rows_lit = {}
    for f in fams:
        cam, o = f.call.camera, out[f.name]
        nx, ny = cam["x_pixel_number"], cam["y_pixel_number"]
        assert 64 <= nx <= 128 and 64 <= ny <= 128 and f.call.num_rays <= 1e5
        assert set(f.slots) <= set(path_stats.SPLAT_SLOTS), f.name
        img, lit = o["image"], int((o["image"] != 0).sum())
        assert 0 < o["rays_on_sensor"] < f.call.num_rays, f.name        # images straddle the sensor's edges
        assert np.isnan(o["pos"][:, 0]).sum() == f.call.num_rays - o["rays_on_sensor"], f.name
        d_x, d_y = sf.pixel_coords(f.call, o["pos"], f.path)
        on = ~np.isnan(d_x)
        if f.erf:
            if f.isolated:
                assert o["sensor_taps"] == lit, f.name                   # no pixel receives two increments
            if f.name.split("_")[0] in ("iso", "one", "two"):
                assert img[0].any() and img[-1].any() and img[:, 0].any() and img[:, -1].any(), f.name
                assert img[0, 0] and img[0, -1] and img[-1, 0] and img[-1, -1], f.name
                X, Y = d_x[on] - F32(0.5), d_y[on] - F32(0.5)
                assert (X < 8).any() and (X >= 8).any() and (Y < 8).any() and (Y >= 8).any(), f.name
                assert (X < 0).any() and (X > nx - 1.5).any() and (Y < 0).any() and (Y > ny - 1.5).any(), f.name
        else:
            ii, jj, w, inside = oracle.pixel_taps(cam, o["pos"][on, 0], o["pos"][on, 1])
            assert inside.all()
            if f.isolated:                                              # a tap of weight zero is counted and lights nothing
                landed = [[tap_index(a, b, nx, ny) is not None for a, b in zip(ri, rj)] for ri, rj in zip(ii, jj)]
                assert o["sensor_taps"] - int(((w == 0) & np.array(landed)).sum()) == lit, f.name
            if not f.name.startswith("taps_ulp"):
                assert (d_x[on] < 0.5).any() and (d_y[on] < 0.5).any(), f.name
                assert (jj == 0).any() and (jj == nx).any() and (ii == ny).any(), f.name   # column 0 (the wrap), taps beyond the last column and row
                assert img[:, nx - 1].any() and img[:, nx - 2].any() and img[ny - 2].any() and not img[ny - 1].any(), f.name
                rows_lit.setdefault((f.train, f.volume, f.noise_seed), []).append((img[0].any(), img[1].any()))
    for mode, lit in rows_lit.items():                                  # rows 0 and 1 of the image (hits in rows 1 and 2), in every kernel
        assert any(a for a, _ in lit) and any(b for _, b in lit), mode
    assert any(f.call.num_rays % sf.W for f in fams if not f.erf), "no 4-pixel family ends on a partial wave"
    for kind in ("erf", "taps"):
        group = [f for f in fams if f.erf == (kind == "erf")]
        assert any(f.train for f in group) and any(f.volume for f in group) and any(f.train and f.volume for f in group), kind
        assert any(f.noise_seed for f in group), kind
    for D in sf.SPOT_DIAMETERS:
        for path in ("lens", "apparent"):
            assert any(f.path == path and f.call.camera["diffraction_diameter"] == D for f in fams), (D, path)


def _wave_tiles(windows):
    """tiles_x * tiles_y of a wave whose live rays have the windows [(c0, c1, r0, r1), ...] (erf_splat_wave, bilinear_splat_wave)."""
    w = np.array(windows)
    return ((w[:, 1].max() - w[:, 0].min()) // 8 + 1) * ((w[:, 3].max() - w[:, 2].min()) // 8 + 1)


def test_packed_and_spread_families_pick_their_route(rendered):
    """The packed isolated families keep every wave's live rays within kSplatTiles = 6 tiles and within 7 pixels per window
    (the cooperative route), their fill sources aim off the sensor yet are not ruled out by the launch's source cull (which
    would pack the live sources of several waves into one); the spread ones need more tiles (the per-lane route)."""
    from photon_amd.library import PhotonLibrary
    fams, out, _ = rendered
    lib = PhotonLibrary()
    for f in fams:
        if not (f.isolated and ("packed" in f.name or "spread" in f.name)) or f.volume:
            continue
        d_x, d_y = sf.pixel_coords(f.call, out[f.name]["pos"], f.path)
        tiles = []
        for w0 in range(0, f.call.num_rays, sf.W):
            win = []
            for k in range(w0, min(w0 + sf.W, f.call.num_rays)):
                if np.isnan(d_x[k]):
                    continue
                if f.erf:
                    rfD = F32(sf.RENDER_FRACTION[f.path]) * F32(f.call.camera["diffraction_diameter"])
                    X, Y = F32(np.float64(d_x[k]) - 0.5), F32(np.float64(d_y[k]) - 0.5)
                    win.append((int(np.floor(X - rfD)), int(np.ceil(X + rfD)), int(np.floor(Y - rfD)), int(np.ceil(Y + rfD))))
                else:
                    taps, _ = taps_of_hit(f.call, *out[f.name]["pos"][k, :2])
                    win.append((taps[0][1], taps[0][1] + 1, taps[0][0], taps[0][0] + 1))
            if win:
                tiles.append(_wave_tiles(win))
                if f.erf and "packed" in f.name:
                    assert all(c1 - c0 + 1 <= 7 and r1 - r0 + 1 <= 7 for c0, c1, r0, r1 in win), f.name
        if "packed" in f.name:
            assert max(tiles) <= 6 and max(tiles) > 1, (f.name, tiles)
            if f.path != "apparent" and not f.train:                   # the cull applies behind a real first element only
                off = lib.sources_missing_sensor(f.call, [0.0], [0.0])
                assert off is not None and not off.any(), f.name
        else:
            assert sum(t > 6 for t in tiles) >= max(1, len(tiles) - 1), (f.name, tiles)      # (the last wave may be a few rays)


def test_bars_are_attainable_by_the_oracle_alone(oracle, rendered):
    """Three summation orders of the oracle (1, 5, 16 threads; the f64 accumulators are added in thread order): the erf
    families bit-identical, the 4-pixel families within the GPU tier's bar."""
    fams, out, d = rendered
    bad = []
    for f in fams:
        imgs = [sf.oracle_render(oracle, f, d, threads=t) for t in THREADS]
        for t, o in zip(THREADS, imgs):
            assert o["rays_on_sensor"] == out[f.name]["rays_on_sensor"] and o["sensor_taps"] == out[f.name]["sensor_taps"], (f.name, t)
            assert np.array_equal(o["pos"].view(np.uint32), out[f.name]["pos"].view(np.uint32)), (f.name, t)
            for other in (imgs[0]["image"], out[f.name]["image"]):
                m = image_mismatch(f, o["image"], other, f"oracle at {t} threads against another order")
                if m:
                    bad.append(m)
    assert not bad, "\n".join(bad[:20])


def test_erf_splat_against_the_numpy_model_at_the_edges(rendered):
    """Every isolated erf family, spot by spot from the dumped final positions: the lit pixels are exactly the model's
    support, and the values are one amplitude per spot times the model's erf factors to 1e-6 of the spot's maximum (the bar
    of test_erf_splat_is_the_pixel_integral_of_a_gaussian).  On the apparent-image path the dumped direction gives cos^4, so
    the amplitude itself is radiance / f#^2 * cos^4 / 4 (I0 * pi / 32 with I0 = radiance * cos^4 * 8 / pi, rounded to f32)."""
    fams, out, _ = rendered
    checked = clipped = 0
    for f in fams:
        if not (f.erf and f.isolated):
            continue
        o = out[f.name]
        img = o["image"].astype(np.float64)
        d_x, d_y = sf.pixel_coords(f.call, o["pos"], f.path)
        seen = np.zeros(img.shape, bool)
        for k in np.flatnonzero(~np.isnan(d_x)):
            rows, cols, m = erf_spot(f.call, f.path, d_x[k], d_y[k])
            assert rows.size and not seen[rows, cols].any(), (f.name, k)
            seen[rows, cols] = True
            v = img[rows, cols]
            assert (v != 0).all(), f"{f.name} ray {k}: model pixels unlit at {list(zip(rows[v == 0], cols[v == 0]))[:4]}"
            A = (v * m).sum() / (m * m).sum()
            assert np.abs(v - A * m).max() <= 1e-6 * v.max(), (f.name, k, np.abs(v - A * m).max() / v.max())
            if f.path == "apparent":
                dx, dy, dz = (np.float64(c) for c in o["dir"][k])
                cos4 = np.cos(np.arctan(np.sqrt((dx / dz) ** 2 + (dy / dz) ** 2))) ** 4
                want = f.call.src_radiance[k] / f.call.aperture_f_number ** 2 * cos4 / 4.0
                assert abs(A / want - 1) <= 2e-6, (f.name, k, A / want - 1)          # f32 I0 (6e-8), four factors of an f32 cosine
            checked += 1
            nx, ny = f.call.camera["x_pixel_number"], f.call.camera["y_pixel_number"]
            clipped += bool(rows.min() == 0 or cols.min() == 0 or rows.max() == ny - 1 or cols.max() == nx - 1)
        assert np.array_equal(seen, img != 0), f"{f.name}: {int((seen != (img != 0)).sum())} pixels lit outside the model's support"
    assert checked > 1500 and clipped > 400, (checked, clipped)


def test_four_pixel_splat_against_the_numpy_model_at_the_edges(oracle, rendered):
    """Every isolated 4-pixel family, hit by hit: pixels and area weights as the header states them equal oracle.pixel_taps;
    the lit pixels are exactly the taps the index rule lets land (weight not zero), wrapped ones in the last column of the
    row before; the values are one amplitude per hit times the weights."""
    fams, out, _ = rendered
    wrapped = dropped = 0
    for f in fams:
        if f.erf or not f.isolated:
            continue
        o = out[f.name]
        nx, ny = f.call.camera["x_pixel_number"], f.call.camera["y_pixel_number"]
        img = o["image"].astype(np.float64).ravel()
        ii, jj, w, inside = oracle.pixel_taps(f.call.camera, o["pos"][:, 0], o["pos"][:, 1])
        seen = np.zeros(img.size, bool)
        n_taps = 0
        for k in np.flatnonzero(~np.isnan(o["pos"][:, 0])):
            taps, ins = taps_of_hit(f.call, o["pos"][k, 0], o["pos"][k, 1])
            assert ins and inside[k]
            assert [(a, b) for a, b, _ in taps] == list(zip(ii[k].tolist(), jj[k].tolist())), (f.name, k)
            assert np.allclose([c for _, _, c in taps], w[k], rtol=0, atol=1e-15), (f.name, k)
            idx = [tap_index(a, b, nx, ny) for a, b, _ in taps]
            land = [(i, c) for i, (_, _, c) in zip(idx, taps) if i is not None]
            n_taps += len(land)
            dropped += 4 - len(land)
            wrapped += sum(1 for i, (_, b, _) in zip(idx, taps) if i is not None and b == 0)
            for i, (a, b, _) in zip(idx, taps):
                if i is not None and b == 0:
                    assert i % nx == nx - 1 and i // nx == a - 2, (f.name, k)          # the last column of the row before
            px = np.array([i for i, c in land if c != 0], np.int64)
            wt = np.array([c for i, c in land if c != 0])
            if px.size == 0:
                continue
            assert not seen[px].any(), (f.name, k)
            seen[px] = True
            v = img[px]
            assert (v != 0).all(), (f.name, k)
            A = (v * wt).sum() / (wt * wt).sum()
            assert np.abs(v - A * wt).max() <= 1e-6 * v.max(), (f.name, k)
        assert n_taps == o["sensor_taps"], f.name
        assert np.array_equal(seen, img != 0), f"{f.name}: {int((seen != (img != 0)).sum())} pixels lit outside the model's support"
    assert wrapped > 50 and dropped > 100, (wrapped, dropped)


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


@pytest.mark.skipif(_hipcc() is None or shutil.which("nm") is None, reason="needs hipcc and nm")
def test_debug_build_exports_the_splat_reader(tmp_path):
    out = _build.build_library(verbose=False, extra_flags=path_stats.PATH_STATS_FLAGS, out_path=str(tmp_path / "lib_pathstats.so"))
    syms = subprocess.run(["nm", "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert " photon_debug_splat_stats" in syms and " photon_debug_path_stats" in syms
    assert os.path.getsize(out) > 0
    default = subprocess.run(["nm", "-D", "--defined-only", _build.build_library(verbose=False)], capture_output=True, text=True, check=True).stdout
    assert "photon_debug_" not in default                              # debug builds only
