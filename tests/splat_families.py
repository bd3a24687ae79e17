"""Scene families aimed at the branches of the sensor stage (photon_amd/csrc/device_optics.hpp: erf_splat_wave,
bilinear_splat_wave; photon_sensor.hip: the six sensor_kernel instantiations).

Every family is a RayTracingCall on a small sensor whose images straddle all four edges and corners.  Sources are placed
by PIXEL: the affine map from a source's (x, y) to the sensor coordinate (d_x, d_y) its chief ray gets is measured once
per camera from the oracle's ray dump of two probe sources (the paraxial magnification to within the f32 roundings of the
ray), and the "ulp" families walk a source over an inside-test or window boundary one f32 step at a time, found by
bisection on the oracle's dump.  Waves: a launch gives ray r to lane r % 64 of wave r // 64, source-major, so a family
builds its waves by the order of its sources.  Each family names the counter slots (photon_amd/path_stats.py,
SPLAT_SLOTS) it is built to reach in a default trace of a scene (launch culls on)."""
from __future__ import annotations

import copy
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from photon_amd import scenes
from photon_amd.ray_tracing import single_lens_camera

W = 64
PITCH = 17.0
F32 = np.float32

# render fraction of the two erf paths (device_optics.hpp: sensor_diffraction 0.75, apparent_image 1.0)
RENDER_FRACTION = {"lens": 0.75, "apparent": 1.0}
LENS_MODEL = {"lens": "general", "apparent": "apparent", "taps": "general"}
SENSOR = {"lens": (128, 96), "apparent": (96, 96), "taps": (112, 80)}       # (x_pixel_number, y_pixel_number)
SPOT_DIAMETERS = (1.0, 2.0, 3.0, 4.5, 8.0)


@dataclass
class Family:
    name: str
    call: object                        # RayTracingCall
    path: str                           # "lens" | "apparent": erf splat; "taps": 4-pixel splat
    isolated: bool = False              # one ray per source and no pixel receives two increments
    train: bool = False                 # photon_scene_set_element_train(1) / oracle.set_element_train(1)
    noise_seed: Optional[int] = None    # position noise on, with this seed
    edges: bool = True                  # images straddle the sensor's edges: 0 < rays_on_sensor < rays
    slots: list = field(default_factory=list)

    @property
    def erf(self):
        return self.path != "taps"

    @property
    def volume(self):
        return bool(self.call.simulate_density_gradients)


def pixel_coords(call, pos, path):
    """(d_x, d_y) of final positions [n, 3] as the sensor functions form them, in f32 (device_optics.hpp: sensor_diffraction,
    apparent_image, sensor_bilinear); NaN rows stay NaN."""
    cam = call.camera
    nx, ny, pitch = int(cam["x_pixel_number"]), int(cam["y_pixel_number"]), F32(cam["pixel_pitch"])
    p1x = F32(-float(pitch) * (nx - 1) / 2.0)
    p1y = F32(-float(pitch) * (ny - 1) / 2.0)
    x, y = np.asarray(pos[:, 0], F32), np.asarray(pos[:, 1], F32)
    with np.errstate(invalid="ignore"):
        u = (x - p1x) / pitch
        d_x = u if path == "taps" else F32(nx - 1) - u
        d_y = (y - p1y) / pitch
    return d_x.astype(F32), d_y.astype(F32)


def oracle_render(oracle, fam, workdir, threads=None):
    """The oracle's render of a family with every ray dumped: dict(image, rays_on_sensor, sensor_taps, pos, dir)."""
    call = copy.copy(fam.call)
    d = os.path.join(workdir, "oracle_" + fam.name)
    os.makedirs(d, exist_ok=True)
    call.save_lightrays, call.num_lightrays_save = True, call.num_rays
    call.lightray_position_save_path = call.lightray_direction_save_path = d
    assert call.num_sources <= call.source_point_number            # one chunk: one pair of dump files
    if threads:
        before = oracle.num_threads()
        oracle.set_num_threads(threads)
    oracle.set_noise_seed(fam.noise_seed or 0)
    oracle.set_element_train(1 if fam.train else 0)
    try:
        img, st = oracle.render(call, interpolation=1)
    finally:
        oracle.set_noise_seed(0)
        oracle.set_element_train(0)
        if threads:
            oracle.set_num_threads(before)
    return dict(image=img, rays_on_sensor=int(st.rays_on_sensor), sensor_taps=int(st.sensor_taps),
                pos=np.fromfile(os.path.join(d, "pos_0000.bin"), F32).reshape(-1, 3),
                dir=np.fromfile(os.path.join(d, "dir_0000.bin"), F32).reshape(-1, 3))


def uniform_volume(workdir):
    """A small volume of constant density between target and lens: zero gradient, rays stay straight, the sensor stage
    starts from the march's state arrays (FROM_STATE)."""
    path = os.path.join(workdir, "uniform_12.nrrd")
    if not os.path.exists(path):
        _, sp, org = scenes.bos_volume(12)
        scenes.write_nrrd(path, np.full((12, 12, 12), 1.225, F32), sp, org)
    return path


def _axis(n, step, first=0.25, last_in=0.3):
    """Coordinates along one axis of n pixels: one line off the sensor either side, the first line inside pixel 0 (the erf
    spot centred before the first pixel centre), lines `step` and a bit apart whose sub-pixel phase drifts, and one in the
    last pixel."""
    inner = np.arange(first, n - last_in - step, step + 0.37)
    return np.concatenate([[-0.4], inner, [n - last_in, n + 0.4]])


class Builder:
    def __init__(self, oracle, workdir):
        self.oracle, self.workdir = oracle, workdir
        self.nrrd = uniform_volume(workdir)
        self._map = {}

    # ---- calls -------------------------------------------------------------------------------
    def call(self, path, x, y, rps=1, D=3.0, ratio=1e-4, z=None, radiance=None, volume=False, sensor=None):
        geom = single_lens_camera(lens_model=LENS_MODEL[path], **scenes.SAMPLE_LENS)
        nx, ny = sensor or SENSOR[path]
        cam = scenes.sample_camera(path != "taps", nx, PITCH, D)
        cam["y_pixel_number"] = ny
        x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
        n = x.size
        c = scenes._call(geom, cam, scattering_type="diffuse", src_x=x, src_y=y,
                         src_z=np.full(n, geom["z_object"]) if z is None else geom["z_object"] + np.asarray(z, np.float64),
                         src_radiance=np.full(n, 10.0) if radiance is None else np.asarray(radiance, np.float64),
                         src_diameter_index=np.ones(n, np.int32), lightray_number_per_particle=int(rps),
                         beam_wavelength=0.532 if path == "taps" else 0.0, ray_cone_pitch_ratio=ratio,
                         simulate_density_gradients=bool(volume), density_grad_filename=self.nrrd if volume else "",
                         ray_tracing_algorithm=2 if volume else 0)
        return c

    def _dump_coords(self, path, x, y, sensor=None):
        fam = Family("probe", self.call(path, x, y, sensor=sensor), path)
        out = oracle_render(self.oracle, fam, self.workdir)
        return pixel_coords(fam.call, out["pos"], path)

    def affine(self, path, sensor=None):
        """(ax, bx, ay, by): d_x = ax * src_x + bx, d_y = ay * src_y + by for the chief ray of a source at the object plane."""
        key = (path, sensor)
        if key not in self._map:
            M = scenes.SAMPLE_LENS["focal_length"] / (scenes.SAMPLE_LENS["object_distance"] - scenes.SAMPLE_LENS["focal_length"])
            a = 20.0 * PITCH / M                                    # images ~20 px either side of the centre
            dx, dy = self._dump_coords(path, [-a, a], [-a, a], sensor)
            assert np.isfinite(dx).all() and np.isfinite(dy).all()
            ax, ay = (float(dx[1]) - float(dx[0])) / (2 * a), (float(dy[1]) - float(dy[0])) / (2 * a)
            self._map[key] = (ax, (float(dx[1]) + float(dx[0])) / 2, ay, (float(dy[1]) + float(dy[0])) / 2)
        return self._map[key]

    def sources(self, path, d_x, d_y, sensor=None):
        ax, bx, ay, by = self.affine(path, sensor)
        return (np.asarray(d_x, np.float64) - bx) / ax, (np.asarray(d_y, np.float64) - by) / ay

    # ---- f32 ladders over a boundary ------------------------------------------------------------
    def ladders(self, path, targets_x, targets_y):
        """Sources whose sensor coordinate along one axis lies within two f32 steps OF THE SOURCE COORDINATE of a boundary
        value: for every target t of targets_x, four sources lined up along y 7 px apart, each bisected on its own (the lens
        couples the axes at the 1e-5 px level) to the adjacent pair of f32 x either side of the crossing of d_x = t -- 0 and
        the pixel count are the inside test itself, read from the dump's NaNs -- and put just before, just after, and one
        step further out either side; likewise targets_y.  Returns (x, y) of all of them."""
        nx, ny = SENSOR[path]
        jobs = []                                                   # (axis, target, pixel coordinate along the other axis, member)
        for axis, targets in ((0, targets_x), (1, targets_y)):
            for t in targets:
                slot = sum(1 for tt in targets if tt < t and abs(tt - t) < 2.0)          # ladders that share this edge sit side by side
                for m in range(4):
                    jobs.append((axis, float(t), 8.0 + 28.0 * slot + 7.0 * m, m))
                    assert jobs[-1][2] < (ny, nx)[axis] - 12
        k = len(jobs)
        axis = np.array([j[0] for j in jobs])
        t = np.array([j[1] for j in jobs])
        limit = np.where(axis == 0, nx, ny).astype(np.float64)
        o_x, o_y = self.sources(path, [j[2] for j in jobs], [j[2] for j in jobs])
        s_lo = self.sources(path, t - 0.04, t - 0.04)
        s_hi = self.sources(path, t + 0.04, t + 0.04)
        lo = np.where(axis == 0, s_lo[0], s_lo[1]).astype(F32)
        hi = np.where(axis == 0, s_hi[0], s_hi[1]).astype(F32)

        def evaluate(s):
            dx, dy = self._dump_coords(path, np.where(axis == 0, s, o_x), np.where(axis == 0, o_y, s))
            v = np.where(axis == 0, dx, dy)
            with np.errstate(invalid="ignore"):
                return np.where((t == 0.0) | (t == limit), np.isnan(v), v < t.astype(F32))

        p_lo, p_hi = evaluate(lo), evaluate(hi)
        assert (p_lo != p_hi).all(), [j for j, a, c in zip(jobs, p_lo, p_hi) if a == c]
        as_int = lambda a: a.view(np.int32).astype(np.int64)        # noqa: E731  (same sign within a pair: ordered like the floats)
        for _ in range(40):
            if (np.abs(as_int(hi) - as_int(lo)) <= 1).all():
                break
            mid = ((as_int(lo) + as_int(hi)) // 2).astype(np.int32).view(F32)
            same = evaluate(mid) == p_lo
            lo, hi = np.where(same, mid, lo).astype(F32), np.where(same, hi, mid).astype(F32)
        assert (np.abs(as_int(hi) - as_int(lo)) == 1).all()
        a, b = np.minimum(lo, hi), np.maximum(lo, hi)
        member = np.array([j[3] for j in jobs])
        s = np.select([member == 0, member == 1, member == 2], [a, b, np.nextafter(a, F32(-np.inf))], np.nextafter(b, F32(np.inf)))
        s = s.astype(np.float64)
        return np.where(axis == 0, s, o_x), np.where(axis == 0, o_y, s)


def _grid(ax_x, ax_y):
    gx, gy = np.meshgrid(ax_x, ax_y)
    return gx.ravel(), gy.ravel()


def _packed(rng, nx, ny, clusters, live_offsets):
    """Waves of 64 sources: the live ones of a cluster first, the rest aimed half a pixel off the sensor's first column
    (on no pixel, yet too near for the launch's source cull to rule out), so that each wave's live rays stay together."""
    dx, dy = [], []
    for cx, cy in clusters:
        n_live = len(live_offsets)
        dx += [cx + ox for ox, _ in live_offsets] + [-0.5] * (W - n_live)
        dy += [cy + oy for _, oy in live_offsets] + list(rng.uniform(5.0, ny - 5.0, W - n_live))
    return np.array(dx), np.array(dy)


def build_families(oracle, workdir):
    """Every family, in a fixed order."""
    b = Builder(oracle, workdir)
    rng = np.random.default_rng(2024)
    fams = []

    def add(name, path, d_x, d_y, slots, isolated=False, train=False, noise=None, edges=True, **kw):
        sensor = kw.get("sensor")
        x, y = b.sources(path, d_x, d_y, sensor)
        c = b.call(path, x, y, **kw)
        if noise:
            c.add_pos_noise, c.pos_noise_std = True, float(noise[1])
        fams.append(Family(name, c, path, isolated, train, noise[0] if noise else None, edges, list(slots)))
        return fams[-1]

    for path in ("lens", "apparent"):
        nx, ny = SENSOR[path]
        rf = RENDER_FRACTION[path]
        # ---- isolated spots, spread over the whole sensor: far more than kSplatTiles tiles per wave -> erf_splat_lane;
        # every spot size through both render fractions; D = 4.5 and 8 are also too wide for the parked layout
        for D in SPOT_DIAMETERS:
            step = float(np.ceil(2 * rf * D)) + 4.0
            slots = ["E_WAVES", "E_FALLBACK", "E_FB_TILES", "E_LANE_CLIPPED_LANES", "K_GEN_ERF"] + (["E_FB_WIDE"] if rf * D > 3.0 else [])
            add(f"iso_spread_{path}_D{D:g}", path, *_grid(_axis(nx, step), _axis(ny, step)), slots, isolated=True, D=D)
        # ---- isolated spots, two per wave 10 px apart (3 x 1 or 3 x 2 tiles): the cooperative route, one increment per pixel.
        # Clusters in each corner, on each edge, in the X < 8 / Y < 8 bands and inside.
        for D in (1.0, 3.0) if path == "lens" else (1.0, 2.0):      # (apparent image, D = 3: a window of 8 falls back)
            cl = [(0.25, 0.3), (nx - 10.4, 0.3), (0.25, ny - 0.35), (nx - 10.4, ny - 0.3),                     # corners
                  (nx / 2 + 0.6, 0.45), (nx / 2 - 3.3, ny - 0.4), (0.3, ny / 2 + 0.2), (nx - 10.3, ny / 2 - 0.7),     # edges
                  (4.7, 20.2), (7.45, 33.5), (8.45, 62.5), (8.55, 76.0), (nx / 2 - 17.8, 7.3), (nx / 2 + 22.2, 8.45),  # X, Y either side of 8
                  (50.5, 40.5), (33.1, 61.8), (nx - 40.3, 70.2)]
            add(f"iso_packed_{path}_D{D:g}", path, *_packed(rng, nx, ny, cl, [(0.0, 0.0), (10.0, 0.0)]),
                ["E_COOP", "E_BOTH_X_LANES", "E_BOTH_Y_LANES", "E_SHARED_X_LANES", "E_SHARED_Y_LANES", "E_CLIPPED_LANES", "E_MULTI_TILE",
                 "E_TILES_SAME"], isolated=True, D=D)
        # ---- one source per wave: 64 rays in a narrow cone, every ray of a wave with the same window
        for D in (1.0, 3.0) if path == "lens" else (2.0,):
            add(f"one_source_{path}_D{D:g}", path, *_grid(_axis(nx, 9.0), _axis(ny, 9.0)),
                ["E_COOP", "E_TILES_SAME", "E_CLIPPED_LANES", "E_BOTH_X_LANES", "E_SHARED_X_LANES"], rps=64, D=D)
        # ---- waves across two sources 5 px apart (100 rays per source: their windows meet in one tile) and rows of 64
        # neighbouring one-ray sources a quarter pixel apart: windows differ within the wave, several tiles
        D = 3.0 if path == "lens" else 2.0
        add(f"two_sources_{path}", path, *_grid(_axis(nx, 5.0), _axis(ny, 5.0)), ["E_COOP", "E_TILES_MIXED", "E_MULTI_TILE", "E_TILES_SAME"],
            rps=100, D=D)
        rows = np.concatenate([[0.3, 4.2, 7.9, 8.1], np.arange(14.7, ny - 8, 13.3), [ny - 0.3]])
        starts = [-3.1, nx / 2 - 8.2, nx - 12.9]
        dx = np.concatenate([s + 0.25 * np.arange(W) for _ in rows for s in starts])
        dy = np.concatenate([np.full(W, r) + 0.01 * np.arange(W) for r in rows for _ in starts])
        add(f"dense_rows_{path}", path, dx, dy, ["E_COOP", "E_TILES_MIXED", "E_MULTI_TILE", "E_CLIPPED_LANES"], D=D)
        # ---- inside test and window boundaries within one f32 step of the source: d = 0, 0.5, n - 0.5, n on both axes
        lx, ly = b.ladders(path, [0.0, 0.5, nx - 0.5, float(nx)], [0.0, 0.5, ny - 0.5, float(ny)])
        c = b.call(path, lx, ly, D=1.0)
        fams.append(Family(f"ulp_edges_{path}", c, path, True, slots=["E_FALLBACK"]))
        # ---- after a march through the uniform volume (FROM_STATE), through the element train, and both
        add(f"one_source_{path}_volume", path, *_grid(_axis(nx, 9.0), _axis(ny, 9.0)), ["K_STATE_ERF", "E_COOP"], rps=64, D=D, volume=True)
        if path == "lens":
            add("one_source_lens_train", path, *_grid(_axis(nx, 9.0), _axis(ny, 9.0)), ["K_GEN_TRAIN", "E_COOP"], rps=64, D=D, train=True)
            add("two_sources_lens_train_volume", path, *_grid(_axis(nx, 5.0), _axis(ny, 5.0)), ["K_STATE_TRAIN", "E_COOP", "E_TILES_MIXED"], rps=100, D=D,
                train=True, volume=True)
        # ---- position noise pushes hits across the sensor's edges after the lens
        add(f"one_source_{path}_noise", path, *_grid(_axis(nx, 9.0), _axis(ny, 9.0)), ["E_WAVES", "E_TILES_MIXED"], rps=64, D=D, noise=(77, 1.5))

    # ---- a render radius outside (0, 1e4): the third fall-back reason.  Every pixel of a 64 x 64 sensor is inside the window.
    add("radius_out_of_range", "lens", [10.3, 63.6, 70.0], [12.2, 0.2, 5.0], ["E_FB_RADIUS", "E_FALLBACK"], D=1.4e4, sensor=(64, 64))

    # ---- the 4-pixel splat: the 4-pixel-only kernel, the element train (bilinear_splat_wave on the erf splat's LDS layout),
    # and both after a march
    nx, ny = SENSOR["taps"]
    iso = _grid(_axis(nx, 3.7, first=0.2), _axis(ny, 3.7, first=0.2))
    cl = [(0.2, 0.2), (nx - 19.2, 0.3), (0.3, ny - 9.7), (nx - 19.25, ny - 9.75), (40.4, 0.6), (0.7, 30.3), (nx - 19.1, 33.4), (44.0, ny - 9.65),
          (30.55, 30.45), (64.45, 1.2), (20.3, 12.2)]
    packed = _packed(rng, nx, ny, cl, [(3.13 * i, 3.13 * j) for j in range(4) for i in range(7)])
    rows = np.concatenate([[0.2, 0.7, 1.3], np.arange(6.6, ny - 4, 9.3), [ny - 0.7, ny - 0.2]])
    starts = [-3.1, nx / 2 - 8.2, nx - 12.9]
    dense = (np.concatenate([s + 0.25 * np.arange(W) for _ in rows for s in starts]),
             np.concatenate([np.full(W, r) + 0.013 * np.arange(W) for r in rows for _ in starts]))
    n_part = 131
    edge = np.array([(0.2, 0.2), (0.3, 17.6), (0.25, 41.1), (0.1, ny - 0.2), (13.3, 0.3), (55.5, 0.2), (nx - 0.2, 0.4), (nx - 0.3, 29.9),
                     (nx - 0.25, ny - 0.3), (37.7, ny - 0.2), (80.1, ny - 0.35), (0.6, 1.4)])
    cloud = (np.concatenate([edge[:, 0], rng.uniform(-3.0, nx + 3.0, n_part - len(edge))]),
             np.concatenate([edge[:, 1], rng.uniform(-3.0, ny + 3.0, n_part - len(edge))]))
    cloud_kw = dict(rps=37, ratio=1.0, z=rng.uniform(-7.5e3, 7.5e3, n_part), radiance=rng.uniform(2.0, 30.0, n_part))
    for tag, kw, k_slot in (("", {}, "K_GEN_TAPS"), ("_train", dict(train=True), "K_GEN_TRAIN"), ("_volume", dict(volume=True), "K_STATE_TAPS"),
                            ("_train_volume", dict(train=True, volume=True), "K_STATE_TRAIN")):
        add("taps_iso_spread" + tag, "taps", *iso, [k_slot, "T_WAVES", "T_LANE_ROUTE", "T_TAPS_DROPPED", "T_TAPS_WRAPPED", "T_TAPS_LANDED"],
            isolated=True, **kw)
        add("taps_iso_packed" + tag, "taps", *packed, [k_slot, "T_COOP", "T_MULTI_TILE", "T_TAPS_DROPPED", "T_TAPS_WRAPPED"], isolated=True, **kw)
        add("taps_dense_rows" + tag, "taps", *dense, [k_slot, "T_COOP", "T_TAPS_DROPPED", "T_TAPS_WRAPPED"], **kw)
        # 131 particles x 37 rays through the full aperture, in and out of focus: overlapping hits, a partial last wave
        add("taps_cloud" + tag, "taps", *cloud, [k_slot, "T_WAVES"], **kw, **cloud_kw)
    lx, ly = b.ladders("taps", [0.0, 0.5, nx - 0.5, float(nx)], [0.0, 0.5, ny - 0.5, float(ny)])
    fams.append(Family("taps_ulp_edges", b.call("taps", lx, ly), "taps", True, slots=["T_TAPS_DROPPED", "T_TAPS_WRAPPED"]))
    fams.append(Family("taps_ulp_edges_train", b.call("taps", lx, ly), "taps", True, train=True, slots=["K_GEN_TRAIN"]))
    add("taps_cloud_noise", "taps", *cloud, ["T_WAVES"], noise=(31, 1.2), **cloud_kw)
    add("taps_dense_rows_train_noise", "taps", *dense, ["K_GEN_TRAIN", "T_WAVES"], train=True, noise=(32, 0.8))
    names = [f.name for f in fams]
    assert len(set(names)) == len(names)
    return fams
