"""Ray families aimed at the branches of the wave-cooperative samplers (photon_amd/csrc/device_volume_coop.hpp).

Both march launches (trace_rays: the plain grid; trace_rays_queued: the render path's persistent waves) give ray r to lane
r % 64 of group r // 64, so a family builds its waves 64 rays at a time.  Rays are placed by cell from the volume's info():
the samplers see a position p at lookup coordinate L = 1 + (p - min) / (max - min) * (n - 2), and a lane whose L lies in
[c + 0.5, c + 1.5) blends from cell c.  Each family names the counter slots (photon_amd/path_stats.py) it is built to
reach, per sampler ("C" tricubic, "L" trilinear)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

W = 64


def volume_density(kind: str) -> tuple:
    """(rho [nz, ny, nx], spacing, origin) of the three volumes the families march through."""
    if kind == "mid":                                   # lopsided, deep in z, smooth with noise
        dims = (64, 40, 44)
        rng = np.random.default_rng(77)
        z, y, x = np.meshgrid(*(np.linspace(-1, 1, k) for k in dims), indexing="ij")
        rho = 1.2 + 0.3 * np.exp(-(x ** 2 + 1.5 * y ** 2 + 0.7 * z ** 2) * 3) + 0.02 * rng.standard_normal(dims)
        return rho.astype(np.float32), (100.0, 100.0, 100.0), (-2000.0, -1500.0, 750e3)
    if kind == "tiny":                                  # a 4-texel axis: every brick is wider than the volume
        dims = (9, 4, 7)
        rng = np.random.default_rng(78)
        rho = 1.2 + 0.05 * rng.standard_normal(dims)
        return rho.astype(np.float32), (100.0, 100.0, 100.0), (0.0, 0.0, 750e3)
    if kind == "const":                                 # every blend sits on data_min: the tricubic sum's rounding dips below it
        return np.full((12, 12, 12), 1.225, np.float32), (100.0, 100.0, 100.0), (0.0, 0.0, 750e3)
    if kind == "vac":                                   # dense, with one line of near-vacuum texels along z: the volume's minimum
        rng = np.random.default_rng(79)
        rho = 1.2 + 0.01 * rng.standard_normal((16, 12, 12))
        rho[:, VAC_J, VAC_I] = 1e-9
        return rho.astype(np.float32), (100.0, 100.0, 100.0), (0.0, 0.0, 750e3)
    raise ValueError(kind)


VOLUMES = ("mid", "tiny", "const", "vac")
VAC_I, VAC_J = 6, 5                                     # texel column (x, y) of the vacuum line


@dataclass
class Family:
    name: str
    volume: str
    pos: np.ndarray                     # f32 [n, 3]
    dir: np.ndarray                     # f32 [n, 3]
    enters: np.ndarray                  # bool [n]: the ray is meant to take steps (False: meant to miss)
    slots: dict = field(default_factory=dict)       # {"C": [...], "L": [...]}: slots the family is built to reach


class Grid:
    """World positions of lookup coordinates of one volume (its info())."""

    def __init__(self, info):
        self.n = np.array([info.nx, info.ny, info.nz], np.float64)
        self.lo = np.array(info.min_bound, np.float64)
        self.hi = np.array(info.max_bound, np.float64)

    def world(self, L):
        L = np.asarray(L, np.float64)
        return self.lo + (L - 1.0) / (self.n - 2.0) * (self.hi - self.lo)

    def lookup32(self, p):
        """The march's lookup index of f32 positions, in f32 as the device forms it (lookup_index_u)."""
        p = np.asarray(p, np.float32)
        lo, hi = self.lo.astype(np.float32), self.hi.astype(np.float32)
        scale = np.float32(1.0) / (hi - lo)
        return np.float32(1.0) + (scale * (p - lo)) * (self.n.astype(np.float32) - np.float32(2.0))


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _wave(g: Grid, L, d):
    """One wave: lookup coordinates [64, 3] and directions [64, 3] (or one direction for all)."""
    L = np.asarray(L, np.float64).reshape(W, 3)
    d = np.broadcast_to(_unit(d), (W, 3))
    return g.world(L), d


def _family(name, volume, waves, slots, enters=None):
    pos = np.concatenate([w[0] for w in waves]).astype(np.float32)
    d = np.concatenate([w[1] for w in waves]).astype(np.float32)
    return Family(name, volume, pos, d, np.ones(len(pos), bool) if enters is None else enters, slots)


def _column(ci, cj, lz, jitter=0.04, seed=0):
    """64 lanes in cell column (ci, cj) at lookup z `lz` (scalar or per lane), spread a little in x and y."""
    rng = np.random.default_rng(seed)
    L = np.empty((W, 3))
    L[:, 0] = ci + 1.0 + rng.uniform(-jitter, jitter, W)
    L[:, 1] = cj + 1.0 + rng.uniform(-jitter, jitter, W)
    L[:, 2] = lz
    return L


def mid_families(info):
    g = Grid(info)
    nx, ny, nz = int(info.nx), int(info.ny), int(info.nz)
    fams = []
    # one column up (+z) and one down (-z): tiles fetched upwards / downwards, cells of the parked tile, the parked cell
    fams.append(_family("column_up", "mid", [_wave(g, _column(20, 18, 2.0, seed=1), (0, 0, 1)),
                                             _wave(g, _column(9, 30, 2.0, seed=2), (0.002, -0.001, 1))],
                        {"C": ["C_FETCH_UP", "C_CELL_IN_TILE", "C_HIT_CELL", "C_COHERENT"], "L": ["L_FETCH", "L_HIT_A", "L_COHERENT"]}))
    fams.append(_family("column_down", "mid", [_wave(g, _column(20, 18, nz - 2.0, seed=3), (0, 0, -1)),
                                               _wave(g, _column(30, 9, nz - 2.0, seed=4), (-0.002, 0.001, -1))],
                        {"C": ["C_FETCH_DOWN", "C_CELL_IN_TILE"], "L": ["L_FETCH_DOWN", "L_HIT_A"]}))
    # a coherent wave along x: a new column, hence a new tile, at every cell
    L = _column(0, 20, 30.0, seed=5)
    L[:, 0] = 1.6
    L[:, 1] = 21.0
    fams.append(_family("row_x", "mid", [_wave(g, L, (1, 0, 0.001))], {"C": ["C_FETCH_UP"], "L": ["L_FETCH"]}))
    # two columns in one wave: the first sample needs two new tiles (A and B); then tile B's second test serves it
    L = _column(14, 14, 2.0, seed=6)
    L[32:, 0] += 1.0
    L2 = _column(25, 8, nz - 2.0, seed=7)
    L2[::2, 1] += 1.0
    fams.append(_family("two_columns", "mid", [_wave(g, L, (0, 0, 1)), _wave(g, L2, (0, 0, -1))],
                        {"C": ["C_INCOHERENT", "C_BRICK_LANES", "C_BRICK_REUSED"],
                         "L": ["L_FETCH_TWO", "L_FETCH_TO_B", "L_HIT_B", "L_TILE_B_LANES"]}))
    # one column whose lanes straddle layer boundaries: lane 0 (the leader) in the middle, lanes behind and ahead of it (the
    # lanes that leave a tile first lead its replacement alone: the shift for lanes ahead needs the "ahead" family below)
    def straddle(ci, cj, c, seed):
        L = _column(ci, cj, c + 1.0, seed=seed)
        L[1:32, 2] = c + 0.3
        L[32:, 2] = c + 1.7
        return L
    fams.append(_family("straddle", "mid", [_wave(g, straddle(10, 10, 4, 8), (0, 0, 1)), _wave(g, straddle(33, 29, nz - 6, 9), (0, 0, -1))],
                        {"C": ["C_INCOHERENT", "C_BRICK_PASS"], "L": ["L_BASE_BEHIND", "L_FETCH_DOWN"]}))
    # the base shift for lanes AHEAD of a downward leader: one column, lane 0 and half the lanes in the bottom cell of the
    # first tile (base = their layer k0: nobody behind the leader) heading -z, the other half in its top cell (k0 + 14 with
    # 16 layers) heading +z, both a quarter cell from leaving it -- they leave together, tile A serves nobody, and its
    # replacement is fetched downwards (the leader lies below A's base) with lanes of the column above the leader
    k0 = 20
    L = _column(27, 15, k0 + 0.75, seed=15)
    d = np.zeros((W, 3))
    d[:, 2] = -1.0
    L[W // 2:, 2] = k0 + 14 + 1.25
    d[W // 2:, 2] = 1.0
    fams.append(_family("ahead", "mid", [_wave(g, L, d)], {"C": ["C_INCOHERENT"], "L": ["L_BASE_AHEAD", "L_FETCH_DOWN", "L_OUT_OF_REACH"]}))
    # one column whose lanes lie more than TL - 1 layers apart: out of the tile's reach -- bricks, then the gather
    L = _column(22, 22, 0.0, seed=10)
    L[:, 2] = 2.0 + (np.arange(W) % 24)
    fams.append(_family("out_of_reach", "mid", [_wave(g, L, (0, 0, 1))],
                        {"C": ["C_BRICK_FETCH", "C_GATHER_LANES"], "L": ["L_OUT_OF_REACH", "L_MARK_INCOHERENT", "L_GATHER_LANES"]}))
    # three columns converging into one over more than 32 trips: incoherent, retried (and skipped) trips, two columns again
    # (two new tiles on a retry), coherent again
    c = 21
    L = _column(c, 12, 1.6, jitter=0.02, seed=11)
    d = np.zeros((W, 3))
    d[:, 2] = 1.0
    L[21:43, 0] = c + 1.0 - 1.0
    d[21:43, 0] = 0.5 / 34 * 1.0
    L[43:, 0] = c + 1.0 + 1.3
    d[43:, 0] = -0.8 / 38 * 1.0
    fams.append(_family("converge", "mid", [_wave(g, L, d)],
                        {"C": ["C_INCOHERENT", "C_COHERENT"],
                         "L": ["L_NO_FREE_TILE", "L_MARK_INCOHERENT", "L_TILES_SKIPPED", "L_RETRY", "L_COHERENT_AGAIN", "L_FETCH_TWO"]}))
    # a 3 x 3 fan of lane groups 6 cells apart: nine bricks, more than PHOTON_BRICK_PASSES: the gather serves the rest
    L = np.empty((W, 3))
    grp = np.arange(W) % 9
    L[:, 0] = 10.0 + 6 * (grp % 3) + 0.05 * (np.arange(W) % 3)
    L[:, 1] = 10.0 + 6 * (grp // 3) + 0.05 * (np.arange(W) % 2)
    L[:, 2] = 3.0
    fams.append(_family("fan", "mid", [_wave(g, L, (0, 0, 1))],
                        {"C": ["C_BRICK_FETCH", "C_GATHER_LANES", "C_INCOHERENT_LANES"], "L": ["L_NO_FREE_TILE", "L_BRICK_LANES", "L_GATHER_LANES"]}))
    # a partial last wave and lanes that finish early (need != every lane): a column whose lanes start at different heights,
    # and rays that miss (start outside, head away) in the same waves
    L = _column(15, 25, 0.0, seed=12)
    L[:, 2] = np.where(np.arange(W) % 3 == 0, nz - 3.0, 4.0)
    p1, d1 = _wave(g, L, (0, 0, 1))
    L = _column(28, 20, 5.0, seed=13)
    p2, d2 = g.world(L[:37]), np.broadcast_to(_unit((0.001, 0, 1)), (37, 3))
    miss = np.zeros(W + 37, bool)
    pos = np.concatenate([p1, p2])
    dd = np.concatenate([d1, d2]).copy()
    k = np.arange(W + 37) % 11 == 5                     # start below the box, pointing away: a miss
    pos[k, 2] = g.lo[2] - 500.0
    dd[k] = (0, 0, -1)
    miss[k] = True
    fams.append(Family("partial_wave", "mid", pos.astype(np.float32), dd.astype(np.float32), ~miss,
                       {"C": ["C_COHERENT"], "L": ["L_COHERENT"]}))
    # rays that start far below the box, heading up: the f32 intersection lands them short of the face, more than a texel
    # outside -- their first lookup is not accessible, and they spin (the reference's `continue`) until it is
    fams.append(spin_family(g))
    return fams


def spin_family(g: Grid):
    cand = []
    rng = np.random.default_rng(14)
    d = np.array([0.0, 0.28, 0.96], np.float32)
    for D in rng.uniform(1.0e9, 3.0e9, 20000):
        p = np.array([g.world([12.0 + rng.uniform(0, 20), 1, 1])[0], g.world([1, 12.0 + rng.uniform(0, 16), 1])[1] - 0.28 / 0.96 * D,
                      g.lo[2] - D], np.float32)
        q = intersect32(p, d, g)
        if q is None:
            continue
        lz = g.lookup32(q)
        if -0.3 < lz[2] < -0.02 and 2.0 < lz[1] < g.n[1] - 3.0:      # one spin, then the march takes steps
            cand.append(p)
        if len(cand) == W:
            break
    assert len(cand) == W, len(cand)
    return Family("spin_outside", "mid", np.array(cand, np.float32), np.tile(d, (W, 1)), np.ones(W, bool),
                  {"C": ["C_SPIN_OUTSIDE"], "L": ["L_SPIN_OUTSIDE"]})


def intersect32(pos, d, g: Grid):
    """intersect_with_volume (device_volume.hpp) in f32, as the march does it: the entry point, or None (a miss)."""
    f = np.float32
    p1, p2 = g.lo.astype(f), g.hi.astype(f)
    tnear, tfar = f(-(np.finfo(np.float32).max - 1)), np.finfo(np.float32).max
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            t1, t2 = f((p1[a] - pos[a]) / d[a]), f((p2[a] - pos[a]) / d[a])
            if t1 > t2:
                t1, t2 = t2, t1
            if (a < 2 and t1 > tnear) or (a == 2 and t1 >= 0 and t1 > tnear):
                tnear = t1
            if t2 < tfar:
                tfar = t2
            if tnear > tfar or tfar < 0.0:
                return None
    t = tfar if tnear < 0 else tnear
    return np.array([pos[a] + d[a] * t for a in range(3)], np.float32)


def tiny_families(info):
    g = Grid(info)
    n = [int(info.nx), int(info.ny), int(info.nz)]
    waves = []
    # coherent waves along every edge: clamped tiles at every face
    for a in range(3):
        o = [b for b in range(3) if b != a]
        for s1 in (0, 1):
            for s2 in (0, 1):
                for up in (True, False):
                    L = np.empty((W, 3))
                    L[:, o[0]] = 1.05 if s1 == 0 else n[o[0]] - 1.05
                    L[:, o[1]] = 1.05 if s2 == 0 else n[o[1]] - 1.05
                    L[:, a] = 1.2 if up else n[a] - 1.2
                    d = np.zeros(3)
                    d[a] = 1.0 if up else -1.0
                    d[o[0]] = 1e-3
                    waves.append(_wave(g, L, d))
    # incoherent waves at every corner: lanes over a 3 x 3 patch of cells, clamped bricks
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                L = np.empty((W, 3))
                k = np.arange(W)
                L[:, 0] = (1.1 + (k % 3) * 0.9) if cx == 0 else (n[0] - 1.1 - (k % 3) * 0.9)
                L[:, 1] = (1.1 + ((k // 3) % 3) * 0.9) if cy == 0 else (n[1] - 1.1 - ((k // 3) % 3) * 0.9)
                L[:, 2] = 1.2 if cz == 0 else n[2] - 1.2
                waves.append(_wave(g, L, (0.001, 0.002, 1.0 if cz == 0 else -1.0)))
    return [_family("tiny_faces", "tiny", waves,
                    {"C": ["C_TILE_CLAMPED", "C_BRICK_CLAMPED"], "L": ["L_TILE_CLAMPED", "L_BRICK_CLAMPED"]})]


def const_families(info):
    g = Grid(info)
    waves = [_wave(g, _column(5, 5, 1.5, seed=20), (0.01, 0.003, 1)), _wave(g, _column(4, 7, 10.5, seed=21), (0, 0.004, -1))]
    k = np.arange(W)
    L = np.stack([1.3 + (k % 8) * 1.2, 1.4 + (k // 8) * 1.2, np.full(W, 1.5)], 1)
    waves.append(_wave(g, L, (0.02, -0.01, 1)))
    return [_family("constant", "const", waves, {"C": ["C_SPIN_LOW"], "L": []})]


def vacuum_families(info):
    """The trilinear repair.  The blends are fmaf(t, b - a, a), and an 8-bit weight can be exactly 1: lanes a thousandth of
    a cell short of the vacuum line's texel centre in x (weight 255.5/256 or more: 1) and on a texel centre in y (weight 0)
    blend the dense texel a and the vacuum texel b < ulp(a) / 2, where fl(b - a) = -a -- the blend is 0, below data_min = b.
    A ray's first such sample has no value before it (val_prev 0): resampled one layer down; the later ones keep val_prev.
    Exact weights stay below 1 (or meet two equal clamped texels), so each blend lies between its corners: no repair."""
    g = Grid(info)
    rng = np.random.default_rng(22)
    waves = []
    for lz, dz in ((1.6, 1.0), (float(info.nz) - 1.6, -1.0)):
        L = np.empty((W, 3))
        L[:, 0] = VAC_I + 0.499 + rng.uniform(-4e-4, 4e-4, W)      # x - 0.5 - floor(x - 0.5) = 0.999 -> weight 1 (8 bits)
        L[:, 1] = VAC_J + 0.5                                       # on the texel centre: weight 0
        L[:, 2] = lz + rng.uniform(0, 0.8, W)
        waves.append(_wave(g, L, (0, 0, dz)))
    return [_family("repair", "vac", waves, {"C": [], "L": ["L_LOW", "L_REPAIR_LANES", "L_KEEP_PREV_LANES"]})]


def all_families(infos: dict):
    """infos: {volume: info} of the volumes volume_density() describes (VOLUMES)."""
    return (mid_families(infos["mid"]) + tiny_families(infos["tiny"]) + const_families(infos["const"])
            + vacuum_families(infos["vac"]))


# the sampler / weight modes of the matrix: (name, interpolation, trilinear weight bits)
SAMPLERS = (("L8", 1, 8), ("L0", 1, 0), ("C", 2, 0))
ALGORITHMS = (1, 2)
SEGMENTS = (1, 3, 7)


def oracle_results(oracle):
    """The oracle's march of every family, sampler and algorithm: {key: array}, keys f"{family}/{sampler}/{algorithm}/{pos|dir|steps}"."""
    vols = {k: {s: oracle.volume_from_density(*volume_density(k), interp, tex_frac_bits=bits if interp == 1 else 8)
                for s, interp, bits in SAMPLERS} for k in VOLUMES}
    fams = all_families({k: v["L8"].info() for k, v in vols.items()})
    out = {}
    for f in fams:
        for s, _, _ in SAMPLERS:
            for a in ALGORITHMS:
                p, d, st = vols[f.volume][s].trace_rays(f.pos, f.dir, a)
                out[f"{f.name}/{s}/{a}/pos"], out[f"{f.name}/{s}/{a}/dir"], out[f"{f.name}/{s}/{a}/steps"] = p, d, st
    for v in vols.values():
        for x in v.values():
            x.free()
    return fams, out


def adversarial_case(seed: int):
    """The fuzz of tests/test_parity_gpu.py::test_march_bit_exact_on_adversarial_cases: (rho, spacing, origin, rays), where
    rays(info) builds the next 4096 rays from the volume's bounds -- call it once per sampler, trilinear first, tricubic
    second: both share one generator, as the test always has."""
    rng = np.random.default_rng(1000 + seed)
    dims = [(4, 5, 33), (17, 4, 9), (12, 12, 12), (40, 7, 21), (9, 31, 6), (24, 20, 28)][seed]          # nz, ny, nx
    z, y, x = np.meshgrid(*(np.linspace(-1, 1, k) for k in dims), indexing="ij")
    if seed == 2:
        rho = np.full(dims, 1.225, np.float32)                                         # constant: n - 1 == data_min everywhere
    else:
        rho = (1.2 + 0.4 * np.exp(-(x ** 2 + 2 * y ** 2 + 0.5 * z ** 2) * 2) + 0.05 * rng.standard_normal(dims)).astype(np.float32)
    spacing = tuple(float(v) for v in rng.uniform(80.0, 400.0, 3))
    origin = (-1000.0, 500.0, 750e3 + 2000.0)

    def rays(i, n=4096):
        lo, hi = np.array(i.min_bound, np.float64), np.array(i.max_bound, np.float64)
        ext = hi - lo
        centre = 0.5 * (lo + hi)
        # starts on a sphere around the box, aimed at random points of it; then the special families
        u = rng.standard_normal((n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        pos = centre + u * 1.5 * np.linalg.norm(ext)
        target = lo + rng.uniform(-0.05, 1.05, (n, 3)) * ext
        d = target - pos
        pos[:400] = lo + rng.uniform(0, 1, (400, 3)) * ext                              # inside starts
        d[:400] = rng.standard_normal((400, 3))
        k = np.arange(400, 800)                                                        # axis-parallel, from outside
        axis = rng.integers(0, 3, k.size)
        d[k] = 0.0
        d[k, axis] = np.where(pos[k, axis] > centre[axis], -1.0, 1.0)
        pos[k] = lo + rng.uniform(0.01, 0.99, (k.size, 3)) * ext
        pos[k, axis] = np.where(d[k, axis] < 0, hi[axis] + 300.0, lo[axis] - 300.0)
        k = np.arange(800, 1000)                                                       # start exactly on the max-z face, heading in
        pos[k] = lo + rng.uniform(0.05, 0.95, (k.size, 3)) * ext
        pos[k, 2] = np.float32(hi[2])
        d[k] = np.stack([rng.normal(0, 0.2, k.size), rng.normal(0, 0.2, k.size), -np.ones(k.size)], 1)
        d[1000:1100] *= -1.0                                                           # pointing away: a miss
        pos[1100:1164] = pos[1100] + rng.uniform(-1e-3, 1e-3, (64, 3))                 # one fully coherent wave's worth
        d[1100:1164] = d[1100]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        order = rng.permutation(n)
        order[:1164] = np.arange(1164)                                                 # families contiguous, the rest shuffled
        return pos[order], d[order]

    return rho, spacing, origin, rays


ADVERSARIAL_SEEDS = range(6)


def adversarial_rays(seed: int, info):
    """{1: (pos, dir), 2: (pos, dir)}: the fuzz rays of one seed for the trilinear and the tricubic sampler."""
    rho, spacing, origin, rays = adversarial_case(seed)
    return {1: rays(info), 2: rays(info)}


def oracle_adversarial(oracle):
    """The oracle's march of the fuzz rays: keys f"adv{seed}/{sampler}/{algorithm}/{pos|dir|steps}"."""
    out = {}
    for seed in ADVERSARIAL_SEEDS:
        rho, spacing, origin, _ = adversarial_case(seed)
        vols = {s: oracle.volume_from_density(rho, spacing, origin, interp, tex_frac_bits=bits if interp == 1 else 8)
                for s, interp, bits in SAMPLERS}
        rays = adversarial_rays(seed, vols["L8"].info())
        for s, interp, _ in SAMPLERS:
            for a in ALGORITHMS:
                p, d, st = vols[s].trace_rays(*rays[interp], a)
                out[f"adv{seed}/{s}/{a}/pos"], out[f"adv{seed}/{s}/{a}/dir"], out[f"adv{seed}/{s}/{a}/steps"] = p, d, st
        for v in vols.values():
            v.free()
    return out


# renders through the real launch path (start_ray_tracing with sensor moments), compared with the records the host model
# (photon_amd.deflections.moments_from_dumps) makes of the oracle's ray dumps
RENDER_EXACT = [0, 1, 2, 3, 7]          # n, position sums, sum r^2: bit for bit


def render_call(name: str, nrrd: str, algorithm: int):
    """A small source-major BOS scene and a small lens-major PIV scene (full-aperture cones), both through the volume."""
    from photon_amd import scenes
    if name == "bos":
        c = scenes.bos_scene(n_dots=4, points_per_dot=8, rays_per_source=120, density_grad_filename=nrrd, seed=4)
    else:
        c = scenes.piv_scene(n_particles=160, rays_per_source=40, mie=False, density_grad_filename=nrrd, field_half_width=3.0e4,
                             seed=6)
    c.ray_tracing_algorithm = algorithm
    return c


RENDERS = ("bos", "piv")


def render_volume(path: str) -> str:
    from photon_amd import scenes
    rho, sp, org = scenes.bos_volume(40)
    return scenes.write_nrrd(path, rho, sp, org)


def oracle_render_records(oracle, nrrd: str, workdir: str):
    """Records of the oracle's ray dumps: keys f"render/{scene}/{interp}/{algorithm}"."""
    import os

    from photon_amd import deflections as dfl
    out = {}
    for name in RENDERS:
        for interp in (1, 2):
            for a in ALGORITHMS:
                c = render_call(name, nrrd, a)
                d = os.path.join(workdir, f"dump_{name}_{interp}_{a}")
                os.makedirs(d, exist_ok=True)
                c.save_lightrays, c.num_lightrays_save = True, c.num_rays
                c.lightray_position_save_path = c.lightray_direction_save_path = d
                oracle.render(c, interpolation=interp)
                pos = np.fromfile(os.path.join(d, "pos_0000.bin"), np.float32).reshape(-1, 3)
                dirs = np.fromfile(os.path.join(d, "dir_0000.bin"), np.float32).reshape(-1, 3)
                out[f"render/{name}/{interp}/{a}"] = dfl.moments_from_dumps(pos, dirs, c.lightray_number_per_particle)
    return out
