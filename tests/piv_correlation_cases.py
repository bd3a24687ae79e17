"""Shared cases of the exact correlation tests (test_piv_correlation.py, test_piv_correlation_gpu.py): image pairs on which
every f32 operation of photon_piv_correlate is exact, so that the device can be held bit for bit against the f64 model.

The exactness condition, per window that is not flat by definition (``assert_exact`` checks it from the images alone):

* every pixel the window reads is an integer-valued f32, and the sums of |pixel| over the window stay below 2^24;
* mean a and mean b (over the in-image pixels of the zero-shift window) are integers;
* sum a^2, sum b^2 and max |b| * sum |a| (mean-subtracted; a bound of sum |a| |b| for every shift) stay below 2^24.

Then every partial sum of the kernel is an integer below 2^24 in any order: C, ea and eb equal the model's, and what follows
(1 / sqrt(ea eb), the products with it, the ratio, the parabolic fit) are the same correctly rounded f64 operations on both
sides.  Only the Gaussian fit's log may differ in its last bit.

A window is flat by definition when all win^2 pixels of a are equal, or when the in-image pixels of b at zero shift are all
equal or there are none; for f32 pixels (at most 4096 equal values: their f64 sums are exact) that is when the model's
energies are 0.  Such windows may hold any finite value -- the constant families use values that are not dyadic.

The periodic construction: an integer tile of win x win (rounded Gaussian blobs 0 .. 3, then -1 on as many empty pixels as
make its sum 0), tiled, plus an integer constant; im2's tile is p roll(tile, s) + q roll(tile, s + (1, 0)) + r roll(tile,
s + (0, 1)).  A win-periodic image has the same sum over every win x win window, so both means are the constants for any
step and any offset that keeps the zero-shift window inside the image.
"""
import dataclasses
import functools
from typing import Optional

import numpy as np

from photon_amd import piv_correlation as pc

LIMIT = 1 << 24
TILE = 4                # shifts per lane and axis in the kernel: tied shifts in different tiles belong to different lanes
REPS = 3


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    family: str         # "plan", "offset", "pixels", "planted", "constant"
    win: int
    step: int
    R: int
    im1: np.ndarray     # f32 [height, width]
    im2: np.ndarray
    offset: Optional[np.ndarray] = None         # int32 [n_rows, n_cols, 2] (ox, oy)

    @property
    def grid(self):
        return pc.grid_shape(self.im1.shape, self.win, self.step)


# ---- what the windows read, from the images alone -------------------------------------------------------------------------
def _windows(case: Case):
    """(a [n, win, win], b [n, span, span], inside [n, span, span]) as f64 raw pixels; b 0 outside the image."""
    win, step, R = case.win, case.step, case.R
    H, W = case.im1.shape
    n_rows, n_cols = case.grid
    k = np.arange(n_rows * n_cols)
    wy0, wx0 = (k // n_cols) * step, (k % n_cols) * step
    o = np.zeros((k.size, 2), np.int64) if case.offset is None else np.asarray(case.offset, np.int64).reshape(k.size, 2)
    iw, isp = np.arange(win), np.arange(win + 2 * R)
    a = case.im1.astype(np.float64)[(wy0[:, None] + iw)[:, :, None], (wx0[:, None] + iw)[:, None, :]]
    gy, gx = wy0[:, None] + o[:, 1:2] - R + isp, wx0[:, None] + o[:, 0:1] - R + isp
    inside = ((gy >= 0) & (gy < H))[:, :, None] & ((gx >= 0) & (gx < W))[:, None, :]
    b = case.im2.astype(np.float64)[np.clip(gy, 0, H - 1)[:, :, None], np.clip(gx, 0, W - 1)[:, None, :]]
    return a, np.where(inside, b, 0.0), inside


def window_stats(case: Case):
    """Per window, from the images alone: flat_a, flat_b (the definition: all pixels equal / all in-image pixels of b at zero
    shift equal, or none), outside (a pixel of the search region lies outside the image), and the raw windows."""
    a, b, inside = _windows(case)
    R, win = case.R, case.win
    z = (slice(None), slice(R, R + win), slice(R, R + win))
    bz, iz = b[z], inside[z]
    flat_a = a.max(axis=(1, 2)) == a.min(axis=(1, 2))
    hi = np.where(iz, bz, -np.inf).max(axis=(1, 2))
    lo = np.where(iz, bz, np.inf).min(axis=(1, 2))
    flat_b = ~iz.any(axis=(1, 2)) | (hi == lo)
    return dict(a=a, b=b, inside=inside, bz=bz, iz=iz, flat_a=flat_a, flat_b=flat_b, outside=~inside.all(axis=(1, 2)))


def energies(case: Case):
    """(ea, eb) per window as exact integers (f64 holding them), 0 on windows that are flat by definition."""
    s = window_stats(case)
    cnt = s["iz"].sum(axis=(1, 2))
    a = s["a"] - s["a"].mean(axis=(1, 2))[:, None, None]
    mb = np.where(s["iz"], s["bz"], 0.0).sum(axis=(1, 2)) / np.maximum(cnt, 1)
    bz = np.where(s["iz"], s["bz"] - mb[:, None, None], 0.0)
    flat = s["flat_a"] | s["flat_b"]
    return np.where(flat, 0.0, (a * a).sum(axis=(1, 2))), np.where(flat, 0.0, (bz * bz).sum(axis=(1, 2)))


def assert_exact(case: Case):
    """The exactness condition of the module's docstring on every window that is not flat by definition."""
    assert case.im1.dtype == np.float32 and case.im2.dtype == np.float32 and case.im1.shape == case.im2.shape
    assert np.isfinite(case.im1).all() and np.isfinite(case.im2).all()
    s = window_stats(case)
    live = ~(s["flat_a"] | s["flat_b"])
    a, b, inside, iz = s["a"][live], s["b"][live], s["inside"][live], s["iz"][live]
    R, win = case.R, case.win
    bz = b[:, R:R + win, R:R + win]
    assert (a == np.rint(a)).all() and (b == np.rint(b)).all(), f"{case.name}: a pixel is not an integer"
    assert iz.all(), f"{case.name}: a zero-shift window leaves the image"
    assert np.abs(a).sum(axis=(1, 2)).max(initial=0) < LIMIT and np.abs(bz).sum(axis=(1, 2)).max(initial=0) < LIMIT
    sa, sb = a.sum(axis=(1, 2)), bz.sum(axis=(1, 2))
    n_pix = win * win
    assert (sa % n_pix == 0).all() and (sb % n_pix == 0).all(), f"{case.name}: a window mean is not an integer"
    a = a - (sa / n_pix)[:, None, None]
    b = np.where(inside, b - (sb / n_pix)[:, None, None], 0.0)
    bz = b[:, R:R + win, R:R + win]
    assert (a * a).sum(axis=(1, 2)).max(initial=0) < LIMIT and (bz * bz).sum(axis=(1, 2)).max(initial=0) < LIMIT
    bound = np.abs(b).max(axis=(1, 2), initial=0) * np.abs(a).sum(axis=(1, 2))
    assert bound.max(initial=0) < LIMIT, f"{case.name}: sum |a| |b| may reach {bound.max()}"


# ---- the model's outputs, once per case, and the path each window takes ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name: str):
    """correlate_model on the named case: (vectors [n, 4] f64, flags [n], planes [n, nS, nS] f64).  Treat as read-only."""
    c = all_cases()[name]
    v, f, p = pc.correlate_model(c.im1, c.im2, c.win, c.step, c.R, offset=c.offset, planes=True)
    out = (v.reshape(-1, 4), f.ravel(), p.reshape(f.size, 2 * c.R + 1, 2 * c.R + 1))
    for x in out:
        x.setflags(write=False)
    return out


def classify(case: Case, vectors, flags, planes):
    """The path every window takes, from the model's outputs (vectors [n, 4], flags [n], planes [n, nS, nS]): a dict of bool
    [n] arrays.  The three values through the peak are the planes times sqrt(ea eb), rounded: the integers C."""
    R, nS = case.R, 2 * case.R + 1
    n = flags.size
    k = np.arange(n)
    flat = (flags & pc.FLAG_FLAT) != 0
    ea, eb = energies(case)
    C = np.rint(np.where(flat[:, None, None], 0.0, planes) * np.sqrt(ea * eb)[:, None, None])
    Cf = C.reshape(n, -1)
    best = np.argmax(Cf, axis=1)
    py, px = best // nS, best % nS
    top = Cf == Cf[k, best][:, None]
    tiles = (np.arange(nS)[:, None] // TILE) * nS + np.arange(nS)[None, :] // TILE         # the 4 x 4 tile of every shift
    other_tile = (top & (tiles.ravel()[None, :] != tiles[py, px][:, None])).any(axis=1)
    edge_x, edge_y = (px == 0) | (px == nS - 1), (py == 0) | (py == nS - 1)
    pxi, pyi = np.clip(px, 1, nS - 2), np.clip(py, 1, nS - 2)
    o = np.zeros((n, 2)) if case.offset is None else np.asarray(case.offset, np.float64).reshape(n, 2)
    live = ~flat
    out = dict(flat=flat, live=live, px=px, py=py)
    for ax, edge, (cm, c0, cp), delta in (("x", edge_x, (C[k, py, pxi - 1], C[k, py, pxi], C[k, py, pxi + 1]),
                                           vectors[:, 0] - (o[:, 0] + px - R)),
                                          ("y", edge_y, (C[k, pyi - 1, px], C[k, pyi, px], C[k, pyi + 1, px]),
                                           vectors[:, 1] - (o[:, 1] + py - R))):
        fit = live & ~edge
        gauss = fit & (cm > 0) & (c0 > 0) & (cp > 0)
        nonzero = np.nan_to_num(delta) != 0.0
        out["gauss_" + ax] = gauss
        out["gauss_nonzero_" + ax] = gauss & nonzero
        out["parabolic_" + ax] = fit & ~gauss
        out["parabolic_nonzero_" + ax] = fit & ~gauss & nonzero
        # (the parabolic denominator; the Gaussian one is 0 only when cm cp = c0^2)
        out["zero_den_" + ax] = fit & np.where(gauss, cm * cp == c0 * c0, cm - 2.0 * c0 + cp == 0.0)
    out["edge_x_only"] = live & edge_x & ~edge_y
    out["edge_y_only"] = live & edge_y & ~edge_x
    out["edge_both"] = live & edge_x & edge_y
    out["inner"] = live & ~edge_x & ~edge_y
    out["tie"] = live & (top.sum(axis=1) > 1)
    out["tie_other_tile"] = live & other_tile
    inf = live & np.isposinf(np.where(flat, 0.0, vectors[:, 3]))
    no_far = (nS == 3) & (px == 1) & (py == 1)
    out["ratio_one"] = live & (np.where(flat, 0.0, vectors[:, 3]) == 1.0)
    out["ratio_inf_no_far_shift"] = inf & no_far
    out["ratio_inf_far_not_positive"] = inf & ~no_far
    s = window_stats(case)
    integer_a = (s["a"] == np.rint(s["a"])).all(axis=(1, 2))
    integer_b = (s["b"] == np.rint(s["b"])).all(axis=(1, 2))
    out["flat_a"] = flat & s["flat_a"]
    out["flat_b"] = flat & s["flat_b"] & ~s["flat_a"]
    out["flat_outside"] = flat & s["outside"]
    out["flat_constant_a"] = flat & s["flat_a"] & ~integer_a        # a constant that is no integer
    out["flat_constant_b"] = flat & s["flat_b"] & ~integer_b
    return out


# ---- the periodic construction --------------------------------------------------------------------------------------------
def make_tile(win: int, seed: int) -> np.ndarray:
    """An integer tile [win, win] with values -1 .. 3 and sum 0: rounded periodic Gaussian blobs (sigma 1, peak 3, centres
    at sub-pixel positions), then -1 on as many empty pixels as the blobs sum to."""
    rng = np.random.default_rng(seed)
    t = np.zeros((win, win), np.int64)
    d = np.arange(-3, 4)
    for _ in range(max(2, win * win // 64)):
        cy, cx = rng.uniform(0, win, 2)
        iy, ix = int(np.floor(cy)), int(np.floor(cx))
        g = np.rint(3.0 * np.exp(-((iy + d[:, None] - cy) ** 2 + (ix + d[None, :] - cx) ** 2) / 2.0)).astype(np.int64)
        np.add.at(t, (((iy + d) % win)[:, None], ((ix + d) % win)[None, :]), g)
    t = np.minimum(t, 3)
    empty = np.flatnonzero(t == 0)
    total = int(t.sum())
    assert 0 < total <= empty.size
    t.ravel()[rng.choice(empty, total, replace=False)] = -1
    assert t.sum() == 0
    return t


def periodic_pair(tile, shift, p=2, q=1, r=1, c1=7, c2=12, reps=REPS, crop=(0, 0)):
    """(im1, im2) f32: the tile and its shifted mix, tiled reps x reps, plus the constants, cut by `crop` rows / columns.
    shift = (sx, sy): im2(p + s) = im1(p), a pattern moved right and down gives positive values."""
    sx, sy = shift
    t2 = (p * np.roll(tile, (sy, sx), (0, 1)) + q * np.roll(tile, (sy, sx + 1), (0, 1)) + r * np.roll(tile, (sy + 1, sx), (0, 1)))
    im1, im2 = np.tile(tile, (reps, reps)) + c1, np.tile(t2, (reps, reps)) + c2
    h, w = im1.shape[0] - crop[0], im1.shape[1] - crop[1]
    return im1[:h, :w].astype(np.float32), im2[:h, :w].astype(np.float32)


def pull_offsets(shape, win, step, pull):
    """Offsets of `pull` = (ox, oy) on every second window that can take them with its zero-shift window inside the image."""
    n_rows, n_cols = pc.grid_shape(shape, win, step)
    off = np.zeros((n_rows, n_cols, 2), np.int32)
    i, j = np.meshgrid(np.arange(n_rows), np.arange(n_cols), indexing="ij")
    y0, x0 = i * step + pull[1], j * step + pull[0]
    ok = (y0 >= 0) & (y0 + win <= shape[0]) & (x0 >= 0) & (x0 + win <= shape[1])
    take = np.zeros_like(ok)
    take.ravel()[np.flatnonzero(ok)[::2]] = True
    off[take] = pull
    return off


# steps per window size, cycled over the radii: steps that do not divide win, steps that do, and step == win
STEPS = {16: (16, 5, 8, 11, 7, 16, 12, 9), 32: (32, 12, 20, 27, 16, 11, 23, 32), 64: (64, 40, 56, 48, 33, 64, 50, 32)}


def plan_case(win: int, R: int) -> Case:
    """One case of the "every plan" family.  R = 1: a centre peak.  R divisible by 4: the shift on the x edge of the search
    square (at R = win / 2 the periodicity ties -R with +R), R = 2 mod 4: on the y edge, R = 5 mod 8: on both; on those,
    every second window takes an offset of one pixel that pulls its peak inside.  Other radii: a shift inside."""
    rng = np.random.default_rng(1000 * win + R)
    step = STEPS[win][(R - 1) % 8]
    inner = lambda: int(rng.integers(-(R - 1), R))                     # noqa: E731
    sign = lambda: int(rng.choice((-1, 1)))                            # noqa: E731
    pull = None
    if R == 1:
        shift = (0, 0)
    elif R % 4 == 0:
        gx = sign()
        shift, pull = (gx * R, inner()), (gx, 0)
    elif R % 4 == 2:
        gy = sign()
        shift, pull = (inner(), gy * R), (0, gy)
    elif R % 8 == 5:
        gx, gy = sign(), sign()
        shift, pull = (gx * R, gy * R), (gx, gy)
    else:
        shift = (inner(), inner())
    im1, im2 = periodic_pair(make_tile(win, 7 * win + R), shift, c1=3 + R % 5, c2=10 + R % 7, crop=(R % 3, 2 * (R % 2)))
    off = pull_offsets(im1.shape, win, step, pull) if pull else None
    return Case(f"plan_w{win}_r{R}_s{step}", "plan", win, step, R, im1, im2, off)


def offset_case(win: int, R: int, step: int, shift) -> Case:
    """A shift well outside the radius and a per-window integer predictor near it (within 2 pixels, so some peaks land on
    the edge of the search square), moved back where the zero-shift window would leave the image."""
    rng = np.random.default_rng(50 * win + R)
    im1, im2 = periodic_pair(make_tile(win, 3 * win + R), shift, p=3, q=1, r=2, c1=21, c2=5, crop=(3, 0))
    n_rows, n_cols = pc.grid_shape(im1.shape, win, step)
    off = np.asarray(shift)[None, None, :] + rng.integers(-2, 3, (n_rows, n_cols, 2))
    i, j = np.meshgrid(np.arange(n_rows), np.arange(n_cols), indexing="ij")
    off[..., 0] = np.clip(off[..., 0], -j * step, im1.shape[1] - win - j * step)
    off[..., 1] = np.clip(off[..., 1], -i * step, im1.shape[0] - win - i * step)
    return Case(f"offset_w{win}_r{R}_s{step}", "offset", win, step, R, im1, im2, off.astype(np.int32))


# ---- hand-made pixels: one bright pixel per window, of win^2 so that the window's mean is 1 --------------------------------
def pixel_case(win: int, R: int = 4) -> Case:
    """5 x 5 windows, step = win.  Window (i, j) of im1 holds one pixel of win^2 at its centre; im2 holds pixels of m win^2
    at the listed (dx, dy, m) from it.  Every C is then 0, -(sum m) win^2 or win^2 (m win^2 - sum m) -- a neighbour <= 0
    takes the parabolic fit."""
    V, c = win * win, win // 2
    im1 = np.zeros((5 * win, 5 * win))
    im2 = np.zeros_like(im1)
    plants = {
        (1, 1): [(R, -1, 1)],                                   # the edge in x only
        (1, 2): [(2, -R, 1)],                                   # the edge in y only
        (1, 3): [(-R, R, 1)],                                   # both edges
        (2, 1): [(1, -2, 1), (-2, 1, 1)],                       # an exact tie across shift tiles: the earlier shift, ratio 1
        (2, 2): [(1, 0, 2), (2, 0, 1)],                         # parabolic in x, the neighbours differ
        (2, 3): [(-3, 3, 1)],                                   # nothing positive two shifts away: ratio +inf
        (3, 1): [(0, 0, 1)],                                    # (a is made constant below)
        (3, 2): [],                                             # b flat at zero shift
        (3, 3): [(0, 1, 2), (0, 2, 1)],                         # parabolic in y
        (0, 2): [(1, 1, 1)],                                    # on the border: outside, not flat
        (2, 0): [],                                             # flat b and outside
        (2, 4): [(-1, 0, 1)],
    }
    for (i, j), pix in plants.items():
        im1[i * win + c, j * win + c] = V
        for dx, dy, m in pix:
            im2[i * win + c + dy, j * win + c + dx] = m * V
    im1[3 * win:4 * win, win:2 * win] = 5.0                     # flat a, inside
    im1[:win, :win] = 2.0                                       # flat a and outside (b flat too); every other window: both flat
    return Case(f"pixels_w{win}_r{R}", "pixels", win, win, R, im1.astype(np.float32), im2.astype(np.float32))


def planted_case(win: int, R: int, reps: int) -> Case:
    """Integer constants planted on whole windows of a periodic pair (step = win): flat a inside, flat a on the border, flat
    b at zero shift on the border -- whose pixels also enter the search margins of its neighbours."""
    im1, im2 = periodic_pair(make_tile(win, 11 * win), (1, -2), c1=6, c2=9, reps=reps)
    im1[win:2 * win, win:2 * win] = 9.0
    im1[:win, :win] = 2.0
    im2[win:2 * win, 2 * win:3 * win] = 4.0
    return Case(f"planted_w{win}_r{R}", "planted", win, win, R, im1, im2)


# ---- constants that are not dyadic: the kernel's own f32 sums, replayed ----------------------------------------------------
def plan_threads(win: int, R: int, lds_limit: int = 160 * 1024) -> int:
    """The workgroup size the library's plan takes for (win, R) on a device with `lds_limit` bytes of LDS per workgroup.
    Used only to replay the sums below (which constants an f32 mean does not reproduce); no test depends on the plan."""
    nS = 2 * R + 1
    nSp = (nS + TILE - 1) // TILE * TILE
    units = (nSp // TILE) ** 2
    fixed = win * win + (win + nSp - 1) * (win + nSp) + 64
    best, best_cost = 0, None
    for K in range(1, min(8, win // 4) + 1):
        if 4 * (fixed + K * nSp * nSp) > lds_limit:
            break
        items = units * K
        threads = min(512, (items + 63) // 64 * 64)
        cost = -(-items // threads) * threads * (-(-win // K))
        if best_cost is None or cost < best_cost:
            best, best_cost = threads, cost
    return best


def replay_mean(c, win: int, threads: int) -> np.float32:
    """The f32 mean a workgroup of `threads` lanes finds for a window of win^2 copies of c, in the kernel's order: every lane
    adds its strided pixels one by one, a 64-lane butterfly (offsets 32 .. 1) per wave, then the wave totals in wave order."""
    c = np.float32(c)
    count = np.array([len(range(t, win * win, threads)) for t in range(threads)])
    lane = np.zeros(threads, np.float32)
    for i in range(int(count.max())):
        lane = np.where(count > i, lane + c, lane).astype(np.float32)
    lanes = np.arange(threads)
    for o in (32, 16, 8, 4, 2, 1):
        lane = (lane + lane[lanes ^ o]).astype(np.float32)
    total = np.float32(0.0)
    for w in range(threads // 64):
        total = np.float32(total + lane[64 * w])
    return np.float32(total / np.float32(win * win))


def pick_constant(win: int, R: int, seed: int = 0) -> np.float32:
    """The first of a seeded sequence of constants in [0.01, 100] whose replayed mean differs from it: a window of this
    value has f32 energies above 0 although all its pixels are equal."""
    rng = np.random.default_rng(seed)
    threads = plan_threads(win, R)
    for _ in range(1000):
        c = np.float32(rng.uniform(0.01, 100.0))
        if replay_mean(c, win, threads) != c:
            return c
    raise AssertionError(f"no constant found for win {win}, radius {R}: the replay calls every one flat")


def constant_case(win: int, R: int, which: str) -> Case:
    """which = "a": two windows of im1 (one inside, one on the border) set to a constant that is not dyadic, on a periodic
    pair with step = win; "b": all of im2 set to such a constant -- every window is flat."""
    c = pick_constant(win, R, seed=win + R)
    im1, im2 = periodic_pair(make_tile(win, 13 * win + R), (2, 1), c1=4, c2=15)
    if which == "a":
        im1[win:2 * win, win:2 * win] = c
        im1[:win, 2 * win:3 * win] = c
    else:
        im2[...] = c
    return Case(f"constant_{which}_w{win}_r{R}", "constant", win, win, R, im1, im2)


CONSTANT_CONFIGS = ((32, 4, "a"), (32, 8, "a"), (64, 8, "a"), (64, 32, "a"), (32, 4, "b"), (64, 32, "b"))


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: Case} of every family, in a fixed order."""
    cases = [plan_case(win, R) for win in (16, 32, 64) for R in range(1, win // 2 + 1)]
    cases += [offset_case(16, 3, 11, (6, -5)), offset_case(32, 5, 23, (-9, 12)), offset_case(64, 7, 50, (20, 17))]
    cases += [pixel_case(16), pixel_case(32)]
    cases += [planted_case(16, 3, 4), planted_case(32, 6, 4), planted_case(64, 9, 3)]
    cases += [constant_case(*cfg) for cfg in CONSTANT_CONFIGS]
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    for c in cases:
        c.im1.setflags(write=False)
        c.im2.setflags(write=False)
    return out


def names(family=None):
    return [n for n, c in all_cases().items() if family is None or c.family == family]
