"""Shared cases of the ensemble-correlation tests (test_piv_ensemble.py, test_piv_ensemble_gpu.py; section 14 of
include/parallel_ray_tracing.h):

* the exact stacks: N pairs of the periodic integer construction of piv_correlation_cases.py, one shape, win, step and R per
  stack, another tile seed and shift per pair, one pair with whole windows set to a constant (flat there).  Every pair
  passes ``assert_exact``, and the sums over the pairs of ea, of eb and of max |b| sum |a| stay below 2^24
  (``assert_exact_stack``): then every partial sum of the ensemble kernel is an integer below 2^24 in any order, so C, Ea
  and Eb equal the f64 model's and what follows is the same correctly rounded f64 arithmetic on both sides;
* the particle stacks: N pairs of one uniform shift with fresh particles per pair;
* the sparse stack of the issue: 16 pairs at 0.002 particles per pixel, where no single pair gives a whole field and the
  sum does.
"""
import dataclasses
import functools
from typing import Optional

import numpy as np

import piv_correlation_cases as cc
from photon_amd import piv_correlation as pc
from photon_amd import piv_ensemble as pe


@dataclasses.dataclass(frozen=True, eq=False)
class Stack:
    name: str
    win: int
    step: int
    R: int
    im1: np.ndarray     # f32 [N, height, width]
    im2: np.ndarray
    offset: Optional[np.ndarray] = None         # int32 [n_rows, n_cols, 2] (ox, oy), shared by all pairs

    @property
    def n_pairs(self):
        return self.im1.shape[0]

    @property
    def grid(self):
        return pc.grid_shape(self.im1.shape[1:], self.win, self.step)

    def pair(self, k: int) -> cc.Case:
        return cc.Case(f"{self.name}[{k}]", "ensemble", self.win, self.step, self.R, self.im1[k], self.im2[k], self.offset)


# ---- the exact stacks ---------------------------------------------------------------------------------------------------
def exact_stack(name, win, R, reps, shifts, seed, flat_pair, offset_pull=None, plant_b=True) -> Stack:
    """step = win, reps x reps windows.  Pair k: tile seed + k, shift shifts[k], its own mix and constants.  Pair `flat_pair`
    has window (1, 1) of im1 and window (0, 0) of im1 constant, and (plant_b) window (1, 2) of im2: whole windows, so that
    every other window keeps its integer mean.  offset_pull: every second window takes that offset."""
    ims1, ims2 = [], []
    for k, shift in enumerate(shifts):
        im1, im2 = cc.periodic_pair(cc.make_tile(win, seed + k), shift, p=2 + k % 2, q=1, r=1 + k % 3, c1=4 + k, c2=11 - k, reps=reps)
        if k == flat_pair:
            im1[win:2 * win, win:2 * win] = 9.0
            im1[:win, :win] = 2.0
            if plant_b:
                im2[win:2 * win, 2 * win:3 * win] = 4.0
        ims1.append(im1)
        ims2.append(im2)
    im1, im2 = np.stack(ims1), np.stack(ims2)
    off = cc.pull_offsets(im1.shape[1:], win, win, offset_pull) if offset_pull else None
    im1.setflags(write=False)
    im2.setflags(write=False)
    return Stack(name, win, win, R, im1, im2, off)


@functools.lru_cache(maxsize=None)
def exact_stacks():
    """{name: Stack}: win 16 at R = win / 2 (ties between -R and +R of a periodic pattern), win 32 with offsets (no constant
    planted in im2: an offset window would take a part of it), win 64; 5 to 6 pairs each."""
    stacks = [
        exact_stack("exact_w16_r8", 16, 8, 4, [(2, -1), (3, -1), (2, -2), (2, -1), (1, 0), (2, -1)], 400, flat_pair=2),
        exact_stack("exact_w32_r5_off", 32, 5, 3, [(4, -2), (5, -3), (4, -3), (3, -2), (4, -2)], 500, flat_pair=0, offset_pull=(4, -2),
                    plant_b=False),
        exact_stack("exact_w64_r7", 64, 7, 3, [(-3, 5), (-3, 4), (-2, 5), (-3, 5), (-4, 6)], 600, flat_pair=4),
    ]
    return {s.name: s for s in stacks}


def stack_energies(stack: Stack):
    """Per pair and window, exact integers held in f64: (ea, eb, max |b| sum |a|) [N, n], 0 where the pair's window is flat by
    definition -- the three quantities whose sums over the pairs bound every partial sum of the ensemble."""
    ea, eb, bound = [], [], []
    for k in range(stack.n_pairs):
        case = stack.pair(k)
        a_k, b_k = cc.energies(case)
        s = cc.window_stats(case)
        flat = s["flat_a"] | s["flat_b"]
        a = s["a"] - s["a"].mean(axis=(1, 2))[:, None, None]
        cnt = np.maximum(s["iz"].sum(axis=(1, 2)), 1)
        mb = np.where(s["iz"], s["bz"], 0.0).sum(axis=(1, 2)) / cnt
        b = np.where(s["inside"], s["b"] - mb[:, None, None], 0.0)
        ea.append(a_k)
        eb.append(b_k)
        bound.append(np.where(flat, 0.0, np.abs(b).max(axis=(1, 2)) * np.abs(a).sum(axis=(1, 2))))
    return np.stack(ea), np.stack(eb), np.stack(bound)


def assert_exact_stack(stack: Stack):
    """The condition that makes every f32 sum of the ensemble kernel exact in any order."""
    for k in range(stack.n_pairs):
        cc.assert_exact(stack.pair(k))
    ea, eb, bound = stack_energies(stack)
    for what, v in (("ea", ea), ("eb", eb), ("max |b| sum |a|", bound)):
        total = v.sum(axis=0).max()
        assert total < cc.LIMIT, f"{stack.name}: the sum of {what} over the pairs reaches {total}"
    return ea.sum(axis=0).max(), eb.sum(axis=0).max(), bound.sum(axis=0).max()


@functools.lru_cache(maxsize=None)
def exact_model(name: str):
    """correlate_ensemble_model on the named exact stack: (vectors [n, 4], flags [n], count [n], planes [n, nS, nS]), read-only."""
    s = exact_stacks()[name]
    v, f, c, p = pe.correlate_ensemble_model(s.im1, s.im2, s.win, s.step, s.R, offset=s.offset, planes=True)
    out = (v.reshape(-1, 4), f.ravel(), c.ravel(), p.reshape(f.size, 2 * s.R + 1, 2 * s.R + 1))
    for x in out:
        x.setflags(write=False)
    return out


# ---- particle stacks ------------------------------------------------------------------------------------------------------
def particle_stack(shape, shift, n_pairs, seed, per_px=0.015, noise=0.02):
    """N pairs of one uniform shift, fresh particles and noise per pair: (im1, im2) f32 [N, height, width]."""
    rng = np.random.default_rng(seed)
    h, w = shape
    a, b = [], []
    for _ in range(n_pairs):
        n = int(per_px * h * w)
        x, y = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n)
        amp = rng.uniform(0.5, 1.0, n)
        a.append(pc.particle_image(shape, x, y, 2.5, amp) + noise * rng.random(shape))
        b.append(pc.particle_image(shape, x + shift[0], y + shift[1], 2.5, amp) + noise * rng.random(shape))
    return np.stack(a).astype(np.float32), np.stack(b).astype(np.float32)


# (win, R, step, (height, width), shift, with offsets): three of test_piv_correlation_gpu.CASES, one per win
PARTICLE_STACKS = [
    (16, 4, 16, (64, 100), (2.3, 1.6), True),
    (32, 16, 12, (150, 131), (7.4, -5.9), False),
    (64, 32, 64, (140, 200), (-12.3, 17.8), False),
]
PARTICLE_PAIRS = 8


# ---- the sparse stack -----------------------------------------------------------------------------------------------------
SPARSE_SHAPE, SPARSE_SHIFT, SPARSE_WIN, SPARSE_STEP, SPARSE_R, SPARSE_PAIRS, SPARSE_DENSITY = (96, 112), (2.3, -1.6), 32, 16, 6, 16, 0.002


@functools.lru_cache(maxsize=None)
def sparse_stack(seed: int):
    """16 pairs at 0.002 particles per pixel, shift (2.3, -1.6) px: (im1, im2) f32 [16, 96, 112], read-only."""
    rng = np.random.default_rng(seed)
    h, w = SPARSE_SHAPE
    a, b = [], []
    for _ in range(SPARSE_PAIRS):
        n = rng.poisson(SPARSE_DENSITY * (h + 16) * (w + 16))
        x, y, amp = rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n), rng.uniform(0.5, 1.0, n)
        a.append((pc.particle_image(SPARSE_SHAPE, x, y, 2.5, amp) + 0.05 * rng.random(SPARSE_SHAPE)).astype(np.float32))
        b.append((pc.particle_image(SPARSE_SHAPE, x + SPARSE_SHIFT[0], y + SPARSE_SHIFT[1], 2.5, amp)
                  + 0.05 * rng.random(SPARSE_SHAPE)).astype(np.float32))
    a, b = np.stack(a), np.stack(b)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def valid(vectors, shift=SPARSE_SHIFT, within: float = 0.5):
    """The vectors within `within` px of the true shift, bool [n_rows, n_cols] (a NaN vector is not)."""
    v = np.asarray(vectors, np.float64)
    with np.errstate(invalid="ignore"):
        return np.hypot(v[..., 0] - shift[0], v[..., 1] - shift[1]) < within


@functools.lru_cache(maxsize=None)
def sparse_model(seed: int):
    """(valid [n_rows, n_cols] of the ensemble, [valid of pair k alone]) from the f64 models, computed once per seed."""
    a, b = sparse_stack(seed)
    v, _, _ = pe.correlate_ensemble_model(a, b, SPARSE_WIN, SPARSE_STEP, SPARSE_R)
    single = [valid(pc.correlate_model(a[k], b[k], SPARSE_WIN, SPARSE_STEP, SPARSE_R)[0]) for k in range(SPARSE_PAIRS)]
    return valid(v), single, v
