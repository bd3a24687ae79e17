"""Ensemble correlation (sum of correlation) of a stack of image pairs (pure numpy: usable without a GPU).

The device form is photon_piv_correlate_ensemble (include/parallel_ray_tracing.h, section 14;
``PhotonLibrary.piv_correlate_ensemble`` on raw device pointers, ``PhotonLibrary.correlate_ensemble`` on stacks).  Where a
single pair holds too few particles per window for a reliable peak -- steady or periodic flow recorded many times, a static
BOS object, micro-PIV seeding -- the correlation planes of the pairs are summed before the peak is read (Meinhart, Wereley
& Santiago 2000): the true peak adds up in every pair, the random ones do not.

``correlate_ensemble_model`` is the f64 host model: section 5's planes and energies of every pair
(``piv_correlation.raw_planes``), summed over the pairs that contribute, then ``piv_correlation.peak_outputs``.
"""
from __future__ import annotations

import numpy as np

from . import piv_correlation as pc


def pair_stacks(frames1, frames2=None):
    """(stack1, stack2), each [N, height, width]: the two stacks as given, or, with frames2 None, the pairs (f_k, f_k+1) of
    a time series of N + 1 frames."""
    s1 = np.asarray(frames1)
    if frames2 is None:
        if s1.ndim != 3 or s1.shape[0] < 2:
            raise ValueError("a time series must be [N + 1, height, width] with at least two frames")
        return s1[:-1], s1[1:]
    s2 = np.asarray(frames2)
    if s1.ndim != 3 or s1.shape != s2.shape or s1.shape[0] < 1:
        raise ValueError("stack1 and stack2 must be two [N, height, width] arrays of one shape, N >= 1")
    return s1, s2


def correlate_ensemble_model(stack1, stack2, win: int, step: int, radius: int, offset=None, planes: bool = False):
    """Host model of photon_piv_correlate_ensemble in f64.  stack1, stack2: [N, height, width], pair k = (stack1[k],
    stack2[k]); offset: integer (ox, oy) per window as correlate_model takes it, shared by all pairs.  Per window, over the
    pairs that contribute -- those whose window is not flat, an f64 energy of 0, as in correlate_model -- in pair order:
    C = sum C_k, Ea = sum ea_k, Eb = sum eb_k, each sum starting from the first contributing pair's value; then
    peak_outputs on C with 1 / sqrt(Ea Eb).  A window no pair contributes to is flat (flag 2, NaN).
    Returns (vectors [n_rows, n_cols, 4], flags [n_rows, n_cols] int32, count [n_rows, n_cols] int32 -- the contributing
    pairs) and, with planes=True, the normalised planes [n_rows, n_cols, 2R+1, 2R+1] as a fourth item."""
    s1, s2 = pair_stacks(stack1, stack2)
    C = Ea = Eb = None
    for im1, im2 in zip(s1, s2):
        Ck, ea, eb, ox, oy, outside, grid = pc.raw_planes(im1, im2, win, step, radius, offset)
        if C is None:
            C, Ea, Eb = np.zeros_like(Ck), np.zeros_like(ea), np.zeros_like(eb)
            count = np.zeros(ea.shape, np.int32)
        use = (ea != 0.0) & (eb != 0.0)
        first = use & (count == 0)
        more = use & (count > 0)
        C = np.where(first[:, None, None], Ck, np.where(more[:, None, None], C + Ck, C))
        Ea = np.where(first, ea, np.where(more, Ea + ea, Ea))
        Eb = np.where(first, eb, np.where(more, Eb + eb, Eb))
        count = count + use.astype(np.int32)
    flat = count == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(Ea * Eb)
    out = pc.peak_outputs(C, int(radius), ox, oy, norm, flat, outside, grid, planes)
    return out[:2] + (count.reshape(grid),) + out[2:]
