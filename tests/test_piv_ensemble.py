"""Ensemble correlation on the host (photon_amd/piv_ensemble.py; include/parallel_ray_tracing.h, section 14): the f64 model
against correlate_model and against a plain sum of raw planes, the exactness condition of the exact stacks, and what the
feature is for -- a field from pairs too sparse to give one each."""
import numpy as np
import pytest

import piv_ensemble_cases as cs
import piv_tail_cases
from photon_amd import piv_correlation as pc
from photon_amd import piv_ensemble as pe


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("with_off", [False, True], ids=["no offsets", "offsets"])
def test_one_pair_is_correlate_model(with_off):
    """N = 1: every value of the model equals correlate_model's, flat windows (NaN) and windows off the image included."""
    im1, im2, _, off = piv_tail_cases.nine_windows()
    off = off if with_off else None
    want = pc.correlate_model(im1, im2, 16, 16, 4, offset=off, planes=True)
    v, f, c, p = pe.correlate_ensemble_model(im1[None], im2[None], 16, 16, 4, offset=off, planes=True)
    assert same(v, want[0]) and np.array_equal(f, want[1]) and same(p, want[2])
    flat = (want[1] & pc.FLAG_FLAT) != 0
    assert flat.any() and not flat.all()
    assert np.array_equal(c, np.where(flat, 0, 1))
    assert len(pe.correlate_ensemble_model(im1[None], im2[None], 16, 16, 4)) == 3


def plain_sum(s1, s2, win, step, R, offset=None):
    """The definition, written as a plain loop over pairs and windows."""
    parts = [pc.raw_planes(a, b, win, step, R, offset) for a, b in zip(s1, s2)]
    n = len(parts[0][1])
    C, Ea, Eb, count = np.zeros_like(parts[0][0]), np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    for Ck, ea, eb, *_ in parts:
        for w in range(n):
            if ea[w] != 0.0 and eb[w] != 0.0:
                C[w] += Ck[w]
                Ea[w] += ea[w]
                Eb[w] += eb[w]
                count[w] += 1
    _, _, _, ox, oy, outside, grid = parts[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = 1.0 / np.sqrt(Ea * Eb)
    v, f, p = pc.peak_outputs(C, R, ox, oy, norm, count == 0, outside, grid, True)
    return v, f, count.reshape(grid), p


def test_many_pairs_are_the_sum_of_raw_planes_in_any_order_and_a_flat_pair_only_counts():
    s1, s2 = cs.particle_stack((70, 90), (1.4, -0.8), 5, seed=3)
    s1[2, :16, :32] = 0.25                      # pair 2 is flat in windows (0, 0) and (0, 1): a constant
    s2[4, 16:48, 40:72] = 0.5                   # pair 4 in the windows of b inside that square
    off = np.random.default_rng(2).integers(-2, 3, size=pc.grid_shape((70, 90), 16, 8) + (2,)).astype(np.int32)
    for offset in (None, off):
        got = pe.correlate_ensemble_model(s1, s2, 16, 8, 4, offset=offset, planes=True)
        want = plain_sum(s1, s2, 16, 8, 4, offset)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[2].min() < 5 and got[2].max() == 5 and got[2].min() >= 3
        np.testing.assert_allclose(got[3], want[3], rtol=0, atol=1e-14)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-12, atol=1e-12)
        # the pair order matters to rounding only
        order = [3, 0, 4, 2, 1]
        other = pe.correlate_ensemble_model(s1[order], s2[order], 16, 8, 4, offset=offset, planes=True)
        assert np.array_equal(other[1], got[1]) and np.array_equal(other[2], got[2])
        np.testing.assert_allclose(other[3], got[3], rtol=0, atol=1e-14)
        np.testing.assert_allclose(other[0][..., :2], got[0][..., :2], rtol=0, atol=1e-9)
    # a pair that is flat in every window contributes nowhere: every output, the count included, stays
    flat1, flat2 = np.concatenate([s1, np.full_like(s1[:1], 0.3)]), np.concatenate([s2, s2[:1]])
    more = pe.correlate_ensemble_model(flat1, flat2, 16, 8, 4, planes=True)
    base = pe.correlate_ensemble_model(s1, s2, 16, 8, 4, planes=True)
    for x, y in zip(more, base):
        assert same(x, y)
    # and in front of the others as well: the sums start from the first pair that contributes
    front = pe.correlate_ensemble_model(flat1[[5, 0, 1, 2, 3, 4]], flat2[[5, 0, 1, 2, 3, 4]], 16, 8, 4, planes=True)
    for x, y in zip(front, base):
        assert same(x, y)


def test_a_time_series_is_its_consecutive_pairs():
    s1, s2 = cs.particle_stack((48, 64), (0.6, 0.3), 4, seed=8)
    frames = np.concatenate([s1, s2[-1:]])
    a, b = pe.pair_stacks(frames)
    assert np.array_equal(a, frames[:-1]) and np.array_equal(b, frames[1:])
    got = pe.correlate_ensemble_model(*pe.pair_stacks(frames), 16, 16, 3)
    want = pe.correlate_ensemble_model(frames[:-1], frames[1:], 16, 16, 3)
    for x, y in zip(got, want):
        assert same(x, y)
    for bad in (frames[0], frames[:1]):
        with pytest.raises(ValueError):
            pe.pair_stacks(bad)
    with pytest.raises(ValueError):
        pe.pair_stacks(s1, s2[:3])


@pytest.mark.parametrize("name", list(cs.exact_stacks()))
def test_exact_stacks_keep_every_f32_sum_exact(name):
    """Each pair passes assert_exact, and the sums over the pairs of ea, eb and max |b| sum |a| stay below 2^24: every partial
    sum of the device, in any order, is an integer an f32 holds."""
    s = cs.exact_stacks()[name]
    assert s.n_pairs >= 5 and s.step == s.win
    ea, eb, bound = cs.assert_exact_stack(s)
    print(f"{name}: {s.n_pairs} pairs, largest sums ea {ea:.0f}, eb {eb:.0f}, max |b| sum |a| {bound:.0f} of {cs.cc.LIMIT}")
    v, f, c, p = cs.exact_model(name)
    assert c.max() == s.n_pairs and 0 < c.min() < s.n_pairs             # the flat pair is missing from some windows
    assert not (f & pc.FLAG_FLAT).any()
    # the model's C is the integer the device must reach: planes * sqrt(Ea Eb) are integers
    Ea, Eb, _ = cs.stack_energies(s)
    C = p * np.sqrt(Ea.sum(axis=0) * Eb.sum(axis=0))[:, None, None]
    assert np.abs(C - np.rint(C)).max() < 1e-6


def test_the_exact_stacks_cover_what_the_issue_asks():
    stacks = cs.exact_stacks().values()
    assert {s.win for s in stacks} == {16, 32, 64}
    assert any(s.R == s.win // 2 for s in stacks) and any(s.offset is not None and s.offset.any() for s in stacks)


@pytest.mark.parametrize("seed", [1, 2])
def test_sparse_pairs_give_a_field_only_together(seed):
    """16 pairs at 0.002 particles per pixel: the ensemble has every vector within 0.5 px of the truth, no single pair has."""
    ok, single, v = cs.sparse_model(seed)
    err = np.hypot(v[..., 0] - cs.SPARSE_SHIFT[0], v[..., 1] - cs.SPARSE_SHIFT[1])
    counts = [int(s.sum()) for s in single]
    print(f"seed {seed}: ensemble {int(ok.sum())} of {ok.size} within 0.5 px (largest error {err.max():.3f} px); "
          f"single pairs {min(counts)} to {max(counts)} of {ok.size}: {counts}")
    assert ok.all()
    assert all(not s.all() for s in single)
