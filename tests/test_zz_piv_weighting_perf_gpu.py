"""The weighted direct correlator against section 5's kernel at 1024^2 (runs late, with the other timing bounds): the
weight costs one load and one multiply per staged pixel, under 1 % of the tile loop's multiply-adds at these radii, so the
weighted call may take section 5's time plus twice what section 5 differs from itself in the same run."""
import ctypes

import numpy as np
import pytest

import test_piv_correlation_gpu as base
from photon_amd import piv_weighting as pw

pytestmark = pytest.mark.gpu

SIZES = [(32, 16, 8), (64, 32, 16)]         # win, step, R
WARMUP, REPS = 2, 5


@pytest.mark.parametrize("win,step,R", SIZES, ids=[f"w{w}_s{s}_r{r}" for w, s, r in SIZES])
def test_the_weighted_correlator_costs_what_section_5_costs(photon, win, step, R):
    """Per round: section 5, the weighted call, section 5 again (the A/A pair), each timed with device events; medians of
    five rounds after two warm-up rounds.  weighted <= section 5 (1 + 2 |A/A difference|).

    Measured on one MI355X: win 32 / R 8 section 5 106.7 us, again 107.0 us (A/A 0.34 %), weighted 105.4 us (-1.2 %);
    win 64 / R 16 204.0 us, 204.6 us (0.33 %), 197.6 us (-3.1 %).  The weighted kernel's staging loops ask for the loads
    of four trips together; with section 5's trip-by-trip staging it was 1.6 to 2.6 % slower and missed this bound
    (DESIGN.md section 4.3q)."""
    import torch
    im1, im2 = base.particle_pair((1024, 1024), (3.3, -2.7), seed=5)
    a, b = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    table = torch.from_numpy(pw.window_weights(win)).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_rows = n_cols = (1024 - win) // step + 1
    vec = torch.empty((n_rows, n_cols, 4), dtype=torch.float32, device="cuda")      # outputs allocated once: the events bracket
    flg = torch.empty((n_rows, n_cols), dtype=torch.int32, device="cuda")           # one launch and nothing else
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    L = photon.lib

    def plain():
        return L.photon_piv_correlate(p(a), p(b), 1024, 1024, win, step, R, None, p(vec), p(flg), None, None, None, stream)

    def weighted():
        return L.photon_piv_correlate_weighted(p(a), p(b), p(table), 1024, 1024, win, step, R, None, p(vec), p(flg), None, None, None, stream)

    def timed(run):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        rc = run()
        stop.record()
        stop.synchronize()
        assert rc == 0
        return start.elapsed_time(stop) * 1e3           # microseconds

    times = {"a": [], "w": [], "a2": []}
    for k in range(WARMUP + REPS):
        for name, run in (("a", plain), ("w", weighted), ("a2", plain)):
            us = timed(run)
            if k >= WARMUP:
                times[name].append(us)
    assert np.isfinite(vec.cpu().numpy()).any()
    t_a, t_w, t_a2 = (float(np.median(times[k])) for k in ("a", "w", "a2"))
    spread = abs(t_a2 - t_a) / t_a
    print(f"win {win}, step {step}, R {R} at 1024^2: section 5 {t_a:.1f} us, again {t_a2:.1f} us (A/A {100 * spread:.2f} %), "
          f"weighted {t_w:.1f} us ({100 * (t_w / t_a - 1):+.2f} %)")
    assert t_w <= t_a * (1.0 + 2.0 * spread), (t_w, t_a, t_a2)
