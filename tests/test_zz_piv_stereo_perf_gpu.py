"""One dewarp launch of two 1024^2 frames against two photon_piv_deform calls on the same frames (runs late, with the other
timing bounds).  The warp is the yardstick: the dewarp evaluates two f64 cubics per pixel where the warp interpolates a grid
field, and shares coordinate, weights and mirrored indices between the two frames where two warps compute them twice."""
import ctypes

import numpy as np
import pytest

import test_piv_correlation_gpu as base
from photon_amd import library

pytestmark = pytest.mark.gpu

WARMUP, REPS = 2, 7
BOUND = 1.5


def test_one_dewarp_of_two_frames_costs_no_more_than_one_and_a_half_times_two_warps(photon):
    """Per round: the two warps, the dewarp, the two warps again, each timed with device events; medians of seven rounds after
    two warm-up rounds.  dewarp <= 1.5 x two warps.  Measured on one MI355X: two warps 30.3 us, again 30.3 us, one dewarp 13.2 us (ratio 0.44;
    DESIGN.md section 4.3w)."""
    import torch
    n = 1024
    im1, im2 = base.particle_pair((n, n), (3.3, -2.7), seed=5)
    frames = torch.from_numpy(np.stack([im1, im2])).cuda()
    coef, out = torch.empty_like(frames), torch.empty_like(frames)
    for k in range(2):
        photon.bspline_coefficients(frames[k].data_ptr(), n, n, coef[k].data_ptr())
    mask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    win, step = 32, 16
    rows = cols = (n - win) // step + 1
    rng = np.random.default_rng(3)
    field = torch.from_numpy(rng.uniform(-4.0, 4.0, (rows, cols, 2)).astype(np.float32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    # a camera like the suite's 30 degree views: magnification 0.87 along x, a few pixels of curvature, everything inside
    job = library.photon_piv_dewarp_t(d_coef=coef.data_ptr(), frame_stride=n * n, n_frames=2, width=n, height=n, out_width=n, out_height=n,
                                      out_stride=n * n, d_out=out.data_ptr(), d_mask=mask.data_ptr(), stream=stream)
    x = (60.0, 0.87, 0.004, 1.5e-5, -4e-6, 2e-6, 1e-9, -2e-9, 1e-9, 5e-10)
    y = (8.0, -0.003, 0.97, 3e-6, 1e-5, -2e-6, -1e-9, 1e-9, 2e-9, -5e-10)
    for k in range(10):
        job.poly[0][k], job.poly[1][k] = x[k], y[k]
    job.grid[0], job.grid[1], job.grid[2], job.grid[3] = 0.0, 1.0, 0.0, 1.0
    L, p = photon.lib, lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def warps():
        rc = 0
        for k, scale in ((0, -0.5), (1, 0.5)):
            rc |= L.photon_piv_deform(p(coef[k]), n, n, p(field), 2, rows, cols, win, step, scale, p(out[k]), ctypes.c_void_p(stream))
        return rc

    def dewarp():
        return L.photon_piv_dewarp(ctypes.byref(job))

    def timed(run):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        rc = run()
        stop.record()
        stop.synchronize()
        assert rc == 0
        return start.elapsed_time(stop) * 1e3           # microseconds

    times = {"a": [], "d": [], "a2": []}
    for k in range(WARMUP + REPS):
        for name, run in (("a", warps), ("d", dewarp), ("a2", warps)):
            us = timed(run)
            if k >= WARMUP:
                times[name].append(us)
    assert not mask.cpu().numpy().any() and np.isfinite(out.cpu().numpy()).all()
    t_a, t_d, t_a2 = (float(np.median(times[k])) for k in ("a", "d", "a2"))
    print(f"two 1024^2 frames: two warps {t_a:.1f} us, again {t_a2:.1f} us, one dewarp {t_d:.1f} us (ratio {t_d / t_a:.3f})")
    assert t_d <= BOUND * t_a, (t_d, t_a, t_a2)
