"""The two kernels of section 20 against parent code that does the same work (runs late, with the other timing bounds): the
3-D correlator against the ensemble correlator on as many plane pairs, the line-of-sight kernel against the dewarp launches
that produce the same samples.  Device events around the launches alone; medians of five rounds after two warm-up rounds."""
import ctypes

import numpy as np
import pytest

from photon_amd import library
from photon_amd import piv_stereo as ps
from photon_amd import piv_tomo as pt

pytestmark = pytest.mark.gpu

WARMUP, REPS = 2, 5


def timed(run):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3           # microseconds


def medians(runs):
    times = {name: [] for name in runs}
    for k in range(WARMUP + REPS):
        for name, run in runs.items():
            us = timed(run)
            if k >= WARMUP:
                times[name].append(us)
    return {name: float(np.median(t)) for name, t in times.items()}


def test_the_volume_correlator_against_the_ensemble_correlator(photon):
    """Volume 512 x 512 x 16, win 32, step 16, R 8, win_z 16, R_z 4: 9 x 16 = 144 plane pairs per window.  Yardstick:
    photon_piv_correlate_ensemble with 144 pairs of 512^2 frames on the same grid -- the same plane-pair count, the same
    staging per pair.  Bound: ratio <= 1.5 (one more read of the window for the means, and the 3-D tail).

    Measured on one MI355X: the volume correlator 3102 us, the ensemble of 144 pairs 3688 us, again 3681 us: ratio 0.841
    (DESIGN.md section 4.3x)."""
    import torch
    torch.manual_seed(3)
    n = 512
    vols = torch.rand((2, 16, n, n), device="cuda")
    frames = torch.rand((2, 144, n, n), device="cuda")
    rows = cols = (n - 32) // 16 + 1
    stream = torch.cuda.current_stream().cuda_stream
    vec5 = torch.empty((1, rows, cols, 5), dtype=torch.float32, device="cuda")
    flg = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
    pln = torch.empty((rows, cols, 9, 17, 17), dtype=torch.float32, device="cuda")
    job = library.photon_piv_correlate_volume_t(d_vol1=vols[0].data_ptr(), d_vol2=vols[1].data_ptr(), nx=n, ny=n, nz=16, win=32, step=16, radius=8,
                                                win_z=16, step_z=16, radius_z=4, d_vectors=vec5.data_ptr(), d_flags=flg.data_ptr(),
                                                d_planes=pln.data_ptr(), stream=stream)
    vec4 = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda")
    flg2 = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    L = photon.lib

    def volume():
        assert L.photon_piv_correlate_volume(ctypes.byref(job)) == 0

    def ensemble():
        assert L.photon_piv_correlate_ensemble(p(frames[0]), p(frames[1]), n * n, 144, n, n, 32, 16, 8, None, p(vec4), p(flg2), None, None, None, None,
                                               ctypes.c_void_p(stream)) == 0
    t = medians({"ensemble": ensemble, "volume": volume, "ensemble_again": ensemble})
    ratio = t["volume"] / t["ensemble"]
    print(f"3-D correlator 512 x 512 x 16, win 32 / R 8 / win_z 16 / R_z 4: {t['volume']:.0f} us; ensemble of 144 pairs {t['ensemble']:.0f} us, "
          f"again {t['ensemble_again']:.0f} us; ratio {ratio:.3f}")
    assert np.isfinite(vec5.cpu().numpy()).all() and np.isfinite(vec4.cpu().numpy()).all()
    assert ratio <= 1.5


def test_the_los_kernel_against_the_dewarp_launches(photon):
    """4 cameras, 512^2 sensors, volume 256 x 256 x 32, 2 frames.  Yardstick: the 4 x 32 photon_piv_dewarp launches that
    produce the same samples.  Bound: ratio <= 1.0 (the same arithmetic, a quarter of the stores, one launch for 128).

    Measured on one MI355X: the line-of-sight launch 259 us, the 128 dewarp launches 1292 us, again 1266 us: ratio 0.200
    (DESIGN.md section 4.3x)."""
    import torch
    torch.manual_seed(4)
    vol = pt.centred_volume(256, 256, 32, 0.1)
    views = pt.calibrated_views(pt.CASES["uniform"]["angles"], vol, shape=(512, 512), px_per_mm=15.0)
    cameras = [v[1] for v in views]
    poly, grids = pt.los_coefficients(cameras, vol)
    assert not any(ps.outside_mask(poly[c][k], grids[c], (256, 256), (512, 512)).any() for c in range(4) for k in (0, 31))
    coefs = [torch.rand((2, 512, 512), device="cuda") for _ in range(4)]
    d_poly = torch.empty((4, 32, 2, 10), dtype=torch.float64, device="cuda")
    d_poly.copy_(library._on_device(poly, torch.float64, "cuda", "poly"))
    out = torch.empty((2, 32, 256, 256), dtype=torch.float32, device="cuda")
    mask = torch.empty((32, 256, 256), dtype=torch.uint8, device="cuda")
    planes = torch.empty((4, 32, 2, 256, 256), dtype=torch.float32, device="cuda")
    masks = torch.empty((4, 32, 256, 256), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def los():
        photon.piv_volume_los([c.data_ptr() for c in coefs], [512 * 512] * 4, 2, [(512, 512)] * 4, grids, d_poly.data_ptr(), vol, 32 * 256 * 256,
                              out.data_ptr(), mask.data_ptr(), 0, stream)

    def dewarps():
        for c in range(4):
            for k in range(32):
                photon.piv_dewarp(coefs[c].data_ptr(), 512 * 512, 2, 512, 512, poly[c][k], grids[c], 256, 256, 256 * 256, planes[c, k].data_ptr(),
                                  masks[c, k].data_ptr(), stream)
    t = medians({"dewarps": dewarps, "los": los, "dewarps_again": dewarps})
    ratio = t["los"] / t["dewarps"]
    print(f"line of sight, 4 cameras 512^2, volume 256 x 256 x 32, 2 frames: {t['los']:.0f} us; 128 dewarp launches {t['dewarps']:.0f} us, "
          f"again {t['dewarps_again']:.0f} us; ratio {ratio:.3f}")
    want = torch.clamp(planes, min=0.0).amin(dim=0).permute(1, 0, 2, 3)             # the same samples: the minimum over the cameras
    assert torch.equal(out, want.contiguous()) and not mask.any().item()
    assert ratio <= 1.0
