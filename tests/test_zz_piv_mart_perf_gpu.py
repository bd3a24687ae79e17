"""One MART iteration against one line-of-sight launch on the same cameras and volume (runs late, with the other timing
bounds).  Device events around the calls alone, the two alternating; medians of five rounds after two warm-up rounds."""
import numpy as np
import pytest

from photon_amd import piv_mart as pm
from photon_amd import piv_tomo as pt

pytestmark = pytest.mark.gpu

WARMUP, REPS = 2, 5
RECORDED_RATIO = 1.155          # one MART iteration / one line-of-sight launch, measured on one MI355X


def timed(run):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3           # microseconds


def test_one_mart_iteration_against_one_los_launch(photon):
    """Section 4.3x's line-of-sight shape: 4 cameras, 512^2 sensors, volume 256 x 256 x 32, 2 frames; the first guess is MinLOS
    of a rendered pair (0.05 particles per pixel), so the volume has the zeros a particle volume has: the time scales with
    the live voxels.  Timed: photon_piv_volume_mart with iterations = 1 -- the projection of the first guess and the four
    fused camera steps -- from the first guess each time.  Yardstick: one photon_piv_volume_los launch on the same
    cameras, frames and volume.  Bound: the recorded ratio x 1.5 (boxes differ by several per cent in clock, and the rate
    of 64-bit integer atomic adds was measured on one box only).

    Measured on one MI355X: 0.845 of the first guess at 0; one iteration 293 us, one line-of-sight launch 254 us, again 259 us:
    ratio 1.155."""
    import torch
    vol = pt.centred_volume(256, 256, 32, 0.1)
    views = pt.calibrated_views(pt.CASES["uniform"]["angles"], vol, shape=(512, 512), px_per_mm=15.0)
    cameras = [v[1] for v in views]
    frames, _ = pt.particle_volume_pair([v[0] for v in views], pt.uniform_flow, vol, 7, shape=(512, 512), ppp=0.05)
    poly, grids = pt.los_coefficients(cameras, vol)
    first, mask = photon.reconstruct_volume(list(frames), cameras, vol)
    zero_fraction = float((first == 0).float().mean().item())
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    coefs = [torch.empty_like(f) for f in d_frames]
    for f, c in zip(d_frames, coefs):
        for k in range(2):
            photon.bspline_coefficients(f[k].data_ptr(), 512, 512, c[k].data_ptr())
    d_poly = torch.from_numpy(poly).cuda()
    d_vol, out = first.clone(), torch.empty_like(first)
    out_mask = torch.empty_like(mask)
    acc = torch.empty((2, 2, 512 * 512), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    s, thr = pm.scale_log2_for(list(frames)), pm.default_threshold(list(frames))
    nvox = 32 * 256 * 256

    def mart():
        photon.piv_volume_mart([f.data_ptr() for f in d_frames], [512 * 512] * 4, 2, [(512, 512)] * 4, grids, d_poly.data_ptr(), vol, nvox,
                               d_vol.data_ptr(), acc.data_ptr(), 1, 1, thr, s, mask.data_ptr(), stream)

    def los():
        photon.piv_volume_los([c.data_ptr() for c in coefs], [512 * 512] * 4, 2, [(512, 512)] * 4, grids, d_poly.data_ptr(), vol, nvox, out.data_ptr(),
                              out_mask.data_ptr(), 0, stream)
    times = {"mart": [], "los": [], "los_again": []}
    for k in range(WARMUP + REPS):
        for name, run in (("los", los), ("mart", mart), ("los_again", los)):
            d_vol.copy_(first)
            us = timed(run)
            if k >= WARMUP:
                times[name].append(us)
    t = {name: float(np.median(v)) for name, v in times.items()}
    ratio = t["mart"] / t["los"]
    print(f"MART, 4 cameras 512^2, volume 256 x 256 x 32, 2 frames, {zero_fraction:.3f} of the first guess at 0: one iteration {t['mart']:.0f} us; "
          f"one line-of-sight launch {t['los']:.0f} us, again {t['los_again']:.0f} us; ratio {ratio:.3f}")
    assert torch.equal(out, first) and 0.5 < zero_fraction < 0.99
    after = d_vol.cpu().numpy()
    assert np.isfinite(after).all() and 0 < (after > 0).sum() <= (first > 0).sum().item()
    assert ratio <= 1.5 * RECORDED_RATIO
