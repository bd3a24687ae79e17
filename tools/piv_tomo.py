#!/usr/bin/env python3
"""Tomographic PIV (section 20) on one GPU: kernel times against their yardsticks, the quality Q of both line-of-sight modes,
the accuracy table of the synthetic cases for the device chain and the model chain, and the kernels' static resources -- the
figures of DESIGN.md section 4.3x.

    python tools/piv_tomo.py [--reps 10] [--no-model]
    python tools/piv_tomo.py --mart [--reps 10] [--no-model]      MART (section 21): the figures of DESIGN.md section 4.3y

Times are device events around `reps` back-to-back calls (one wait at the end), after a warm-up; the driver is timed on the
host around whole calls.  The accuracy cases are photon_amd.piv_tomo.CASES (volume 64 x 64 x 24 voxels at 0.1 mm, sensors 96 x
96 at 10 px/mm, three or four pinhole cameras at 300 mm, 0.08 particles per pixel; win 16, step 8, radius 3, win_z 16, step_z
4, radius_z 3)."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_us(run, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def mart(lib, args):
    """--mart: the figures of DESIGN.md section 4.3y.  Times on section 4.3x's line-of-sight shape from the MinLOS volume of a
    rendered pair: the whole call with 1 and with 2 iterations (each behind a copy that restores the first guess; the copy
    alone is subtracted), so that one fused camera step is a quarter of their difference.  Then per case of
    photon_amd.piv_mart.CASES at seed 0: Q of the first exposure on the whole volume and on the interior for MinLOS and after
    every iteration, and the vector rms of the MART chain next to MinLOS's."""
    import torch
    from photon_amd import piv_mart as pm
    from photon_amd import piv_tomo as pt
    vol = pt.centred_volume(256, 256, 32, 0.1)
    views = pt.calibrated_views(pt.CASES["uniform"]["angles"], vol, shape=(512, 512), px_per_mm=15.0)
    cams = [v[1] for v in views]
    frames, _ = pt.particle_volume_pair([v[0] for v in views], pt.uniform_flow, vol, 7, shape=(512, 512), ppp=0.05)
    poly, grids = pt.los_coefficients(cams, vol)
    first, unseen = lib.reconstruct_volume(list(frames), cams, vol)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    d_poly = torch.from_numpy(poly).cuda()
    d_vol = first.clone()
    acc = torch.empty((2, 2, 512 * 512), dtype=torch.int64, device="cuda")
    s, thr = pm.scale_log2_for(list(frames)), pm.default_threshold(list(frames))

    def run(iterations):
        d_vol.copy_(first)
        if iterations:
            lib.piv_volume_mart([f.data_ptr() for f in d_frames], [512 * 512] * 4, 2, [(512, 512)] * 4, grids, d_poly.data_ptr(), vol, 32 * 256 * 256,
                                d_vol.data_ptr(), acc.data_ptr(), iterations, 1, thr, s, unseen.data_ptr())
    t0, t1, t2, t5 = (device_us(lambda k=k: run(k), args.reps) for k in (0, 1, 2, 5))
    live = [float((first > 0).float().mean().item())]
    run(5)
    live.append(float((d_vol > 0).float().mean().item()))
    print(f"{lib.version()}")
    print(f"MART, 4 cameras 512^2, volume 256 x 256 x 32, 2 frames, live voxels {live[0]:.3f} of the first guess, {live[1]:.3f} after 5 iterations:")
    print(f"  1 iteration {t1 - t0:.0f} us, 2 iterations {t2 - t0:.0f} us, 5 iterations {t5 - t0:.0f} us; one camera step {(t2 - t1) / 4:.1f} us "
          f"(the copy that restores the first guess, subtracted: {t0:.0f} us)")

    print("case            Q MinLOS (interior)   Q after iteration 1 .. 5, whole volume / interior                 chain    rms dX     dY     dZ [voxels]")
    for name in pm.CASES:
        frames, cameras, vol, (P, brightness, half) = pm.case_inputs(name, 0)
        truth = pt.true_volume(vol, P - half, brightness)
        los = lib.reconstruct_volume(list(frames), cameras, vol)[0][0].cpu().numpy()
        qs = []
        for k in range(1, 6):
            E = lib.reconstruct_volume(list(frames), cameras, vol, method="mart", iterations=k)[0][0].cpu().numpy()
            qs.append(f"{pt.quality(E, truth):.3f}/{pm.interior_quality(E, truth):.3f}")
        chains = [("MinLOS", lib.correlate_tomo(list(frames), cameras, vol, **pt.CASE_GRID)),
                  ("MART", lib.correlate_tomo(list(frames), cameras, vol, reconstruction="mart", **pt.CASE_GRID))]
        if not args.no_model:
            chains.append(("model", pm.mart_tomo_model(frames, cameras, vol, **pt.CASE_GRID)))
        for chain, res in chains:
            rms, _ = pm.case_figures(name, res[0])
            head = f"{name:15s} {pt.quality(los, truth):.3f} ({pm.interior_quality(los, truth):.3f})         {' '.join(qs)}" if chain == "MinLOS" else " " * 96
            print(f"{head:96s}   {chain:7s} {rms[0]:6.4f} {rms[1]:6.4f} {rms[2]:6.4f}")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_report.py"), "--unit", "photon_piv_mart", "--match", "kernel"],
                       capture_output=True, text=True)
    print(r.stdout.strip() or r.stderr.strip()[-500:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-model", action="store_true", help="skip the host model chain (the accuracy table's second half)")
    ap.add_argument("--mart", action="store_true", help="the MART figures (section 21, DESIGN.md section 4.3y) instead of section 20's")
    args = ap.parse_args()
    import torch
    from photon_amd import library
    from photon_amd import piv_tomo as pt
    lib = library.PhotonLibrary()
    if args.mart:
        return mart(lib, args)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    # ---- the 3-D correlator against the ensemble correlator on as many plane pairs
    n = 512
    torch.manual_seed(3)
    vols, frames = torch.rand((2, 16, n, n), device="cuda"), torch.rand((2, 144, n, n), device="cuda")
    rows = (n - 32) // 16 + 1
    vec4, flg = torch.empty((rows, rows, 4), device="cuda"), torch.empty((rows, rows), dtype=torch.int32, device="cuda")
    print("3-D correlator, volume 512 x 512 x 16, win 32, step 16, win_z 16, one slab of 31 x 31 windows")
    print("   R  R_z  plane pairs   volume [us]   ensemble of as many pairs [us]   ratio")
    for R, Rz in ((8, 4), (8, 0), (4, 2), (16, 4)):
        pairs = 16 * (2 * Rz + 1)
        vec5 = torch.empty((1, rows, rows, 5), device="cuda")
        pln = torch.empty((rows, rows, 2 * Rz + 1, 2 * R + 1, 2 * R + 1), device="cuda")
        job = library.photon_piv_correlate_volume_t(d_vol1=vols[0].data_ptr(), d_vol2=vols[1].data_ptr(), nx=n, ny=n, nz=16, win=32, step=16,
                                                    radius=R, win_z=16, step_z=16, radius_z=Rz, d_vectors=vec5.data_ptr(), d_flags=flg.data_ptr(),
                                                    d_planes=pln.data_ptr(), stream=None)
        t_v = device_us(lambda: lib.lib.photon_piv_correlate_volume(ctypes.byref(job)), args.reps)
        t_e = device_us(lambda: lib.lib.photon_piv_correlate_ensemble(p(frames[0]), p(frames[1]), n * n, pairs, n, n, 32, 16, R, None, p(vec4), p(flg),
                                                                     None, None, None, None, None), args.reps)
        print(f"  {R:2d}  {Rz:2d}     {pairs:4d}       {t_v:9.0f}        {t_e:9.0f}                     {t_v / t_e:5.3f}")
    del vols, frames

    # ---- the line-of-sight kernel against the dewarp launches that give the same samples
    vol = pt.centred_volume(256, 256, 32, 0.1)
    cams = [v[1] for v in pt.calibrated_views(pt.CASES["uniform"]["angles"], vol, shape=(512, 512), px_per_mm=15.0)]
    poly, grids = pt.los_coefficients(cams, vol)
    coefs = [torch.rand((2, 512, 512), device="cuda") for _ in range(4)]
    d_poly = library._on_device(poly, torch.float64, "cuda", "poly")
    out, unseen = torch.empty((2, 32, 256, 256), device="cuda"), torch.empty((32, 256, 256), dtype=torch.uint8, device="cuda")
    planes, masks = torch.empty((4, 32, 2, 256, 256), device="cuda"), torch.empty((4, 32, 256, 256), dtype=torch.uint8, device="cuda")

    def los(mode, n_frames=2):
        lib.piv_volume_los([c.data_ptr() for c in coefs], [512 * 512] * 4, n_frames, [(512, 512)] * 4, grids, d_poly.data_ptr(), vol, 32 * 256 * 256,
                           out.data_ptr(), unseen.data_ptr(), mode)

    def dewarps():
        for c in range(4):
            for k in range(32):
                lib.piv_dewarp(coefs[c].data_ptr(), 512 * 512, 2, 512, 512, poly[c][k], grids[c], 256, 256, 256 * 256, planes[c, k].data_ptr(),
                               masks[c, k].data_ptr())
    t_min, t_prod, t_one, t_dw = (device_us(f, args.reps) for f in (lambda: los(0), lambda: los(1), lambda: los(0, 1), dewarps))
    print(f"line of sight, 4 cameras 512^2, volume 256 x 256 x 32: two frames minimum {t_min:.0f} us, product {t_prod:.0f} us; one frame {t_one:.0f} us; "
          f"the 128 dewarp launches of two frames {t_dw:.0f} us (ratio {t_min / t_dw:.3f})")

    # ---- quality, driver and accuracy
    print("case        Q min    Q product   chain   rms dX     dY     dZ [voxels]   interior nodes   driver [ms]")
    for name in pt.CASES:
        frames, cameras, vol, (P, brightness, half) = pt.case_inputs(name, 0)
        truth = pt.true_volume(vol, P - half, brightness)
        q = {mode: pt.quality(lib.reconstruct_volume(list(frames), cameras, vol, mode=mode)[0][0].cpu().numpy(), truth) for mode in pt.MODES}
        d = [torch.from_numpy(f).cuda() for f in frames]
        lib.correlate_tomo(d, cameras, vol, **pt.CASE_GRID)
        t0 = time.perf_counter()
        for _ in range(5):
            result = lib.correlate_tomo(d, cameras, vol, **pt.CASE_GRID)
        ms = (time.perf_counter() - t0) / 5 * 1e3
        chains = [("device", result, f"{ms:8.2f}")]
        if not args.no_model:
            chains.append(("model", pt.correlate_tomo_model(frames, cameras, vol, **pt.CASE_GRID), ""))
        for chain, res, took in chains:
            rms, count = pt.case_figures(name, res[0])
            print(f"{name:11s} {q['min']:6.3f}   {q['product']:6.3f}      {chain:7s} {rms[0]:6.4f} {rms[1]:6.4f} {rms[2]:6.4f}          {count:3d}          {took}")

    # ---- static resources
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_report.py"), "--unit", "photon_piv_tomo", "--match", "kernel"],
                       capture_output=True, text=True)
    print(r.stdout.strip() or r.stderr.strip()[-500:])


if __name__ == "__main__":
    main()
