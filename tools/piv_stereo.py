#!/usr/bin/env python3
"""Stereo PIV (section 19) on one GPU: kernel and driver times, the accuracy table of the three synthetic pairs for the device
chain and the model chain, and the kernels' static resources -- the figures of DESIGN.md section 4.3w.

    python tools/piv_stereo.py [--size 1024] [--reps 20] [--no-model]
    python tools/piv_stereo.py --self-calibrate [--no-model]

--self-calibrate: the self-calibration of photon_amd.piv_stereo.SELFCAL_CASE instead (section 19c) -- the table of the rounds
with the device times of the two dewarps, the ensemble correlation and the triangulation per round, the accuracy of the three
components before and after on the case's pair, and the triangulation's time against the reconstruction's on 512 x 512 nodes.

Times are device events around `reps` back-to-back calls (one wait at the end), after a warm-up; the driver is timed on the
host around whole calls.  The accuracy pairs are photon_amd.piv_stereo.CASES (192 x 160 plane at 0.2 mm/px, sensors 224 x 256,
cameras at 300 mm and +-30 degrees, or 35 / -20 degrees with +5 / -3 degrees of elevation; win 32, step 16, radius 8)."""
import argparse
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
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def self_calibrate(lib, with_model):
    import torch
    from photon_amd import piv_stereo as ps
    case = ps.SELFCAL_CASE
    pl, grid, settings = case["plane"], case["disparity"], dict(case["evaluation"])
    views, frames, pair, aligned = ps.selfcal_inputs()
    cams = tuple(v[1] for v in views)
    true = ps.sheet_frame(case["sheet"], pl)
    target = ps.calibration_target(pl, 9, (-0.5, 0.0, 0.5))

    def off_by(cameras):
        return max(float(np.linalg.norm(ps.map_points(c, target) - v[0].project(ps.to_world(true, target)), axis=-1).max()) for c, v in zip(cameras, views))
    d = [torch.from_numpy(f).cuda() for f in frames]
    lib.self_calibrate_stereo(d[0], d[1], cams, pl, **grid)                                 # warm-up
    timings = []
    t0 = time.perf_counter()
    corrected, report = lib.self_calibrate_stereo(d[0], d[1], cams, pl, timings=timings, **grid)
    ms = (time.perf_counter() - t0) * 1e3
    chains = [("device", corrected, report)]
    if with_model:
        chains.append(("model", *ps.self_calibrate_model(frames[0], frames[1], cams, pl, **grid)))
    print(f"sheet {case['sheet']}, {case['n_frames']} frames per camera, win {grid['win']} step {grid['step']} radius {grid['radius']}; cameras off by "
          f"{off_by(cams):.2f} px before")
    print("chain  round  disparity rms [px]  sheet a [mm]      b         c      sheet rms [mm]  nodes  error median [px]  refit max [px]"
          "   dewarps  correlation  triangulation [ms]")
    for chain, _, rep in chains:
        for k, e in enumerate(rep["rounds"]):
            took = f"{timings[k]['dewarp']:8.3f}  {timings[k]['correlate']:8.3f}  {timings[k]['triangulate']:8.3f}" if chain == "device" else ""
            print(f"{chain:6s} {k + 1:3d}    {e['disparity_rms']:10.4f}        {e['sheet'][0]:9.5f} {e['sheet'][1]:9.6f} {e['sheet'][2]:9.6f}    "
                  f"{e['sheet_rms']:8.5f}     {e['nodes']:4d}     {e['error_median']:8.4f}         {max(r[1] for r in e['refit']):8.1e}     {took}")
    for chain, cameras, rep in chains:
        print(f"{chain}: sheet in the calibration's world {np.round(rep['sheet'], 5)}, cameras off by {off_by(cameras):.4f} px after"
              + (f"; the driver took {ms:.1f} ms with the timing waits" if chain == "device" else ""))
    print("chain   cameras       sheet      rms dX     dY     dZ [px]   residual median [px]")
    rows = [("device", "original", "displaced", lambda: lib.correlate_stereo(*pair, cams, pl, settings=settings)[0], None),
            ("device", "corrected", "displaced", lambda: lib.correlate_stereo(*pair, corrected, pl, settings=settings)[0], report),
            ("device", "original", "aligned", lambda: lib.correlate_stereo(*aligned, cams, pl, settings=settings)[0], None)]
    if with_model:
        args = tuple(settings[k] for k in ("win", "step", "radius", "iterations"))
        rows += [("model", "original", "displaced", lambda: ps.correlate_stereo_model(*pair, cams, pl, *args)[0], None),
                 ("model", "corrected", "displaced", lambda: ps.correlate_stereo_model(*pair, chains[1][1], pl, *args)[0], chains[1][2]),
                 ("model", "original", "aligned", lambda: ps.correlate_stereo_model(*aligned, cams, pl, *args)[0], None)]
    for chain, which, sheet, run, rep in rows:
        rms, median = ps.selfcal_figures(run(), None if rep is None else (rep["R"], rep["O"], rep["C"]))
        print(f"{chain:7s} {which:13s} {sheet:10s} {rms[0]:6.4f} {rms[1]:6.4f} {rms[2]:6.4f}       {median:6.4f}")

    n, win, step = 512, 32, 16
    side = (n - 1) * step + win
    big = ps.centred_plane(side, side, 30.0 / side)
    rng = np.random.default_rng(5)
    f = [torch.from_numpy(rng.uniform(-0.5, 0.5, (n, n, 4)).astype(np.float32) / np.float32(big["pitch"])).cuda() for _ in range(2)]
    s = [torch.from_numpy(rng.uniform(0.02, 0.2, (n, n, 2)).astype(np.float32)).cuda() for _ in range(2)]
    t_rec = device_us(lambda: lib.piv_stereo_reconstruct(f[0].data_ptr(), f[1].data_ptr(), 4, cams, big, win, step, 0, 0, s[0].data_ptr(),
                                                         s[1].data_ptr()), 20)
    line = f"{n} x {n} nodes (size query and allocation included): photon_piv_stereo_reconstruct with sigmas {t_rec:.1f} us; photon_piv_stereo_triangulate"
    for iterations in (1, 4, 16):
        t_tri = device_us(lambda: lib.piv_stereo_triangulate(f[0].data_ptr(), 4, cams, big, win, step, iterations), 20)
        line += f", {iterations} iterations {t_tri:.1f} us"
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--self-calibrate", action="store_true", help="the self-calibration of SELFCAL_CASE instead of the stereo tables")
    ap.add_argument("--size", type=int, default=1024, help="side of the frames the dewarp and the warp are timed on")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the host model chain (the accuracy table's second half)")
    args = ap.parse_args()
    import torch
    from photon_amd import piv_stereo as ps
    from photon_amd.library import PhotonLibrary
    lib = PhotonLibrary()
    if args.self_calibrate:
        self_calibrate(lib, not args.no_model)
        return
    n, rng = args.size, np.random.default_rng(1)

    # ---- kernels
    frames = torch.from_numpy(rng.uniform(0.0, 1.0, (2, n, n)).astype(np.float32)).cuda()
    coef, out = torch.empty((2, n, n), dtype=torch.float32, device="cuda"), torch.empty((2, n, n), dtype=torch.float32, device="cuda")
    mask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    for k in range(2):
        lib.bspline_coefficients(frames[k].data_ptr(), n, n, coef[k].data_ptr())
    pl = ps.centred_plane(n, n, 0.2)
    view = ps.pinhole(np.deg2rad(30.0), 0.0, 300.0 * n / 192, 5.0, (n + 64, n + 64))
    target = ps.calibration_target(pl)
    cam, _, worst = ps.fit_camera(target, view.project(target))
    poly, grid = ps.plane_coefficients(cam, pl)
    print(f"{n} x {n}: camera fitted to {worst:.1e} px, {100 * ps.outside_mask(poly, grid, (n, n), (n, n)).mean():.1f} % of the plane outside")
    win, step = 32, 16
    rows = cols = (n - win) // step + 1
    field = torch.from_numpy(rng.uniform(-4.0, 4.0, (rows, cols, 2)).astype(np.float32)).cuda()
    t_dewarp = device_us(lambda: lib.piv_dewarp(coef.data_ptr(), n * n, 2, n, n, poly, grid, n, n, n * n, out.data_ptr(), mask.data_ptr()), args.reps)
    t_one = device_us(lambda: lib.piv_dewarp(coef.data_ptr(), n * n, 1, n, n, poly, grid, n, n, n * n, out.data_ptr(), mask.data_ptr()), args.reps)

    def warps():
        for k, scale in ((0, -0.5), (1, 0.5)):
            lib.piv_deform(coef[k].data_ptr(), n, n, field.data_ptr(), 2, rows, cols, win, step, scale, out[k].data_ptr())
    t_warps = device_us(warps, args.reps)
    print(f"photon_piv_dewarp, two frames: {t_dewarp:.1f} us; one frame: {t_one:.1f} us; two photon_piv_deform: {t_warps:.1f} us "
          f"(dewarp / two warps {t_dewarp / t_warps:.3f})")
    cams = tuple(c[1] for c in ps.calibrated_pair("symmetric"))
    f = [torch.from_numpy(rng.uniform(-3.0, 3.0, (rows, cols, 4)).astype(np.float32)).cuda() for _ in range(2)]
    s = [torch.from_numpy(rng.uniform(0.02, 0.2, (rows, cols, 2)).astype(np.float32)).cuda() for _ in range(2)]
    t_rec = device_us(lambda: lib.piv_stereo_reconstruct(f[0].data_ptr(), f[1].data_ptr(), 4, cams, pl, win, step, 0, 0, s[0].data_ptr(),
                                                         s[1].data_ptr()), args.reps)
    print(f"photon_piv_stereo_reconstruct, {rows} x {cols} nodes with sigmas (size query and allocation included): {t_rec:.1f} us")

    # ---- driver and accuracy
    settings = dict(ps.CASE_GRID)
    print("case        chain   rms dX     dY     dZ [px]  cam 1 alone  ratio   residual median / max [px]   driver [ms]")
    for name in ps.CASES:
        f1, f2, cams = ps.case_pair(name)
        d1, d2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
        lib.correlate_stereo(d1, d2, cams, ps.CASE_PLANE, settings=settings)
        t0 = time.perf_counter()
        for _ in range(5):
            result = lib.correlate_stereo(d1, d2, cams, ps.CASE_PLANE, settings=settings)
        ms = (time.perf_counter() - t0) / 5 * 1e3
        chains = [("device", result, f"{ms:8.2f}")]
        if not args.no_model:
            chains.append(("model", ps.correlate_stereo_model(f1, f2, cams, ps.CASE_PLANE, *(settings[k] for k in ("win", "step", "radius", "iterations"))), ""))
        for chain, (res, _, (v1, _)), took in chains:
            rms, alone, median, worst = ps.case_figures(name, res, v1)
            print(f"{name:11s} {chain:7s} {rms[0]:6.4f} {rms[1]:6.4f} {rms[2]:6.4f}      {alone:6.3f}     {rms[0] / alone:5.3f}    {median:6.4f} / {worst:6.4f}"
                  f"          {took}")

    # ---- static resources
    for unit, match in (("photon_piv_stereo", "kernel"), ("photon_piv_deform", "deform_kernel")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_report.py"), "--unit", unit, "--match", match], capture_output=True,
                           text=True)
        print(r.stdout.strip() or r.stderr.strip()[-500:])


if __name__ == "__main__":
    main()
