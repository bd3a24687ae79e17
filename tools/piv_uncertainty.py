#!/usr/bin/env python3
"""photon_piv_uncertainty on the GPU: what it costs, how well sigma is calibrated, what it does to the BOS integral.

    python tools/piv_uncertainty.py [--size 2048] [--skip-timing] [--skip-calibration] [--skip-bos] [--out result.json]

1. Timing.  The kernel at win 16 / 32 / 64 (step win / 2) with reach 0 / 2 / 4 on a size^2 pair, and photon_piv_correlate with
   radius 4 on the same pair and grid, all in the same alternating windows of about a quarter of a second (device events after
   a warm-up; median, smallest and largest; the shader clock read while they run: tools/bos_tomography.py).  Reported with
   the ratio uncertainty (reach 2) / correlate (radius 4) of the medians per window size.
2. Calibration.  The "uniform" and "vortex" pairs of tests/piv_deformation_cases.py (seeds 1-4, 256^2, win 32, step 16)
   with Gaussian image noise 0.02, 0.05, 0.10: PhotonLibrary.correlate_deform (3 iterations), then
   PhotonLibrary.displacement_uncertainty (reach 2); over the interior nodes, the mean error removed per seed and component:
   rms sigma / std(error) and the share of |error| <= sigma (68 % for a calibrated Gaussian error).
3. BOS.  The rendered blob of DESIGN.md section 4.3c through bos_density.reconstruct with weights="median" and with
   weights="uncertainty": both errors against the chief-ray truth, and the share of nodes whose error lies within
   bos_density.projected_density_uncertainty (and within twice it).  No bound is set on either.
One JSON object on stdout."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)
import bos_density_cases as bc  # noqa: E402
import bos_tomography as bt  # noqa: E402
import piv_deformation_cases as dc  # noqa: E402
import piv_uncertainty_cases as uc  # noqa: E402
from photon_amd import bos_density as bd  # noqa: E402
from photon_amd import piv_correlation as pc  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

WINS, REACHES, RADIUS = (16, 32, 64), (0, 2, 4), 4


def timing(lib, size: int) -> dict:
    f, rng = uc.frame((size, size)), np.random.default_rng(8)
    a, b = (bt.dev((f + rng.normal(0.0, uc.NOISE, f.shape)).astype(np.float32)) for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    fns, keep = {}, []
    for win in WINS:
        step = win // 2
        r, c = pc.grid_shape((size, size), win, step)
        sigma = torch.empty((r, c, 2), dtype=torch.float32, device="cuda")
        vec = torch.empty((r, c, 4), dtype=torch.float32, device="cuda")
        flags = torch.empty((r, c), dtype=torch.int32, device="cuda")
        keep += [sigma, vec, flags]
        vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def unc(win=win, step=step, reach=0, sigma=sigma, flags=flags):
            lib._call("photon_piv_uncertainty", vp(a), vp(b), size, size, win, step, reach, vp(sigma), vp(flags), None, None, None,
                      ctypes.c_void_p(stream))

        def cor(win=win, step=step, vec=vec, flags=flags):
            lib._call("photon_piv_correlate", vp(a), vp(b), size, size, win, step, RADIUS, None, vp(vec), vp(flags), None, None, None,
                      ctypes.c_void_p(stream))
        for reach in REACHES:
            fns[f"uncertainty_win{win}_reach{reach}"] = (lambda u=unc, k=reach: u(reach=k))
        fns[f"correlate_win{win}_radius{RADIUS}"] = cor
    clock = bt.ClockSampler(lib)
    clock.start()
    t = bt.timed(fns)
    clock_read = clock.stop()
    out = dict(image=f"{size} x {size}", step="win / 2", shader_clock_under_load=clock_read, ms={k: bt.spread(v) for k, v in t.items()},
               windows={w: int(np.prod(pc.grid_shape((size, size), w, w // 2))) for w in WINS})
    out["uncertainty_reach2_over_correlate_radius4"] = {
        w: round(t[f"uncertainty_win{w}_reach2"]["median"] / t[f"correlate_win{w}_radius{RADIUS}"]["median"], 3) for w in WINS}
    return out


def calibration_table(lib, reach: int = 2) -> list:
    rows = []
    for kind in ("uniform", "vortex"):
        for noise in (0.02, 0.05, 0.10):
            errors, sigmas, bad = [], [], 0
            for seed in uc.CAL_SEEDS:
                im1, im2 = uc.noisy_pair(kind, seed, noise)
                vec, _ = lib.correlate_deform(im1, im2, dc.WIN, dc.STEP, iterations=3)
                sigma, flags = lib.displacement_uncertainty(im1, im2, vec, dc.WIN, dc.STEP, reach=reach)
                bad += int((flags[1:-1, 1:-1] != 0).sum())
                errors.append(uc.interior_error(vec, kind))
                sigmas.append(sigma[1:-1, 1:-1].reshape(-1, 2).astype(np.float64))
            ratio, cover = uc.calibration(errors, sigmas)
            e, s = np.concatenate(errors), np.concatenate(sigmas)
            rows.append(dict(pair=kind, image_noise=noise, nodes=int(e.shape[0]), flagged=bad,
                             std_error_px=[round(float(v), 4) for v in e.std(axis=0)],
                             rms_sigma_px=[round(float(v), 4) for v in np.sqrt((s * s).mean(axis=0))],
                             rms_sigma_over_std_error=[round(float(v), 3) for v in ratio],
                             share_within_sigma=[round(float(v), 3) for v in cover]))
    return rows


def bos_study(lib, reach: int = 2) -> dict:
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        c1, c2 = bc.blob_calls(lib, wd, False)
        im1, im2 = (lib.render(c).reshape(bc.N_PIX, bc.N_PIX).astype(np.float32) for c in (c1, c2))
    P, mid, h = bc.truth(c2)
    shape = (bc.N_PIX, bc.N_PIX)
    vectors, flags = lib.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    sigma, sflags = lib.displacement_uncertainty(im1, im2, vectors, bc.WIN, bc.STEP, reach=reach)
    sgx, sgy = bd.gradient_uncertainty(sigma, c2.camera, bd.displacement_factor(c2, bc.ORIGIN_Z, bc.EXTENT))
    out["sigma_px"] = dict(median=[round(float(v), 4) for v in np.nanmedian(sigma, axis=(0, 1))], flagged=int((sflags != 0).sum()))
    for weights in ("median", "uncertainty"):
        phi, _, st = bd.integrate_vectors(lib, vectors, flags, shape, c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, weights, sigma=sigma)
        w = bd.measured_gradients(vectors, flags, shape, c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, weights, sigma=sigma)[2]
        rel, off, holes = bc.errors(phi, P, mid, h)
        sphi = bd.projected_density_uncertainty(sgx, sgy, w, None, h, h)
        use = np.isfinite(phi) & np.isfinite(sphi) & (sphi > 0)
        err = np.abs(phi - P)[use]
        out[weights] = dict(rel_l2_error=round(rel, 4), nan_share=round(holes, 4), iterations=st["iterations"],
                            weight_range=[round(float(w[w > 0].min()), 3), round(float(w.max()), 3)], nodes=int(use.sum()),
                            median_sigma_phi_over_peak=round(float(np.median(sphi[use]) / P.max()), 5),
                            rms_error_over_peak=round(float(np.sqrt((err * err).mean()) / P.max()), 5),
                            share_within_sigma_phi=round(float((err <= sphi[use]).mean()), 3),
                            share_within_two_sigma_phi=round(float((err <= 2 * sphi[use]).mean()), 3))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-calibration", action="store_true")
    ap.add_argument("--skip-bos", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    lib = PhotonLibrary()
    lib.set_device(0)
    result = dict(library=lib.version())
    if not args.skip_timing:
        result["timing"] = timing(lib, args.size)
    if not args.skip_calibration:
        result["calibration"] = calibration_table(lib)
    if not args.skip_bos:
        result["bos"] = bos_study(lib)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
