"""A synthetic PIV pair at the size of the reference's sample PIV case (tests/golden/abi_piv_full: 50 000 particles x 10 000
rays, Mie scattering, photon's sample camera), both frames generated and traced on the device.  Frame 1 is the
photon_sources_piv field; frame 2 is the same particles moved through a Lamb-Oseen vortex whose peak image displacement is
about --peak-px pixels (photon_sources_piv_advected).  Both are traced with per-source moments (Scene.trace_moments), and
each particle's centroid shift is held against the paraxial prediction -m(Z) (dX, dY) / pixel_pitch from its world
displacement.  Prints ms per frame, the advection's ms, the particles seen in both frames and the median / 99th percentile
of |measured - predicted| in pixels, then one JSON line.  --tiff DIR writes both frames through the post-process
(postprocess_image) and the TIFF writer; --bench-advect also times 1e6 particles x 16 steps through a 128^3 field.
Run it on a GPU box under a time limit of its own:

    timeout -k 10 600 python tools/piv_pair.py [--tiff DIR] [--bench-advect]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)
from conftest import load_fixture_call  # noqa: E402
from photon_amd import piv_pairs as pp  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402
from photon_amd.ray_tracing import postprocess_image, write_tiff_u16  # noqa: E402

# the sample frame's particle field (run_simulation_02.py:949-965 with the sample parameters): 1.5 x the field of view
BOX_MIN, BOX_MAX = (-7.5e4, -7.5e4, -7.5e3), (7.5e4, 7.5e4, 7.5e3)
BEAM_FWHM, IRRADIANCE = 730.0, 500.0


def timed(fn, reps=3):
    out, best = None, 1e9
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--peak-px", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--tiff", default=None)
    ap.add_argument("--bench-advect", action="store_true")
    args = ap.parse_args()
    lib = PhotonLibrary()
    lib.set_device(0)
    call = load_fixture_call("piv_full")
    n, rays = call.num_sources, call.lightray_number_per_particle
    cam = call.camera
    pitch = float(cam["pixel_pitch"])
    z_object = float(call.z_offset) + float(call.object_distance)
    s_i, s_o = float(call.image_distance), float(call.object_distance)
    # vortex about the axis: peak world speed (t = 1) = peak_px pixels on the sensor at the magnification of the object plane
    rc = 2.0e4
    peak_world = args.peak_px * pitch * s_o / s_i
    gamma = peak_world / pp.lamb_oseen_peak_speed(1.0, rc)
    grid = pp.lamb_oseen_vortex(gamma, rc, (0.0, 0.0), (-8.0e4, -8.0e4, -8.0e3), (8.0e4, 8.0e4, 8.0e3), (129, 129, 3))
    flow = lib.flow_from_grid(*grid)

    f1, w1 = lib.sources_piv_advected(args.seed, n, BOX_MIN, BOX_MAX, z_object, BEAM_FWHM, IRRADIANCE, return_world=True)

    def advect():
        return lib.sources_piv_advected(args.seed, n, BOX_MIN, BOX_MAX, z_object, BEAM_FWHM, IRRADIANCE, flow=flow, t=1.0,
                                        steps=args.steps, return_world=True)
    for _ in range(2):                                  # warm, and free what the timing loop does not keep
        advect()[0].free()
    (f2, w2), advect_ms = timed(advect, 1)

    h, w = call.image_shape
    records, images, frame_ms = [], [], []
    for src in (f1, f2):
        scene = lib.scene_create_from_sources(call, src)
        img = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, 8), dtype=torch.float64, device="cuda")

        def trace():
            img.zero_()
            scene.trace_moments(img.data_ptr(), rec.data_ptr())
        _, ms = timed(trace)
        frame_ms.append(ms)
        records.append(rec.cpu().numpy())
        images.append(img.cpu().numpy().reshape(h, w))
        scene.free()
        src.free()
    flow.free()

    d = pp.image_displacements(records[0], records[1], cam, rays)
    both = ~np.isnan(d).any(axis=1)
    # a particle whose image the sensor's edge clips differently in the two frames has its centroid pulled: the comparison
    # takes the particles with as many rays arriving in frame 2 as in frame 1
    whole = both & (records[0][:, 0] == records[1][:, 0])
    m = s_i / (s_o + w1[:, 2])
    predicted = -m[:, None] * (w2[:, :2] - w1[:, :2]) / pitch
    err = np.hypot(*(d[whole] - predicted[whole]).T)
    shift = np.hypot(*predicted[whole].T)
    print(f"frame 1 {frame_ms[0]:.2f} ms, frame 2 {frame_ms[1]:.2f} ms ({n} particles x {rays} rays, trace with moments)")
    print(f"advection {advect_ms:.3f} ms ({n} particles, {args.steps} RK4 steps, 129 x 129 x 3 field)")
    print(f"particles seen in both frames: {int(both.sum())} of {n}, {int(whole.sum())} of them with equal ray counts; "
          f"predicted image shift up to {shift.max():.2f} px")
    print(f"|measured - predicted| shift (equal counts): median {np.median(err):.4f} px, "
          f"99th percentile {np.percentile(err, 99):.4f} px")
    row = {"particles": n, "rays_per_particle": rays, "frame_ms": [round(v, 2) for v in frame_ms],
           "advect_ms": round(advect_ms, 3), "seen_in_both": int(both.sum()), "equal_counts": int(whole.sum()),
           "max_predicted_px": round(float(shift.max()), 3),
           "median_err_px": float(np.median(err)), "p99_err_px": float(np.percentile(err, 99))}
    if args.tiff:
        os.makedirs(args.tiff, exist_ok=True)
        for k, img in enumerate(images):
            u16 = postprocess_image(img, cam["pixel_gain"], cam["pixel_bit_depth"])
            write_tiff_u16(os.path.join(args.tiff, f"piv_frame{k + 1}.tif"), u16)
        row["tiff"] = args.tiff
    if args.bench_advect:                               # the one number DESIGN records
        big = pp.lamb_oseen_vortex(gamma, rc, (0.0, 0.0), (-8.0e4, -8.0e4, -8.0e3), (8.0e4, 8.0e4, 8.0e3), 128)
        bflow = lib.flow_from_grid(*big)

        def bench():
            lib.sources_piv_advected(args.seed, 1_000_000, BOX_MIN, BOX_MAX, z_object, BEAM_FWHM, IRRADIANCE, flow=bflow,
                                     t=1.0, steps=16).free()
        bench()
        _, row["advect_1e6_16steps_128cubed_ms"] = timed(bench, 5)
        bflow.free()
        print(f"advection of 1e6 particles, 16 steps, 128^3 field: {row['advect_1e6_16steps_128cubed_ms']:.3f} ms")
    print(json.dumps(row), flush=True)
    if not math.isfinite(row["p99_err_px"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
