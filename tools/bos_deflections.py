"""Dot shifts of the sample BOS pair at full size (tests/golden/abi_bos_full_im{1,2}: 120 000 sources x 500 rays per image)
through PhotonLibrary.render_moments -- no ray dumps -- and what the moments cost: the wall time per image of
start_ray_tracing against photon_start_ray_tracing_moments (best of --reps, the two calls alternating), for both sample
images and for C3 (1e7 rays through a 256^3 volume).  Prints the reference's summary lines (light_ray_processing.py:623-624)
and one JSON line per case.  Run it on a GPU box under a time limit of its own:

    timeout -k 10 600 python tools/bos_deflections.py [--reps 5] [--skip-c3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: one HIP runtime per process)
from conftest import load_fixture_call  # noqa: E402
from photon_amd import deflections as dfl  # noqa: E402
from photon_amd import scenes  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402


def timed(fn, reps):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def cost(lib, name, call, reps):
    lib.render(call)
    lib.render_moments(call)                                # warm: volume cache, block cache, moments block
    plain = moments = 1e9
    for _ in range(reps):                                   # alternate, so drift hits both alike
        plain = min(plain, timed(lambda: lib.render(call), 1))
        moments = min(moments, timed(lambda: lib.render_moments(call), 1))
    row = {"case": name, "rays": call.num_rays, "sources": call.num_sources, "start_ray_tracing_ms": round(plain, 2),
           "moments_ms": round(moments, 2), "overhead_ms": round(moments - plain, 2)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-c3", action="store_true")
    args = ap.parse_args()
    lib = PhotonLibrary()
    lib.set_device(0)
    recs = []
    for im in ("im1", "im2"):
        call = load_fixture_call(f"bos_full_{im}")
        cost(lib, f"bos_full_{im}", call, args.reps)
        recs.append(lib.render_moments(call)[1])
    rps = call.lightray_number_per_particle
    d = dfl.dot_deflections(recs[0], recs[1], call.camera, rps)
    whole = ~(np.isnan(d.d_pos).any(axis=1))
    print(dfl.summary(d))
    print(json.dumps({"dots": int(whole.size), "whole_in_both": int(whole.sum()),
                      "max_abs_d_pos_px": float(np.abs(d.d_pos[whole]).max()) if whole.any() else None,
                      "median_rms_spot_px": float(np.nanmedian(d.rms1))}))
    if not args.skip_c3:
        with tempfile.TemporaryDirectory() as tmp:
            cost(lib, "C3", scenes.config("C3", tmp), args.reps)


if __name__ == "__main__":
    main()
