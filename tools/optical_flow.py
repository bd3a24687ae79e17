#!/usr/bin/env python
"""Dense optical flow on the device (include/parallel_ray_tracing.h, section 12): what it costs and what it gains.

    python tools/optical_flow.py [--sizes 512 2048] [--skip-accuracy] [--skip-blob] [--json out.json]

1. Times, per image side: photon_piv_deform_dense, photon_optflow_terms, photon_optflow_iterate at N = 1, T and 8 T sweeps,
   and PhotonLibrary.optical_flow with its defaults from a grid predictor -- device events over alternating windows (the
   windows of tools/bos_tomography.py), the shader clock read beside them.  Then the question the fusion has to answer:
   T sweeps in one launch against T launches of one sweep, for every T the library can be asked for
   (PHOTON_OPTFLOW_SWEEPS), in the same alternating windows.
2. The accuracy table of tests/optical_flow_cases.py from the device: dense predictor error and flow error per field and seed.
3. The projected-density error of the rendered blob of tests/bos_density_cases.py through bos_density.reconstruct_flow next
   to bos_density.reconstruct.
"""
import argparse
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
import optical_flow_cases as oc  # noqa: E402
import piv_deformation_cases as dc  # noqa: E402
from bos_tomography import ClockSampler, spread, timed  # noqa: E402
from photon_amd import bos_density as bd  # noqa: E402
from photon_amd import piv_correlation as pc  # noqa: E402
from photon_amd import piv_deformation as pd  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

MAX_FUSE = 8


def with_sweeps(t, fn):
    """fn() with the library asked for t sweeps per launch (None: its default)."""
    old = os.environ.pop("PHOTON_OPTFLOW_SWEEPS", None)
    if t is not None:
        os.environ["PHOTON_OPTFLOW_SWEEPS"] = str(t)
    try:
        return fn()
    finally:
        os.environ.pop("PHOTON_OPTFLOW_SWEEPS", None)
        if old is not None:
            os.environ["PHOTON_OPTFLOW_SWEEPS"] = old


def timing(lib, n: int) -> dict:
    rng = np.random.default_rng(n)
    im = torch.from_numpy(rng.random((n, n), dtype=np.float32)).cuda()
    im2 = torch.from_numpy(rng.random((n, n), dtype=np.float32)).cuda()
    coef, out = torch.empty_like(im), torch.empty_like(im)
    lib.bspline_coefficients(im.data_ptr(), n, n, coef.data_ptr())
    u = torch.from_numpy(rng.normal(0.0, 1.5, (n, n, 2)).astype(np.float32)).cuda()
    terms = torch.empty((n, n, 4), device="cuda")
    res, tmp = torch.empty_like(u), torch.empty_like(u)
    lib.optflow_terms(im.data_ptr(), im2.data_ptr(), n, n, u.data_ptr(), 3.0, 5.0, terms.data_ptr())
    T = lib.optflow_iterations_per_launch()
    grid = torch.zeros((*pc.grid_shape((n, n), 32, 16), 2), device="cuda")
    bufs = [u, res]

    def sweeps(count):
        def run():                              # ping-pong between two fields: every call reads what the last one wrote
            lib.optflow_iterate(terms.data_ptr(), bufs[0].data_ptr(), n, n, count, bufs[1].data_ptr(), tmp.data_ptr())
            bufs.reverse()
        return run

    fns = {"deform_dense": lambda: lib.piv_deform_dense(coef.data_ptr(), n, n, u.data_ptr(), 0.5, out.data_ptr()),
           "terms": lambda: lib.optflow_terms(im.data_ptr(), im2.data_ptr(), n, n, u.data_ptr(), 3.0, 5.0, terms.data_ptr()),
           "iterate_1": sweeps(1), f"iterate_T={T}": sweeps(T), f"iterate_8T={8 * T}": sweeps(8 * T),
           "driver_3x48": lambda: lib.optical_flow(im, im2, grid)}
    clock = ClockSampler(lib)
    clock.start()
    t = timed(fns)
    # fused against single: 64 sweeps either way, in launches of t (the library asked for t) and in 64 launches of 1
    fuse = {}
    for k in (1, 2, 4, MAX_FUSE):
        fuse[f"64_sweeps_in_launches_of_{k}"] = (lambda k=k: with_sweeps(k, sweeps(64)))
    tf = timed(fuse)
    clock_read = clock.stop()
    single = tf["64_sweeps_in_launches_of_1"]["median"]
    return dict(side=n, T=T, ms={k: spread(v) for k, v in t.items()}, fused_ms={k: spread(v) for k, v in tf.items()},
                us_per_sweep={k: round(1e3 * v["median"] / 64, 3) for k, v in tf.items()},
                fused_over_single={k: round(v["median"] / single, 3) for k, v in tf.items()}, shader_clock_under_load=clock_read)


def accuracy(lib) -> list:
    rows = []
    for kind in oc.KINDS:
        for seed in dc.SEEDS:
            im1, im2 = oc.pair32(kind, seed)
            pred, _ = lib.correlate_deform(im1, im2, dc.WIN, dc.STEP, iterations=1)
            flow = lib.optical_flow(im1, im2, pred[..., :2], dc.WIN, dc.STEP)
            rows.append((kind, seed, oc.flow_rms(pd.dense_field(pred, im1.shape, dc.WIN, dc.STEP), kind), oc.flow_rms(flow, kind)))
    oc.print_table("PhotonLibrary.optical_flow (alpha2 5, 3 warps x 48 sweeps) from one iteration of correlate_deform, 256^2", rows)
    return [dict(field=k, seed=s, predictor_px=round(p, 4), flow_px=round(f, 4)) for k, s, p, f in rows]


def blob(lib) -> dict:
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        for diffraction in (False, True):
            c1, c2 = bc.blob_calls(lib, wd, diffraction)
            im1, im2 = (lib.render(c).reshape(bc.N_PIX, bc.N_PIX).astype(np.float32) for c in (c1, c2))
            P, mid, h = bc.truth(c2)
            args = (lib, im1, im2, c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
            out["erf" if diffraction else "4-pixel"] = dict(
                reconstruct=round(bc.errors(bd.reconstruct(*args, passes=2)[0], P, mid, h)[0], 4),
                reconstruct_flow=round(bc.errors(bd.reconstruct_flow(*args)[0], P, mid, h)[0], 4))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--skip-blob", action="store_true")
    ap.add_argument("--json", help="also write the results to this file")
    args = ap.parse_args()
    lib = PhotonLibrary()
    res = dict(library=lib.version(), timing=[timing(lib, n) for n in args.sizes])
    if not args.skip_accuracy:
        res["accuracy"] = accuracy(lib)
    if not args.skip_blob:
        res["blob_relative_l2_error"] = blob(lib)
    print(json.dumps(res, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
