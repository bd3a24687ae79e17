"""Dot tracking on the device (include/parallel_ray_tracing.h section 8; PhotonLibrary.track_dots).  Prints JSON lines:

1. the rendered blob scene of tests/bos_density_cases.py at 512^2, both splats: the per-dot error table against
   dot_tracking.true_dots (device and f64 model; without a predictor and from PhotonLibrary.correlation_predictor), the
   window-grid comparison with correlate(passes=2) against window_truth, and the relative L2 error of the projected
   density from the true shifts, the two-pass correlation, and the tracked field with and without the predictor;
2. the sample BOS pair at full size (tests/golden/abi_bos_full_im{1,2}, as tools/bos_deflections.py renders it): dots
   found and paired, and the per-source error against the moments' truth;
3. the analytic chain pairs of tests/dot_tracking_cases.py (per-dot error table, device);
4. time at 1024^2 (analytic pair, 0.005 dots per pixel): every entry point by device events around 20 back-to-back
   calls, and track_dots with a grid against correlate_deform(iterations=3) by wall clock (median of 12).

Kernel-level times come from a separate run under rocprofv3 --kernel-trace --stats.  Run it on a GPU box under a time limit:

    timeout -k 10 600 python tools/bos_dot_tracking.py [--skip-sample] [--skip-blob]
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
import torch  # noqa: E402  (first: one HIP runtime per process)
import bos_density_cases as bc  # noqa: E402
import dot_tracking_cases as cs  # noqa: E402
from photon_amd import bos_density as bd  # noqa: E402
from photon_amd import dot_tracking as dt  # noqa: E402
from photon_amd import piv_correlation as pc  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

DOT_PX = 5.4                # e^-2 diameter of the blob scene's dots on the sensor


def rounded(d: dict, digits: int = 4) -> dict:
    return {k: (round(v, digits) if isinstance(v, float) else v) for k, v in d.items()}


def blob(lib, diffraction: bool):
    n = bc.N_PIX
    with tempfile.TemporaryDirectory() as wd:
        c1, call = bc.blob_calls(lib, wd, diffraction)
        im1, r1 = lib.render_moments(c1)
        im2, r2 = lib.render_moments(call)
    im1, im2 = (im.reshape(n, n).astype(np.float32) for im in (im1, im2))
    truth = dt.true_dots(r1, r2, call.camera, call.lightray_number_per_particle, group=bc.DOT_POINTS)
    p = truth["pos1"]
    with np.errstate(invalid="ignore"):
        inside = (p[:, 0] > 4) & (p[:, 0] < n - 5) & (p[:, 1] > 4) & (p[:, 1] < n - 5)
    kw = dict(sigma_w=DOT_PX / 4, grid=(bc.WIN, bc.STEP, 3, 0), **cs.CHAIN)
    name = "erf" if diffraction else "4-pixel"
    want, _ = pc.window_truth(p, truth["shift"], (n, n), bc.WIN, bc.STEP, 3)
    P, mid, h = bc.truth(call)
    geometry = ((n, n), call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)

    def density(vectors, flags, weights="median"):
        phi, _, st = bd.integrate_vectors(lib, vectors, flags, *geometry, weights=weights)
        rel, off, holes = bc.errors(phi, P, mid, h)
        return dict(rel_l2_error=rel, nan_share=holes, argmax_offset_steps=[round(off[0], 2), round(off[1], 2)], converged=st["converged"])

    def window_error(vectors):
        return float(np.nanmedian(np.linalg.norm(np.asarray(vectors, np.float64)[..., :2] - want, axis=-1)))

    pred = lib.correlation_predictor(im1, im2, bc.WIN, bc.STEP)
    for label, predictor in (("no predictor", None), ("correlation predictor", (pred, bc.WIN, bc.STEP))):
        res = lib.track_dots(im1, im2, predictor=predictor, **kw)
        model = dt.track_dots_model(im1, im2, predictor=None if predictor is None else (pred.cpu().numpy(), bc.WIN, bc.STEP), **kw)
        same = (res["pair"] == model["pair"]) & (res["pair"] >= 0)
        print(json.dumps(dict(measurement="blob_per_dot", splat=name, route=label, detected=[res["count1"], res["count2"]], pairs=res["npaired"],
                              status_bit_2=int((res["status1"] & 2 != 0).sum()), device=rounded(dt.score(res, p, truth["shift"], inside)),
                              model=rounded(dt.score(model, p, truth["shift"], inside)), paired_alike=int(same.sum()),
                              worst_device_minus_model_px=float(np.abs(res["shift"][same].astype(np.float64) - model["shift"][same]).max()),
                              window_median_error_px=round(window_error(res["vectors"]), 4),
                              density=rounded(density(res["vectors"], res["flags"])))), flush=True)
    vectors, flags = lib.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    print(json.dumps(dict(measurement="blob_references", splat=name, window_median_error_px_two_pass=round(window_error(vectors), 4),
                          density_two_pass=rounded(density(vectors, flags)),
                          density_true_shifts=rounded(density(want, np.where(np.isfinite(want[..., 0]), 0, 2), "unit")))), flush=True)


def sample_pair(lib):
    from conftest import load_fixture_call
    recs, ims = [], []
    for im in ("im1", "im2"):
        call = load_fixture_call(f"bos_full_{im}")
        image, rec = lib.render_moments(call)
        cam = call.camera
        ims.append(image.reshape(int(cam["y_pixel_number"]), int(cam["x_pixel_number"])).astype(np.float32))
        recs.append(rec)
    truth = dt.true_dots(recs[0], recs[1], call.camera, call.lightray_number_per_particle)
    t0 = time.perf_counter()
    res = lib.track_dots(ims[0], ims[1], 0.25, relative=True, sigma_w=1.0, radius=3.0)
    ms = 1e3 * (time.perf_counter() - t0)
    d = res["shift"][res["pair"] >= 0, 2:]
    print(json.dumps(dict(measurement="sample_pair", sensor=list(ims[0].shape), sources=int(truth["pos1"].shape[0]),
                          detected=[res["count1"], res["count2"]], pairs=res["npaired"], first_call_ms=round(ms, 2),
                          median_diameter_px=float(np.nanmedian(res["dots1"][:, 3])),
                          dx_range_px=[float(d[:, 0].min()), float(d[:, 0].max())] if d.size else None,
                          dy_range_px=[float(d[:, 1].min()), float(d[:, 1].max())] if d.size else None,
                          per_source=rounded(dt.score(res, truth["pos1"], truth["shift"])))), flush=True)


def analytic(lib):
    for name, diameter, im1, im2, pos, shifts in cs.chain_pairs():
        res = lib.track_dots(im1, im2, sigma_w=diameter / 4, **cs.CHAIN)
        print(json.dumps(dict(measurement="analytic_per_dot", pair=name, detected=[res["count1"], res["count2"]], pairs=res["npaired"],
                              **rounded(dt.score(res, pos, shifts)))), flush=True)


def events_ms(fn, calls: int = 20) -> float:
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def timing(lib, n: int = 1024):
    im1, im2, _, _ = cs.analytic_pair(1, 0.005, 4.0, n_pix=n)
    a, b = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    cap = dt.default_max_dots((n, n))
    nb = max(lib.dots_scratch_bytes(n, n), lib.dots_scratch_bytes(n, n, 3.0, cap, cap))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ints = torch.zeros((2, cap + 1), dtype=torch.int32, device="cuda")
    dots = torch.empty((2, cap, 4), device="cuda")
    status = torch.empty((2, cap), dtype=torch.int32, device="cuda")
    top = torch.empty(2, device="cuda")
    pair = torch.empty(cap + 1, dtype=torch.int32, device="cuda")
    shift = torch.empty((cap, 4), device="cuda")
    r, c = pc.grid_shape((n, n), 32, 16)
    vectors, flags = torch.empty((r, c, 4), device="cuda"), torch.empty((r, c), dtype=torch.int32, device="cuda")
    count = [ints[f, cap:].data_ptr() for f in (0, 1)]
    steps = {
        "image_max": lambda: lib.dots_image_max(a.data_ptr(), n, n, top[0].data_ptr()),
        "detect": lambda: lib.dots_detect(a.data_ptr(), n, n, 0.25, top[0].data_ptr(), cap, ints[0].data_ptr(), count[0], scratch.data_ptr(), nb),
        "fit": lambda: lib.dots_fit(a.data_ptr(), n, n, ints[0].data_ptr(), count[0], cap, 3, 1.0, 4, 0.0, dots[0].data_ptr(), status[0].data_ptr()),
        "match": lambda: lib.dots_match(dots[0].data_ptr(), status[0].data_ptr(), count[0], cap, dots[1].data_ptr(), status[1].data_ptr(), count[1],
                                        cap, 3.0, n, n, pair.data_ptr(), shift.data_ptr(), pair[cap:].data_ptr(), scratch.data_ptr(), nb),
        "window_means": lambda: lib.dots_window_means(dots[0].data_ptr(), pair.data_ptr(), shift.data_ptr(), count[0], cap, n, n, 32, 16, 3, 0,
                                                      vectors.data_ptr(), flags.data_ptr()),
    }
    # frame 2 once, so that match has both
    lib.dots_image_max(b.data_ptr(), n, n, top[1].data_ptr())
    lib.dots_detect(b.data_ptr(), n, n, 0.25, top[1].data_ptr(), cap, ints[1].data_ptr(), count[1], scratch.data_ptr(), nb)
    lib.dots_fit(b.data_ptr(), n, n, ints[1].data_ptr(), count[1], cap, 3, 1.0, 4, 0.0, dots[1].data_ptr(), status[1].data_ptr())
    out = {name: round(1e3 * events_ms(fn), 2) for name, fn in steps.items()}                       # microseconds per call
    calls = {"track_dots": lambda: lib.track_dots(a, b, sigma_w=1.0, grid=(32, 16, 3, 0), **cs.CHAIN),
             "correlate_deform_3": lambda: lib.correlate_deform(a, b, 32, 16, 16, iterations=3)}
    wall = {k: [] for k in calls}
    for rep in range(3 + 12):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:
                wall[name].append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(measurement="time", sensor=f"{n}x{n}", dots=[int(ints[0, cap]), int(ints[1, cap])], capacity=cap, us_per_call=out,
                          image_bytes=4 * n * n, wall_ms_median_of_12={k: round(float(np.median(v)), 3) for k, v in wall.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--skip-blob", action="store_true")
    a = ap.parse_args()
    lib = PhotonLibrary(build=False)
    lib.set_device(0)
    if not a.skip_blob:
        for diffraction in (False, True):
            blob(lib, diffraction)
    if not a.skip_sample:
        sample_pair(lib)
    analytic(lib)
    timing(lib)


if __name__ == "__main__":
    main()
