"""A synthetic PIV pair at the size of the reference's sample PIV case (tests/golden/abi_piv_full: 50 000 particles x 10 000
rays, Mie scattering, photon's sample camera), both frames generated and traced on the device.  Frame 1 is the
photon_sources_piv field; frame 2 is the same particles moved through a Lamb-Oseen vortex whose peak image displacement is
about --peak-px pixels (photon_sources_piv_advected).  Both are traced with per-source moments (Scene.trace_moments), and
each particle's centroid shift is held against the paraxial prediction -m(Z) (dX, dY) / pixel_pitch from its world
displacement.  Prints ms per frame, the advection's ms, the particles seen in both frames and the median / 99th percentile
of |measured - predicted| in pixels, then one JSON line.  --tiff DIR writes both frames through the post-process
(postprocess_image) and the TIFF writer; --bench-advect also times 1e6 particles x 16 steps through a 128^3 field.
--correlate cross-correlates the pair on the device (photon_piv_correlate: 32 px windows, 16 px grid, R 16; one and two
passes), prints the correlation's ms per pass and the median / 95th percentile over windows of |measured - truth| (truth:
the mean image displacement of the particles whose frame-1 centroid lies in the window, counting those the laser sheet lights
to >= 10 % of its peak, windows with >= 5 of them), and
times 1024^2 pairs at win 32 / step 16 / R 16 and win 64 / step 32 / R 32 (multiply-adds per second, share of the f32
FMA peak).  --deform adds iterative image deformation (PhotonLibrary.correlate_deform, header section 7): the same error
figures after 1, 2 and 3 iterations against the same truth and windows (and against the truth that collects the particles
by their position half-way between the frames, which is where a symmetric warp measures), and at 1024^2 the device-event
times of the coefficients, one warp, one residual correlation at R 4 and one validate, and the wall time of the whole call
beside correlate(passes=2).  --phase holds the FFT correlator (photon_piv_correlate_phase, header section 13: phase
correlation, Gaussian window of win / 4, spectral filter for 2.5 px particles) next to photon_piv_correlate: the sample
pair's error figures for one pass and for three deformation iterations with both methods, and at 1024^2 the device-event
times of both kernels in the same run, alternating (win 32 / step 16 at R 4 and 15 | 16, win 64 / step 32 at R 4 and 31 | 32;
the median of seven), and the wall time of correlate_deform with both methods.  --multigrid times multigrid window
refinement (PhotonLibrary.correlate_multigrid, header section 16: 64 / 32 -> 32 / 16 -> 16 / 8, iterations 1, 1, 2) on the
sample pair next to correlate_deform at the final grid's 16 / 8 with three iterations: device events around the queued
chains (nothing copied back), alternating, the median of seven; per level the difference between the chains that stop
there; and the time of one photon_piv_regrid per grid change.  --weighting times the weighted direct correlator
(photon_piv_correlate_weighted, header section 18, Gaussian table of win / 4) next to photon_piv_correlate at 1024^2 and
prints the response table of DESIGN.md section 4.3q from the device: the amplitude correlate_deform recovers of
dy = sin(2 pi x / lambda) at lambda 24 and 40 px with a top-hat and with a Gaussian window, after pass 0 and after six
iterations.  Run it on a GPU box under a time limit of its own:

    timeout -k 10 600 python tools/piv_pair.py [--tiff DIR] [--bench-advect] [--correlate] [--deform] [--phase] [--multigrid]
                                               [--mask] [--weighting]
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
from photon_amd import deflections  # noqa: E402
from photon_amd import piv_correlation as pc  # noqa: E402
from photon_amd import piv_pairs as pp  # noqa: E402
from photon_amd.library import PhotonLibrary, _Correlator  # noqa: E402
from photon_amd.ray_tracing import postprocess_image, write_tiff_u16  # noqa: E402

# the sample frame's particle field (run_simulation_02.py:949-965 with the sample parameters): 1.5 x the field of view
BOX_MIN, BOX_MAX = (-7.5e4, -7.5e4, -7.5e3), (7.5e4, 7.5e4, 7.5e3)
BEAM_FWHM, IRRADIANCE = 730.0, 500.0
FMA_PEAK = 157.3e12 / 2             # MI355X f32 vector peak, FMA per second


def correlate_ms(lib, a, b, win, step, radius, offset=None, reps=20):
    """Device time of one photon_piv_correlate call (events around `reps` back-to-back calls, after a warm-up)."""
    h, w = a.shape
    optr = offset.data_ptr() if offset is not None else 0
    lib.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, radius, optr)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        lib.piv_correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, radius, optr)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def correlate_pair(lib, images, records, cam, rays, lit, row):
    """--correlate on the sample pair, then the 1024^2 timings; adds its figures to `row`.  lit: the particles the truth
    counts (those inside the light sheet: the others image too faintly to take part in the correlation)."""
    win, step, radius = 32, 16, 16
    a, b = (torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda() for im in images)
    m1 = deflections.dot_means(records[0], rays, 1, "arrived")
    pos = pc.image_positions(deflections.to_pixels(m1["pos"], cam), cam)[lit]
    d = pp.image_displacements(records[0], records[1], cam, rays)[lit]
    truth, count = pc.window_truth(pos, d, images[0].shape, win, step, min_count=5)
    ms1 = correlate_ms(lib, a, b, win, step, radius)
    vec1, flags1 = lib.correlate(a, b, win, step, radius, passes=1)
    offsets = torch.from_numpy(pc.predictor(vec1, flags1, pc.normalized_median_test(vec1))).cuda()
    ms2 = correlate_ms(lib, a, b, win, step, radius, offsets)
    vec2, flags2 = lib.correlate(a, b, win, step, radius, passes=2)
    use = np.isfinite(truth).all(axis=-1)
    for k, (vec, flags, ms) in enumerate(((vec1, flags1, ms1), (vec2, flags2, ms2)), 1):
        ok = use & ((flags & pc.FLAG_FLAT) == 0)
        err = np.hypot(*(pc.sensor_displacements(vec, cam)[ok] - truth[ok]).T)
        print(f"correlation pass {k}: {ms:.3f} ms ({vec.shape[0]} x {vec.shape[1]} windows of {win} px, step {step}, R {radius}); "
              f"|measured - truth| over {int(ok.sum())} windows with >= 5 particles: median {np.median(err):.4f} px, "
              f"95th percentile {np.percentile(err, 95):.4f} px")
        row[f"correlate_pass{k}_ms"] = round(ms, 4)
        row[f"correlate_pass{k}_median_err_px"] = float(np.median(err))
        row[f"correlate_pass{k}_p95_err_px"] = float(np.percentile(err, 95))
    row["correlate_windows_with_truth"] = int(use.sum())
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    big = [torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6))]
    for win, step, radius in ((32, 16, 16), (64, 32, 32)):
        ms = correlate_ms(lib, big[0], big[1], win, step, radius)
        n_rows, n_cols = pc.grid_shape((1024, 1024), win, step)
        fma = n_rows * n_cols * (2 * radius + 1) ** 2 * win * win
        rate = fma / (ms * 1e-3)
        print(f"1024^2 pair, win {win} step {step} R {radius}: {ms:.3f} ms, {fma / 1e9:.2f} G multiply-adds, "
              f"{rate / 1e12:.2f} T FMA/s = {100 * rate / FMA_PEAK:.1f} % of the f32 FMA peak")
        row[f"correlate_1024_w{win}_ms"] = round(ms, 4)
        row[f"correlate_1024_w{win}_fma_peak_frac"] = round(rate / FMA_PEAK, 4)


def event_ms(fn, reps=20):
    """Device time of one call of fn (events around `reps` back-to-back calls, after a warm-up)."""
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fns, reps=12, warm=3):
    """Median wall time of each of `fns` (name -> call that ends synchronised), alternating, after a warm-up."""
    times = {k: [] for k in fns}
    for rep in range(warm + reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= warm:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return {k: float(np.median(v)) for k, v in times.items()}


def deform_pair(lib, images, records, cam, rays, lit, row):
    """--deform on the sample pair, then the 1024^2 timings; adds its figures to `row`."""
    win, step, radius = 32, 16, 16
    a, b = (torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda() for im in images)
    m1 = deflections.dot_means(records[0], rays, 1, "arrived")
    pos = pc.image_positions(deflections.to_pixels(m1["pos"], cam), cam)[lit]
    d = pp.image_displacements(records[0], records[1], cam, rays)[lit]
    flip = -1.0 if bool(cam.get("implement_diffraction", False)) else 1.0
    truths = {"frame1": pc.window_truth(pos, d, images[0].shape, win, step, min_count=5)[0],
              "halfway": pc.window_truth(pos + 0.5 * d * np.array([flip, 1.0]), d, images[0].shape, win, step, min_count=5)[0]}
    for it in (1, 2, 3):
        vec, status = lib.correlate_deform(a, b, win, step, radius, iterations=it)
        line = f"deformation, {it} iteration(s), {int(((status & 8) != 0).sum())} of {status.size} vectors replaced:"
        for name, truth in truths.items():
            ok = np.isfinite(truth).all(axis=-1) & ((status & pc.FLAG_FLAT) == 0)          # --correlate's window selection
            err = np.hypot(*(pc.sensor_displacements(vec, cam)[ok] - truth[ok]).T)
            line += f" {name} truth ({int(ok.sum())} windows) median {np.median(err):.4f} px, 95th percentile {np.percentile(err, 95):.4f} px;"
            row[f"deform{it}_{name}_median_err_px"] = float(np.median(err))
            row[f"deform{it}_{name}_p95_err_px"] = float(np.percentile(err, 95))
        print(line)
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    big = [torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6))]
    h = w = 1024
    for win, step in ((32, 16), (64, 32)):
        r, c = pc.grid_shape((h, w), win, step)
        coef, out = torch.empty_like(big[0]), torch.empty_like(big[0])
        vec, flg, _ = lib.piv_correlate(big[0].data_ptr(), big[1].data_ptr(), w, h, win, step, win // 2)
        field, smooth = torch.empty((r, c, 2), device="cuda"), torch.empty((r, c, 2), device="cuda")
        status = torch.empty((r, c), dtype=torch.int32, device="cuda")
        lib.piv_validate(0, vec.data_ptr(), flg.data_ptr(), r, c, field.data_ptr(), smooth.data_ptr(), status.data_ptr())
        ms = {"coefficients": event_ms(lambda: lib.bspline_coefficients(big[0].data_ptr(), w, h, coef.data_ptr())),
              "warp": event_ms(lambda: lib.piv_deform(coef.data_ptr(), w, h, smooth.data_ptr(), 2, r, c, win, step, -0.5, out.data_ptr())),
              "correlate_r4": event_ms(lambda: lib.piv_correlate(big[0].data_ptr(), big[1].data_ptr(), w, h, win, step, 4)),
              "correlate_full": event_ms(lambda: lib.piv_correlate(big[0].data_ptr(), big[1].data_ptr(), w, h, win, step, win // 2)),
              "validate": event_ms(lambda: lib.piv_validate(0, vec.data_ptr(), flg.data_ptr(), r, c, field.data_ptr(), smooth.data_ptr(),
                                                            status.data_ptr()))}
        ms.update(wall_ms({"correlate_deform_3_wall": lambda: lib.correlate_deform(big[0], big[1], win, step, iterations=3),
                           "correlate_2_passes_wall": lambda: lib.correlate(big[0], big[1], win, step, passes=2)}))
        print(f"1024^2, win {win} step {step} ({r} x {c} nodes): " + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
        for k, v in ms.items():
            row[f"deform_1024_w{win}_{k}_ms"] = round(v, 4)


def phase_pair(lib, images, records, cam, rays, lit, row):
    """--phase on the sample pair, then the 1024^2 timings; adds its figures to `row`."""
    win, step = 32, 16
    a, b = (torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda() for im in images)
    m1 = deflections.dot_means(records[0], rays, 1, "arrived")
    pos = pc.image_positions(deflections.to_pixels(m1["pos"], cam), cam)[lit]
    d = pp.image_displacements(records[0], records[1], cam, rays)[lit]
    flip = -1.0 if bool(cam.get("implement_diffraction", False)) else 1.0
    truths = {"one_pass": pc.window_truth(pos, d, images[0].shape, win, step, min_count=5)[0],
              "deform3": pc.window_truth(pos + 0.5 * d * np.array([flip, 1.0]), d, images[0].shape, win, step, min_count=5)[0]}
    print("sample pair, |measured - truth| (one pass: frame-1 truth; 3 deformation iterations: half-way truth):")
    for method in ("direct", "phase"):
        results = {"one_pass": lib.correlate(a, b, win, step, method=method), "deform3": lib.correlate_deform(a, b, win, step, iterations=3, method=method)}
        for name, (vec, status) in results.items():
            ok = np.isfinite(truths[name]).all(axis=-1) & ((status & pc.FLAG_FLAT) == 0)
            err = np.hypot(*(pc.sensor_displacements(vec, cam)[ok] - truths[name][ok]).T)
            print(f"  {method:6s} {name:8s} {int(ok.sum())} windows: median {np.median(err):.4f} px, 95th percentile {np.percentile(err, 95):.4f} px, "
                  f"{int((err > 1.0).sum())} beyond 1 px")
            row[f"phase_{method}_{name}_median_err_px"] = float(np.median(err))
            row[f"phase_{method}_{name}_p95_err_px"] = float(np.percentile(err, 95))
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    big = [torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6))]
    h = w = 1024
    p0, p1 = big[0].data_ptr(), big[1].data_ptr()
    for win, step in ((32, 16), (64, 32)):
        calls = {}
        for R in (4, win // 2):
            Rp = min(R, win // 2 - 1)
            calls[f"direct_r{R}"] = lambda R=R: lib.piv_correlate(p0, p1, w, h, win, step, R)
            calls[f"phase_r{Rp}"] = lambda Rp=Rp: lib.piv_correlate_phase(p0, p1, w, h, win, step, Rp, mode=1, window_sigma=win / 4.0, diameter=2.5)
        times = {k: [] for k in calls}
        for rep in range(10):                               # three warm-up rounds, then seven; one event pair per call
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    times[k].append(e0.elapsed_time(e1))
        ms = {k: float(np.median(v)) for k, v in times.items()}
        ms.update(wall_ms({"correlate_deform_3_direct_wall": lambda: lib.correlate_deform(big[0], big[1], win, step, iterations=3),
                           "correlate_deform_3_phase_wall": lambda: lib.correlate_deform(big[0], big[1], win, step, iterations=3, method="phase")}))
        print(f"1024^2, win {win} step {step}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
        for k, v in ms.items():
            row[f"phase_1024_w{win}_{k}_ms"] = round(v, 4)


def multigrid_pair(lib, images, row):
    """--multigrid on the sample pair; adds its figures to `row`."""
    from photon_amd import piv_multigrid as pm
    schedule, iterations = pm.DEFAULT_SCHEDULE, pm.DEFAULT_ITERATIONS
    a, b = (torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda() for im in images)
    h, w = a.shape
    win, step = schedule[-1]

    def chain(schedule, iterations):                        # the drivers' device side with their defaults, nothing copied back
        levels = pm.check_schedule((h, w), schedule, iterations, radius=None, residual_radius=4, method="direct")
        return lib._deform_chain(a, b, *levels, _Correlator([win for win, _ in levels[0]]).on_device(lib, (h, w), a.device))
    calls = {f"multigrid_to_level{n - 1}": lambda n=n: chain(schedule[:n], iterations[:n]) for n in range(1, len(schedule) + 1)}
    calls["correlate_deform_3"] = lambda: chain(((win, step),), (3,))
    for k, (src, dst) in enumerate(zip(schedule, schedule[1:])):
        r, c = pc.grid_shape((h, w), *src)
        fld = torch.zeros((r, c, 2), device="cuda")
        calls[f"regrid_{k}_to_{k + 1}"] = lambda fld=fld, r=r, c=c, src=src, dst=dst: lib.piv_regrid(fld.data_ptr(), 2, r, c, *src, w, h, *dst)
    times = {k: [] for k in calls}
    for rep in range(10):                                   # three warm-up rounds, then seven; one event pair per call
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times[k].append(e0.elapsed_time(e1))
    ms = {k: float(np.median(v)) for k, v in times.items()}
    last = 0.0
    for n in range(len(schedule)):
        ms[f"level{n}"] = ms[f"multigrid_to_level{n}"] - last
        last = ms[f"multigrid_to_level{n}"]
    ms["multigrid"] = last
    print(f"{h} x {w} sample pair, schedule {schedule}, iterations {iterations}, final grid {pc.grid_shape((h, w), win, step)}: "
          + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items() if not k.startswith("multigrid_to")))
    for k, v in ms.items():
        row[f"multigrid_{k}_ms"] = round(v, 4)


def mask_pair(lib, row):
    """--mask: photon_piv_correlate_masked next to photon_piv_correlate on phase_pair's 1024^2 pair, under an all-zero mask
    (every window clear), a disc over about 10 % of the frame, and a sparse dot lattice that touches every window (every
    window takes the normalised path); adds the medians to `row`."""
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    big = [torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6))]
    h = w = 1024
    yy, xx = np.mgrid[:h, :w]
    masks = {"zeros": np.zeros((h, w), bool), "disc": np.hypot(xx - 600.0, yy - 450.0) <= 183.0, "lattice": (yy % 12 == 5) & (xx % 12 == 5)}
    d_masks = {k: torch.from_numpy(m.astype(np.uint8)).cuda() for k, m in masks.items()}
    p0, p1 = big[0].data_ptr(), big[1].data_ptr()
    for win, step in ((32, 16), (64, 32), (16, 8)):
        for R in (4, win // 2):
            calls = {"plain": lambda: lib.piv_correlate(p0, p1, w, h, win, step, R)}
            for k, m in d_masks.items():
                calls[k] = lambda m=m: lib.piv_correlate_masked(p0, p1, m.data_ptr(), m.data_ptr(), w, h, win, step, R, win * win // 2)
            times = {k: [] for k in calls}
            for rep in range(10):                           # three warm-up rounds, then seven; one event pair per call
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if rep >= 3:
                        times[k].append(e0.elapsed_time(e1))
            ms = {k: float(np.median(v)) for k, v in times.items()}
            flg = {k: calls[k]()[1].cpu().numpy() for k in d_masks}
            share = {k: (float(((f & 32) != 0).mean()), float(((f & 16) != 0).mean())) for k, f in flg.items()}
            print(f"1024^2, win {win} step {step} R {R}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items()) + "; partial / masked out: "
                  + ", ".join(f"{k} {100 * a:.0f} % / {100 * b:.0f} %" for k, (a, b) in share.items()))
            for k, v in ms.items():
                row[f"mask_1024_w{win}_r{R}_{k}_ms"] = round(v, 4)


def weighting_pair(lib, row):
    """--weighting: photon_piv_correlate_weighted (Gaussian table, sigma = win / 4) next to photon_piv_correlate on
    mask_pair's 1024^2 pair, alternating, section 5 twice a round (its difference from itself is the run's resolution); then
    the response study of tests/piv_weighting_cases.py through correlate_deform, seeds 1 to 4.  Adds both to `row`."""
    import piv_weighting_cases as wc
    from photon_amd import piv_weighting as pw
    rng = np.random.default_rng(1)
    n = 20_000
    x, y = rng.uniform(-8, 1032, n), rng.uniform(-8, 1032, n)
    big = [torch.from_numpy(pc.particle_image((1024, 1024), x + dx, y + dy).astype(np.float32)).cuda() for dx, dy in ((0, 0), (3.3, -2.6))]
    h = w = 1024
    p0, p1 = big[0].data_ptr(), big[1].data_ptr()
    for win, step in ((32, 16), (64, 32), (16, 8)):
        table = torch.from_numpy(pw.window_weights(win)).cuda()
        for R in sorted({4, win // 4, win // 2}):
            calls = {"plain": lambda: lib.piv_correlate(p0, p1, w, h, win, step, R),
                     "weighted": lambda: lib.piv_correlate_weighted(p0, p1, table.data_ptr(), w, h, win, step, R),
                     "plain_again": lambda: lib.piv_correlate(p0, p1, w, h, win, step, R)}
            times = {k: [] for k in calls}
            for rep in range(10):                           # three warm-up rounds, then seven; one event pair per call
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if rep >= 3:
                        times[k].append(e0.elapsed_time(e1))
            ms = {k: float(np.median(v)) for k, v in times.items()}
            print(f"1024^2, win {win} step {step} R {R}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items())
                  + f"; weighted / plain {ms['weighted'] / ms['plain']:.4f}, plain again / plain {ms['plain_again'] / ms['plain']:.4f}")
            for k, v in ms.items():
                row[f"weighting_1024_w{win}_r{R}_{k}_ms"] = round(v, 4)
    print("response to dy = sin(2 pi x / lambda), win 32, step 8, six iterations, seeds 1-4 (pass 0 | after 6):")
    for lam in wc.WAVELENGTHS:
        for name, weighting in (("uniform", None), ("gaussian", "gaussian")):
            first, last = [], []
            for seed in (1, 2, 3, 4):
                im1, im2 = (np.array(c) for c in wc.response_pair(lam, seed))
                first.append(wc.amplitude(lib.correlate_deform(im1, im2, **wc.R_ARGS, iterations=0, weighting=weighting)[0], lam))
                last.append(wc.amplitude(lib.correlate_deform(im1, im2, **wc.R_ARGS, iterations=wc.R_ITERATIONS, weighting=weighting)[0], lam))
            print(f"  lambda {lam}, {name}: {min(first):+.3f} ... {max(first):+.3f} | {min(last):+.3f} ... {max(last):+.3f}")
            row[f"weighting_response_l{lam}_{name}"] = [round(min(first), 4), round(max(first), 4), round(min(last), 4), round(max(last), 4)]


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
    ap.add_argument("--correlate", action="store_true")
    ap.add_argument("--deform", action="store_true")
    ap.add_argument("--phase", action="store_true")
    ap.add_argument("--multigrid", action="store_true")
    ap.add_argument("--mask", action="store_true")
    ap.add_argument("--weighting", action="store_true")
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
    if args.correlate or args.deform or args.phase:
        sigma = BEAM_FWHM / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        lit = np.exp(-w1[:, 2] ** 2 / (2.0 * sigma * sigma)) >= 0.1       # within 2.15 sigma of the sheet's centre plane
    if args.correlate:
        correlate_pair(lib, images, records, cam, rays, lit, row)
    if args.deform:
        deform_pair(lib, images, records, cam, rays, lit, row)
    if args.phase:
        phase_pair(lib, images, records, cam, rays, lit, row)
    if args.multigrid:
        multigrid_pair(lib, images, row)
    if args.mask:
        mask_pair(lib, row)
    if args.weighting:
        weighting_pair(lib, row)
    print(json.dumps(row), flush=True)
    if not math.isfinite(row["p99_err_px"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
