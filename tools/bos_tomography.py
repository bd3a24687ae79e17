"""Tomographic BOS on the device (include/parallel_ray_tracing.h sections 9 and 10).  Prints JSON lines for two measurements:

1. timing of photon_tomo_project, photon_tomo_backproject and one solver iteration at 128^3 and 256^3 voxels with
   8 x 512^2 rays (the rotated views of tests/tomography_cases.py at that size): ms per call from device events around
   five windows of about a quarter of a second each (median, smallest and largest), the shader clock read from hwmon while
   they run, with --compare-library a second build's operators in the same alternating windows and its solver iterations
   in alternating pairs ("this_over_other": the ratio of the medians per quantity), taps per second (the taps counted by
   the projector itself: a field of ones projects to planes x spacing / |e_a|), the adjoint's atomic bytes per second (8 per tap) next to the two f32 rates of the
   microarchitecture guide (1.3 TB/s contiguous, 0.08 TB/s scattered), the projector's gathered bytes per second, and the
   time of a solver iteration from five pairs of fixed-iteration solves of different length;
2. the rendered study: the BOS scene of tests/bos_density_cases.py through two off-centre blobs, the field rotated by
   R_y(pi k / 16) about the volume centre for k = 0 .. 15 (the camera stays where it is), each pair correlated and
   integrated (bos_density.reconstruct), the views' P at the valid nodes fed with tomography.view_rays(rotation = R_k^T,
   pivot = centre) to tomo_reconstruct: relative L2 error over the voxels above 10 % of the peak for K = 4, 8, 16.

With --deflections both also measure section 10 (tomography from the deflections themselves): photon_tomo_deflect,
photon_tomo_deflect_adjoint and one iteration of photon_tomo_reconstruct_deflections in the same alternating windows as the
projector and its adjoint (the frames of tests/deflection_cases.py, the blob's analytic deflections), and the rendered
study a second time from bos_density.deflection_data with tomography.view_rays and view_frames straight into
tomo_reconstruct_deflections ("route": "direct" next to "two_step").

Kernel times under a profiler come from a separate run.  Run it on a GPU box under a time limit:

    timeout -k 10 900 python tools/bos_tomography.py [--skip-timing] [--skip-study] [--deflections] [--compare-library build/variants/lib_tomo_plain.so]
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
import deflection_cases as dc  # noqa: E402
import tomography_cases as tc  # noqa: E402
from photon_amd import bos_density as bd  # noqa: E402
from photon_amd import scenes  # noqa: E402
from photon_amd import tomography as tm  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

F32_ATOMIC_TBS = dict(contiguous=1.3, scattered=0.08)     # MI355X_MICROARCH, global float atomics (f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def window_ms(fn, reps: int) -> float:
    """ms per call over one window of `reps` back-to-back calls (device events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def timed(fns: dict, window_s: float = 0.25, windows: int = 5) -> dict:
    """Every function of `fns` timed in `windows` windows of about window_s seconds each, the functions alternating window by
    window (so that a drifting clock or a neighbour's work meets all of them alike): per name the median, the smallest and
    the largest ms per call and the calls per window."""
    out = {}
    for name, fn in fns.items():
        fn()                                                       # warm-up: the code objects
        torch.cuda.synchronize()
        out[name] = dict(reps=max(5, int(np.ceil(window_s * 1e3 / window_ms(fn, 3)))), ms=[])
    for _ in range(windows):
        for name, fn in fns.items():
            out[name]["ms"].append(window_ms(fn, out[name]["reps"]))
    return {name: dict(median=float(np.median(r["ms"])), min=min(r["ms"]), max=max(r["ms"]), calls_per_window=r["reps"])
            for name, r in out.items()}


class ClockSampler:
    """The shader clock of the library's device while work runs: hwmon freq1_input (Hz) of its PCI function, read every 20 ms
    by a thread between start() and stop().  median_mhz is None where the file is not there."""
    def __init__(self, lib):
        import glob
        found = glob.glob(f"/sys/bus/pci/devices/{lib.pci_bus_id().lower()}/hwmon/hwmon*/freq1_input")
        self.path, self.samples, self.thread, self.run = (found[0] if found else None), [], None, False

    def _loop(self):
        while self.run:
            try:
                with open(self.path) as f:
                    self.samples.append(int(f.read()) / 1e6)
            except (OSError, ValueError):
                pass
            time.sleep(0.02)

    def start(self):
        import threading
        if self.path:
            self.run, self.thread = True, threading.Thread(target=self._loop, daemon=True)
            self.thread.start()

    def stop(self):
        if self.thread:
            self.run = False
            self.thread.join()
        return dict(median_mhz=float(np.median(self.samples)) if self.samples else None, samples=len(self.samples), source=self.path)


def spread(r: dict) -> str:
    return f"{r['median']:.3f} ({r['min']:.3f}-{r['max']:.3f}, {r['calls_per_window']} calls per window)"


def operator_timing(lib, n: int, n_side: int = 512, other=None, deflections: bool = False) -> dict:
    """other: a second build of the library (--compare-library): every operator and solver iteration this run times is timed
    for it too, in alternation, and held against this one's (its adjoint's result as well).  deflections: section 10's
    operators and solver iteration too, in the same windows."""
    c = tc.view_case(n, n_side)
    o, d = dev(c.origins), dev(c.dirs)
    stream = torch.cuda.current_stream().cuda_stream
    grid_rays = (*c.grid, o.data_ptr(), d.data_ptr(), c.n_rays)
    f = dev(tc.blob_field(c))
    p = torch.empty(c.n_rays, dtype=torch.float64, device="cuda")
    v = torch.zeros(c.shape, dtype=torch.float64, device="cuda")
    # the taps, counted by the projector: ones project to planes * spacing_a / |e_a|
    lib.tomo_project(torch.ones_like(f).data_ptr(), *grid_rays, p.data_ptr(), stream=stream)
    e = np.abs(c.dirs / np.linalg.norm(c.dirs, axis=1, keepdims=True)).max(axis=1)
    taps = 4 * int(np.rint(p.cpu().numpy() * e / c.spacing[0]).sum())
    lib.tomo_project(f.data_ptr(), *grid_rays, p.data_ptr(), stream=stream)
    libs = {"": lib} if other is None else {"": lib, "_other": other}
    fns = {}
    for tag, L in libs.items():
        fns["project" + tag] = lambda L=L: L.tomo_project(f.data_ptr(), *grid_rays, p.data_ptr(), stream=stream)
        fns["backproject" + tag] = lambda L=L: L.tomo_backproject(p.data_ptr(), *grid_rays, v.data_ptr(), stream=stream)
    extra = {}
    if deflections:
        cd = dc.view_frames_of(c)
        t1, t2 = dev(cd.t1), dev(cd.t2)
        frame_rays = (*c.grid, o.data_ptr(), d.data_ptr(), t1.data_ptr(), t2.data_ptr(), c.n_rays)
        g1, g2 = torch.empty_like(p), torch.empty_like(p)
        lib.tomo_deflect(f.data_ptr(), *frame_rays, g1.data_ptr(), g2.data_ptr(), stream=stream)
        for tag, L in libs.items():
            fns["deflect" + tag] = lambda L=L: L.tomo_deflect(f.data_ptr(), *frame_rays, g1.data_ptr(), g2.data_ptr(), stream=stream)
            fns["deflect_adjoint" + tag] = lambda L=L: L.tomo_deflect_adjoint(g1.data_ptr(), g2.data_ptr(), *frame_rays, v.data_ptr(),
                                                                              stream=stream)
    if other is not None:
        va, vb = torch.zeros_like(v), torch.zeros_like(v)
        lib.tomo_backproject(p.data_ptr(), *grid_rays, va.data_ptr(), stream=stream)
        other.tomo_backproject(p.data_ptr(), *grid_rays, vb.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        differ = float((va - vb).abs().max() / va.abs().max())
        if not differ <= 1e-12:
            raise SystemExit(f"the two libraries' adjoints differ by {differ:.2e} of max |v| at {n}^3")
        extra = dict(other_library=other.version(), adjoints_differ_by=differ)
    clock = ClockSampler(lib)
    clock.start()
    t = timed(fns)
    clock_read = clock.stop()
    ms_p, ms_b = t["project"]["median"], t["backproject"]["median"]
    # one solver iteration: pairs of solves of fixed length on the analytic projections, host clock around the synchronised call
    pa = dev(tc.blob_projection(c))
    out = torch.empty(c.shape, dtype=torch.float64, device="cuda")
    solves = {"solver_iteration": lambda L, its: L.tomo_reconstruct_ptr(pa.data_ptr(), *grid_rays, out.data_ptr(), lam=1.0, tol=0.0,
                                                                         max_iter=its, stream=stream)}
    if deflections:
        ga = [dev(g) for g in dc.blob_deflections(cd)]
        out_d = torch.empty_like(out)
        solves["direct_solver_iteration"] = lambda L, its: L.tomo_reconstruct_deflections_ptr(
            ga[0].data_ptr(), ga[1].data_ptr(), *frame_rays, out_d.data_ptr(), lam=1.0, tol=0.0, max_iter=its, stream=stream)

    def solve_ms(run, L, iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = run(L, iterations)
        return 1e3 * (time.perf_counter() - t0), st
    short, long_ = 4, 20
    per_it, last = {name + tag: [] for name in solves for tag in libs}, {}
    for name, run in solves.items():
        for L in libs.values():
            solve_ms(run, L, 2)
    for _ in range(5):
        for name, run in solves.items():
            for tag, L in reversed(libs.items()):               # this library last: its result is what is reported below
                ms_short, _ = solve_ms(run, L, short)
                ms_long, last[name] = solve_ms(run, L, long_)
                per_it[name + tag].append((ms_long - ms_short) / (long_ - short))

    def iteration(name):
        return f"{np.median(per_it[name]):.3f} ({min(per_it[name]):.3f}-{max(per_it[name]):.3f}, 5 pairs of {short} and {long_} iterations)"
    ms_it, st = float(np.median(per_it["solver_iteration"])), last["solver_iteration"]
    err = tc.rel_l2(out.cpu().numpy(), tc.blob_field(c))
    if other is not None:
        medians = {name: r["median"] for name, r in t.items()}
        medians.update({name: float(np.median(v)) for name, v in per_it.items()})
        extra.update({name + "_ms": spread(t[name]) for name in t if name.endswith("_other")},
                     **{name + "_ms": iteration(name) for name in per_it if name.endswith("_other")},
                     this_over_other={name: round(ms / medians[name + "_other"], 4) for name, ms in medians.items()
                                      if not name.endswith("_other")})
    if deflections:
        ms_d, ms_a, ms_it_d = t["deflect"]["median"], t["deflect_adjoint"]["median"], float(np.median(per_it["direct_solver_iteration"]))
        field, got = tc.blob_field(c), out_d.cpu().numpy()
        extra.update(deflect_ms=spread(t["deflect"]), deflect_adjoint_ms=spread(t["deflect_adjoint"]),
                     deflect_over_project=round(ms_d / ms_p, 2), deflect_adjoint_over_backproject=round(ms_a / ms_b, 2),
                     deflect_gtaps_per_s=round(taps / (ms_d * 1e-3) / 1e9, 2), deflect_adjoint_gtaps_per_s=round(taps / (ms_a * 1e-3) / 1e9, 2),
                     direct_solver_iteration_ms=iteration("direct_solver_iteration"),
                     direct_operators_share_of_iteration=round((ms_d + ms_a) / ms_it_d, 3),
                     direct_residual_after_20=last["direct_solver_iteration"]["residual"],
                     direct_rel_l2_error_after_20_mean_removed=round(tc.rel_l2(got - got.mean(), field - field.mean()), 4))
    tbs = taps * 8 / (ms_b * 1e-3) / 1e12
    return dict(extra, measurement="operators", voxels=f"{n}^3", rays=c.n_rays, taps=taps, project_ms=spread(t["project"]),
                backproject_ms=spread(t["backproject"]), shader_clock_under_load=clock_read,
                project_gtaps_per_s=round(taps / (ms_p * 1e-3) / 1e9, 2), backproject_gtaps_per_s=round(taps / (ms_b * 1e-3) / 1e9, 2),
                project_gather_tb_per_s=round(taps * 8 / (ms_p * 1e-3) / 1e12, 3), backproject_atomic_tb_per_s=round(tbs, 3),
                atomic_rate_vs_f32_contiguous=round(tbs / F32_ATOMIC_TBS["contiguous"], 3),
                atomic_rate_vs_f32_scattered=round(tbs / F32_ATOMIC_TBS["scattered"], 2),
                solver_iteration_ms=iteration("solver_iteration"), operators_share_of_iteration=round((ms_p + ms_b) / ms_it, 3),
                residual_after_20=st["residual"], rel_l2_error_after_20=round(err, 4))


# ---- the rendered study -------------------------------------------------------------------------------------------------
CENTRE = np.array([0.0, 0.0, bc.ORIGIN_Z + bc.EXTENT / 2])          # the volume's centre, z from the lens (the NRRD's frame)
BLOBS = (dict(offset=np.array([2000.0, -1500.0, 1000.0]), sigma=2500.0, amplitude=2.0),
         dict(offset=np.array([-3500.0, 2500.0, -3000.0]), sigma=2000.0, amplitude=1.5))
K_MAX = 16
RECON_N, RECON_EXTENT = 32, 24000.0


def blobs(x, y, z, centre, rotation=np.eye(3)):
    """rho - rho_0 of the two blobs, their offsets from `centre` rotated by `rotation`."""
    out = 0.0
    for b in BLOBS:
        c = centre + rotation @ b["offset"]
        out = out + b["amplitude"] * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * b["sigma"] ** 2))
    return out


def render_views(lib, n_pix: int = bc.N_PIX):
    """im1 (no volume) and, per view, im2 through the field rotated by R_y(pi k / K_MAX): (call, im1, [im2_k], [R_k])."""
    f = n_pix / bc.N_PIX
    kw = dict(n_dots=int(bc.N_DOTS * f * f), points_per_dot=bc.DOT_POINTS, rays_per_source=bc.DOT_RAYS, seed=11,
              field_half_width=2.8e4 * f, dot_diameter=bc.DOT_DIAMETER, n_pixels=n_pix)
    h = bc.EXTENT / (bc.VOL_N - 1)
    origin = (-bc.EXTENT / 2, -bc.EXTENT / 2, bc.ORIGIN_Z)
    ax = [origin[a] + np.arange(bc.VOL_N) * h for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    c1 = scenes.bos_scene(**kw)
    to_image = lambda im: torch.from_numpy(im.reshape(n_pix, n_pix).astype(np.float32)).cuda()      # noqa: E731
    im1 = to_image(lib.render(c1))
    frames, rotations, call = [], [], None
    with tempfile.TemporaryDirectory() as wd:
        for k in range(K_MAX):
            R = tc.rot_y(np.pi * k / K_MAX)
            path = scenes.write_nrrd(os.path.join(wd, f"view_{k:02d}.nrrd"), bd.RHO_0 + blobs(x, y, z, CENTRE, R), (h, h, h), origin)
            call = scenes.bos_scene(density_grad_filename=path, **kw)
            frames.append(to_image(lib.render(call)))
            rotations.append(R)
    return call, im1, frames, rotations


def rendered_study(lib, lams, n_pix: int = bc.N_PIX, deflections: bool = False):
    call, im1, frames, rotations = render_views(lib, n_pix)
    shape = (n_pix, n_pix)
    target, _, h_nodes = bd.node_geometry(shape, bc.WIN, bc.STEP, call, bc.ORIGIN_Z, bc.EXTENT)
    centre_world = CENTRE - np.array([0.0, 0.0, tm.WORLD_Z_SHIFT])
    views, direct = [], []
    for im2, R in zip(frames, rotations):
        phi, _, st = bd.reconstruct(lib, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, passes=2)
        o, d = tm.view_rays(call, target, rotation=R.T, pivot=centre_world)
        views.append((phi.ravel(), np.where(np.isfinite(phi), 1.0, 0.0).ravel(), o.reshape(-1, 3), d.reshape(-1, 3)))
        if deflections:
            g1, g2, w, nodes = bd.deflection_data(lib, im1, im2, call, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP, passes=2)
            t1, t2 = tm.view_frames(call, nodes, rotation=R.T)
            direct.append((g1.ravel(), g2.ravel(), w.ravel(), o.reshape(-1, 3), d.reshape(-1, 3), t1.reshape(-1, 3), t2.reshape(-1, 3)))
    hg = RECON_EXTENT / (RECON_N - 1)
    case = tc.Case((RECON_N,) * 3, (hg, hg, hg), centre_world - RECON_EXTENT / 2, views[0][2], views[0][3])
    x, y, z = case.nodes()
    truth = blobs(x, y, z, centre_world)
    support = ((x - centre_world[0]) ** 2 + (y - centre_world[1]) ** 2 + (z - centre_world[2]) ** 2 <= (RECON_EXTENT / 2) ** 2)
    high = truth > 0.1 * truth.max()
    for K in (4, 8, 16):
        use = views[::K_MAX // K]
        p, w, o, d = (np.concatenate([v[i] for v in use]) for i in range(4))
        for lam in lams:
            t0 = time.perf_counter()
            f, st = lib.tomo_reconstruct(p, *case.grid, o, d, w=w, support=support.astype(np.uint8), lam=lam, tol=1e-6, max_iter=500)
            ms = 1e3 * (time.perf_counter() - t0)
            rel = float(np.linalg.norm((f - truth)[high]) / np.linalg.norm(truth[high]))
            yield dict(measurement="rendered_study", route="two_step", views=K, sensor=f"{n_pix}x{n_pix}", nodes_per_view=int(views[0][0].size),
                       node_spacing_um=round(float(h_nodes), 1), voxels=f"{RECON_N}^3", voxel_spacing_um=round(hg, 1), lam=lam,
                       rays_used=st["rays_used"], unknowns=st["unknowns"], iterations=st["iterations"], converged=st["converged"],
                       solve_ms_with_copies=round(ms, 1), rel_l2_error_above_10pct=round(rel, 4),
                       peak_recovered=round(float(f.max() / truth.max()), 3))
        if not deflections:
            continue
        g1, g2, w, o, d, t1, t2 = (np.concatenate([v[i] for v in direct[::K_MAX // K]]) for i in range(7))
        for lam in lams:
            t0 = time.perf_counter()
            f, st = lib.tomo_reconstruct_deflections(g1, g2, *case.grid, o, d, t1, t2, w=w, support=support.astype(np.uint8), lam=lam,
                                                     tol=1e-6, max_iter=500)
            ms = 1e3 * (time.perf_counter() - t0)
            rel = float(np.linalg.norm((f - truth)[high]) / np.linalg.norm(truth[high]))
            yield dict(measurement="rendered_study", route="direct", views=K, sensor=f"{n_pix}x{n_pix}", nodes_per_view=int(direct[0][0].size),
                       node_spacing_um=round(float(h_nodes), 1), voxels=f"{RECON_N}^3", voxel_spacing_um=round(hg, 1), lam=lam,
                       rays_used=st["rays_used"], unknowns=st["unknowns"], iterations=st["iterations"], converged=st["converged"],
                       solve_ms_with_copies=round(ms, 1), rel_l2_error_above_10pct=round(rel, 4),
                       peak_recovered=round(float(f.max() / truth.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-study", action="store_true")
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--rays-side", type=int, default=512)
    ap.add_argument("--lams", default="0.1,1,10")
    ap.add_argument("--deflections", action="store_true",
                    help="section 10 too: its operators and solver iteration in the timing's windows, and the rendered study from the "
                         "deflections themselves next to the two-step one")
    ap.add_argument("--compare-library", default=None,
                    help="a second build of the library: its operators and solver iterations are timed in alternation with this one's "
                         "(this_over_other) and its adjoint is checked against this one's, e.g. the one-atomic-per-tap form: "
                         "python tools/build_variant.py tomo_plain -DPHOTON_TOMO_MERGE_LANES=0")
    a = ap.parse_args()
    lib = PhotonLibrary(build=False)
    lib.set_device(0)
    other = PhotonLibrary(a.compare_library, build=False) if a.compare_library else None
    if not a.skip_timing:
        for n in (int(v) for v in a.sizes.split(",")):
            print(json.dumps(operator_timing(lib, n, a.rays_side, other, a.deflections)), flush=True)
    if not a.skip_study:
        for row in rendered_study(lib, [float(v) for v in a.lams.split(",")], deflections=a.deflections):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
