"""Projected density from BOS displacements on the device (photon_integrate_gradient, include/parallel_ray_tracing.h
section 6).  Prints JSON lines for two measurements:

1. the solver alone on the Gaussian projection of tests/bos_density_cases.py at 256^2, 1024^2 and 2048^2 nodes, frame
   fixed, tol 1e-8: iterations, ms per call (host clock around the synchronised call, after a warm-up call), us per
   iteration, and the achieved GB/s of the byte model (15 f64 per node and iteration);
2. the end-to-end loop at a 1024^2 sensor: the off-centre blob of tests/bos_density_cases.py rendered without and through
   the volume (4-pixel splat), correlated in two passes (win 32, step 16), integrated, and held against the chief-ray
   projection: render, correlate and integrate ms, the relative L2 error over the nodes above 10 % of the peak and the
   argmax offset in grid steps; then the same with PhotonLibrary.correlate_deform (3 iterations of image deformation,
   header section 7) in place of the two-pass correlation.

Kernel times come from a separate run under rocprofv3 --kernel-trace --stats.  Run it on a GPU box under a time limit:

    timeout -k 10 600 python tools/bos_density.py [--skip-e2e]
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
from photon_amd import bos_density as bd  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

BYTES_PER_NODE_ITER = 15 * 8


def solver_timing(lib, n: int, reps: int = 3) -> dict:
    P, gx, gy, h = bc.gaussian_case(n)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (gx, gy, P)]
    phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    fixed = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    fixed[0, :] = fixed[-1, :] = fixed[:, 0] = fixed[:, -1] = 1
    args = (d[0].data_ptr(), d[1].data_ptr(), n, n, phi.data_ptr())
    kw = dict(d_fixed_ptr=fixed.data_ptr(), d_value_ptr=d[2].data_ptr(), hx=h, hy=h, tol=1e-8)
    st = lib.integrate_gradient_ptr(*args, **kw)                   # warm-up: the block cache, the code objects
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = lib.integrate_gradient_ptr(*args, **kw)               # synchronises its stream
        times.append(time.perf_counter() - t0)
    ms = 1e3 * min(times)
    it = max(st["iterations"], 1)
    err = float(np.linalg.norm(phi.cpu().numpy() - P) / np.linalg.norm(P))
    return dict(measurement="solver", nodes=f"{n}x{n}", iterations=st["iterations"], converged=st["converged"],
                residual=st["residual"], ms_per_call=round(ms, 3), us_per_iteration=round(1e3 * ms / it, 2),
                gb_per_s_model=round(BYTES_PER_NODE_ITER * n * n * it / (ms * 1e-3) / 1e9, 1), rel_l2_error=err)


def end_to_end(lib, n_pix: int = 1024) -> dict:
    with tempfile.TemporaryDirectory() as wd:
        c1, c2 = bc.blob_calls(lib, wd, False, n_pix)
        lib.render(c1)                                             # warm
        t0 = time.perf_counter()
        im1 = lib.render(c1)
        t1 = time.perf_counter()
        im2 = lib.render(c2)
        t2 = time.perf_counter()
    im1 = torch.from_numpy(im1.reshape(n_pix, n_pix).astype(np.float32)).cuda()
    im2 = torch.from_numpy(im2.reshape(n_pix, n_pix).astype(np.float32)).cuda()
    lib.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    vectors, flags = lib.correlate(im1, im2, win=bc.WIN, step=bc.STEP, passes=2)
    t4 = time.perf_counter()
    phi, mid, st = bd.integrate_vectors(lib, vectors, flags, (n_pix, n_pix), c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    t5 = time.perf_counter()
    P, mid, h = bc.truth(c2, n_pix)
    rel, off, holes = bc.errors(phi, P, mid, h)
    lib.correlate_deform(im1, im2, win=bc.WIN, step=bc.STEP, iterations=3)
    t6 = time.perf_counter()
    vectors_d, status_d = lib.correlate_deform(im1, im2, win=bc.WIN, step=bc.STEP, iterations=3)
    t7 = time.perf_counter()
    phi_d, _, st_d = bd.integrate_vectors(lib, vectors_d, status_d, (n_pix, n_pix), c2, bc.ORIGIN_Z, bc.EXTENT, bc.WIN, bc.STEP)
    rel_d, off_d, holes_d = bc.errors(phi_d, P, mid, h)
    deform = dict(correlate_ms_deform_3_iterations=round(1e3 * (t7 - t6), 2), deform_iterations_of_the_solver=st_d["iterations"],
                  deform_rel_l2_error=round(rel_d, 4), deform_nan_share=round(holes_d, 4),
                  deform_argmax_offset_steps=[round(off_d[0], 2), round(off_d[1], 2)], deform_replaced=int(((status_d & 8) != 0).sum()))
    return dict(deform, measurement="end_to_end", sensor=f"{n_pix}x{n_pix}", rays_per_frame=c1.num_rays, nodes=f"{phi.shape[0]}x{phi.shape[1]}",
                render_ms_without=round(1e3 * (t1 - t0), 1), render_ms_through=round(1e3 * (t2 - t1), 1),
                correlate_ms_two_passes=round(1e3 * (t4 - t3), 2), integrate_ms_with_host_steps=round(1e3 * (t5 - t4), 2),
                iterations=st["iterations"], rel_l2_error=round(rel, 4), nan_share=round(holes, 4), argmax_offset_steps=[round(off[0], 2), round(off[1], 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--sizes", default="256,1024,2048")
    a = ap.parse_args()
    lib = PhotonLibrary(build=False)
    lib.set_device(0)
    for n in (int(v) for v in a.sizes.split(",")):
        print(json.dumps(solver_timing(lib, n)), flush=True)
    if not a.skip_e2e:
        print(json.dumps(end_to_end(lib)), flush=True)


if __name__ == "__main__":
    main()
