"""Section 19c late in the run: photon_piv_stereo_triangulate and PhotonLibrary.self_calibrate_stereo on a held-back
non-blocking stream, with the rig of tests/test_streams_gpu.py -- the entry point takes its stream inside a job struct, so
that module's inventory does not see it; the module sorts behind test_streams_gpu.py for the reason
tests/test_zz_piv_stereo_streams_gpu.py records --, and the triangulation's time against the reconstruction's on a grid that
fills the chip (with the other timing bounds)."""
import ctypes

import numpy as np
import pytest

import piv_stereo_cases as base
import piv_stereo_selfcal_cases as cases
import test_streams_gpu as ts
import test_zz_piv_stereo_streams_gpu as streams
from photon_amd import library
from photon_amd import piv_stereo as ps

pytestmark = pytest.mark.gpu

WARMUP, REPS, LAUNCHES = 2, 7, 10
BOUND = 4.0


@pytest.fixture(scope="module")
def rig(photon):
    return ts.Rig()


def test_triangulate_on_a_held_back_stream(photon, rig):
    pl, field, flags = cases.disparity_inputs("9x29")
    cams = base.cameras("asymmetric")

    def call(t, stream):
        return photon.piv_stereo_triangulate(t["d"].data_ptr(), 4, cams, pl, cases.WIN, cases.STEP, 4, t["g"].data_ptr(), stream=stream)
    want, got = streams.held_back(rig, "photon_piv_stereo_triangulate", {"d": field, "g": flags}, call, waits=False)
    assert got == want


def test_the_driver_on_a_held_back_current_stream(photon, rig):
    frames = cases.inputs()[1]
    cams = cases.cameras()

    def run(t, _):
        corrected, report = photon.self_calibrate_stereo(t["a"], t["b"], cams, cases.PLANE, rounds=1, **cases.DISPARITY)
        return [corrected[0], corrected[1], report]
    want, got = streams.held_back(rig, "self_calibrate_stereo", {"a": frames[0][:2], "b": frames[1][:2]}, run, waits=True)
    assert len(got) == len(want) and not [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def test_four_iterations_cost_no_more_than_four_reconstructions(photon):
    """512 x 512 nodes (1024 blocks of 256 threads on 256 compute units).  Per round: the reconstruction with sigmas, the
    triangulation with 4 iterations, the reconstruction again, LAUNCHES launches each between two device events; medians of
    seven rounds after two warm-up rounds.  The bound counts operations: an iteration builds the two Jacobians and the
    Cholesky that the reconstruction builds once, and two polynomial evaluations in place of the sigma propagation.
    Measured on one MI355X: DESIGN.md section 4.3w."""
    import torch
    n, win, step = 512, 32, 16
    side = (n - 1) * step + win
    pl = ps.centred_plane(side, side, 30.0 / side)                  # 30 mm across: inside what the cameras were calibrated on
    cams = base.cameras("asymmetric")
    rng = np.random.default_rng(5)
    px = 0.5 / pl["pitch"]                                          # half a millimetre of displacement or disparity
    fields = [torch.from_numpy(rng.uniform(-px, px, (n, n, 4)).astype(np.float32)).cuda() for _ in range(2)]
    sigmas = [torch.from_numpy(rng.uniform(0.02, 0.2, (n, n, 2)).astype(np.float32)).cuda() for _ in range(2)]
    out8, out6 = (torch.empty((n, n, k), dtype=torch.float64, device="cuda") for k in (8, 6))
    flg, flg6 = (torch.empty((n, n), dtype=torch.int32, device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    rec = library._stereo_job(cams, pl, win, step)
    rec.d_field1, rec.d_field2, rec.field_stride = fields[0].data_ptr(), fields[1].data_ptr(), 4
    rec.d_sigma1, rec.d_sigma2 = sigmas[0].data_ptr(), sigmas[1].data_ptr()
    rec.n_rows, rec.n_cols, rec.d_out, rec.d_flags, rec.stream = n, n, out8.data_ptr(), flg.data_ptr(), stream
    tri = library._stereo_job(cams, pl, win, step, library.photon_piv_triangulate_t)
    tri.d_disparity, tri.field_stride, tri.iterations = fields[0].data_ptr(), 4, 4
    tri.n_rows, tri.n_cols, tri.d_out, tri.d_flags, tri.stream = n, n, out6.data_ptr(), flg6.data_ptr(), stream
    L = photon.lib

    def timed(entry, job):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        rc = 0
        for _ in range(LAUNCHES):
            rc |= entry(ctypes.byref(job))
        stop.record()
        stop.synchronize()
        assert rc == 0
        return start.elapsed_time(stop) * 1e3 / LAUNCHES           # microseconds per launch

    times = {"r": [], "t": [], "r2": []}
    for k in range(WARMUP + REPS):
        for name, entry, job in (("r", L.photon_piv_stereo_reconstruct, rec), ("t", L.photon_piv_stereo_triangulate, tri),
                                 ("r2", L.photon_piv_stereo_reconstruct, rec)):
            us = timed(entry, job)
            if k >= WARMUP:
                times[name].append(us)
    points = out6.cpu().numpy()
    assert not flg.cpu().numpy().any() and not flg6.cpu().numpy().any() and np.isfinite(points).all() and np.isfinite(out8.cpu().numpy()).all()      # every thread ran every step
    assert points[..., 4].max() < 1e-9
    t_r, t_t, t_r2 = (float(np.median(times[k])) for k in ("r", "t", "r2"))
    print(f"512 x 512 nodes: reconstruct with sigmas {t_r:.1f} us, again {t_r2:.1f} us, triangulate with 4 iterations {t_t:.1f} us (ratio "
          f"{t_t / t_r:.2f})")
    assert t_t <= BOUND * t_r, (t_t, t_r, t_r2)
