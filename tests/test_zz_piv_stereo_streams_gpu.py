"""Section 19 on a held-back non-blocking stream, with the rig of tests/test_streams_gpu.py (Rig, HeldBack, assert_delay_held): the
two entry points take their stream inside a job struct, so that module's inventory of `void *stream` prototypes does not
see them, and its purpose -- no stream-taking call without a held-back case -- is met here, as is the driver's.
The module sorts behind test_streams_gpu.py on purpose: its side stream is one more stream of the process, and with few
hardware queues every further stream moves the ones created later onto other queues; test_streams_gpu's own check that a
null-stream launch overtakes the held-back stream needs the two on different queues, as they are without this module
before it."""
import time

import pytest

import piv_stereo_cases as cases
import test_piv_stereo_gpu as base
import test_streams_gpu as ts

pytestmark = pytest.mark.gpu

dev, POISON, MASK_POISON, SETTINGS, SHIFTED = base.dev, base.POISON, base.MASK_POISON, base.SETTINGS, base.SHIFTED


@pytest.fixture(scope="module")
def src_coefficients(photon):
    return base.device_coefficients(photon, cases.image(cases.SRC, 21, n=3))[1]


@pytest.fixture(scope="module")
def rig(photon):
    return ts.Rig()


def held_back(rig, name, inputs, call, waits):
    """ts.held_back_run for a call on torch tensors: call(tensors, stream) on the null stream from the real inputs, twice;
    then on the side stream behind a delay, the inputs -- zeros until then -- filled behind the delay too.  Returns (want, got)
    as ts.flatten makes them."""
    import torch
    for _ in range(2):
        tensors = {k: dev(a) for k, a in inputs.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = call(tensors, 0)
        host_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        want = ts.flatten(result)
    staging = {k: dev(a) for k, a in inputs.items()}
    tensors = {k: torch.zeros_like(t) for k, t in staging.items()}
    torch.cuda.synchronize()
    with ts.HeldBack(rig, ts.wait_delay_ms(host_s) if waits else ts.DELAY_MS) as hb:
        for k, t in staging.items():
            tensors[k].copy_(t)
        result = call(tensors, rig.side.cuda_stream)
        held = hb.held()
        got = ts.flatten(result)                                         # copies back on the side stream, behind the work
    hb.finish()
    ts.assert_delay_held(name, waits, held, hb.delay_ms, host_s)
    return want, got


def test_dewarp_on_a_held_back_stream(photon, rig, src_coefficients):
    import torch
    out = cases.OUTS[0]
    poly, grid = cases.dewarp_cameras(cases.SRC, out)["full"]
    h, w = cases.SRC

    def call(t, stream):
        d_out = torch.full((2,) + out, float(POISON), dtype=torch.float32, device="cuda")
        d_mask = torch.full(out, MASK_POISON, dtype=torch.uint8, device="cuda")         # on the current stream: ahead of the launch on it
        photon.piv_dewarp(t["coef"].data_ptr(), h * w, 2, w, h, poly, grid, out[1], out[0], out[0] * out[1], d_out.data_ptr(), d_mask.data_ptr(),
                          stream)
        return d_out, d_mask
    want, got = held_back(rig, "photon_piv_dewarp", {"coef": src_coefficients}, call, waits=False)
    assert got == want


def test_reconstruct_on_a_held_back_stream(photon, rig):
    pl, fields, flags, sigmas = cases.stereo_inputs("9x11")
    cams = cases.cameras("asymmetric")
    inputs = {"f1": fields[0], "f2": fields[1], "g1": flags[0], "g2": flags[1], "s1": sigmas[0], "s2": sigmas[1]}

    def call(t, stream):
        return photon.piv_stereo_reconstruct(t["f1"].data_ptr(), t["f2"].data_ptr(), 4, cams, pl, cases.WIN, cases.STEP, t["g1"].data_ptr(),
                                             t["g2"].data_ptr(), t["s1"].data_ptr(), t["s2"].data_ptr(), stream=stream)
    want, got = held_back(rig, "photon_piv_stereo_reconstruct", inputs, call, waits=False)
    assert got == want


@pytest.mark.parametrize("plane", ["inside", "shifted"])
def test_the_driver_on_a_held_back_current_stream(photon, rig, plane):
    f1, f2 = cases.accuracy_pair("shear")
    cams, pl = cases.cameras("symmetric"), (cases.PLANE if plane == "inside" else SHIFTED)
    run = lambda t, _: photon.correlate_stereo(t["a"], t["b"], cams, pl, settings=dict(SETTINGS, iterations=2), sigma=True)     # noqa: E731
    want, got = held_back(rig, f"correlate_stereo_{plane}", {"a": f1, "b": f2}, run, waits=True)
    assert len(got) == len(want) and not [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
