"""Section 20 on a held-back non-blocking stream, with the rig of tests/test_streams_gpu.py: the two entry points take their
stream inside a job struct, so that module's inventory of `void *stream` prototypes does not see them; its purpose -- no
stream-taking call without a held-back case -- is met here, for the entry points and for the two drivers.  The module sorts
behind test_streams_gpu.py for the reason tests/test_zz_piv_stereo_streams_gpu.py gives."""
import numpy as np
import pytest

import piv_tomo_cases as cases
import test_streams_gpu as ts
from photon_amd import piv_tomo as pt
from test_zz_piv_stereo_streams_gpu import held_back

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig(photon):
    return ts.Rig()


def test_volume_los_on_a_held_back_stream(photon, rig):
    import torch
    n = 3
    coefs = cases.los_coefs(n)
    poly, grids = pt.los_coefficients(cases.los_cameras(n), cases.LOS_VOLUME)
    nz, ny, nx = pt.shape_of(cases.LOS_VOLUME)
    inputs = {f"c{c}": coefs[c] for c in range(n)}
    inputs["poly"] = poly

    def call(t, stream):
        d_out = torch.full((2, nz, ny, nx), float("nan"), dtype=torch.float32, device="cuda")      # on the current stream: ahead of the launch on it
        d_mask = torch.full((nz, ny, nx), 0xFF, dtype=torch.uint8, device="cuda")
        photon.piv_volume_los([t[f"c{c}"].data_ptr() for c in range(n)], [x.shape[1] * x.shape[2] for x in coefs], 2, [x.shape[1:] for x in coefs],
                              grids, t["poly"].data_ptr(), cases.LOS_VOLUME, nz * ny * nx, d_out.data_ptr(), d_mask.data_ptr(), 1, stream)
        return d_out, d_mask
    want, got = held_back(rig, "photon_piv_volume_los", inputs, call, waits=False)
    assert got == want


def test_correlate_volume_on_a_held_back_stream(photon, rig):
    shape, win, step, R, win_z, step_z, Rz, _, _ = cases.CORRELATOR["w16_r8_z16"]
    v1, v2, off, _ = cases.correlator_case("w16_r8_z16")

    def call(t, stream):
        return photon.piv_correlate_volume(t["a"].data_ptr(), t["b"].data_ptr(), shape[2], shape[1], shape[0], win, step, R, win_z, step_z, Rz,
                                           t["off"].data_ptr(), stream)
    want, got = held_back(rig, "photon_piv_correlate_volume", {"a": v1, "b": v2, "off": np.ascontiguousarray(off, np.int32)}, call, waits=False)
    assert got == want


def test_the_drivers_on_a_held_back_current_stream(photon, rig):
    frames, cameras, _ = cases.chain_model("three")
    inputs = {f"f{c}": f for c, f in enumerate(frames)}
    grid = dict(pt.CASE_GRID, win_z=8, step_z=8, radius_z=1)
    reconstruct = lambda t, _: photon.reconstruct_volume([t[k] for k in inputs], cameras, pt.CASE_VOLUME, mode="product")     # noqa: E731
    want, got = held_back(rig, "reconstruct_volume", inputs, reconstruct, waits=True)          # the table's upload is a copy on the current stream
    assert got == want
    correlate = lambda t, _: photon.correlate_tomo([t[k] for k in inputs], cameras, pt.CASE_VOLUME, **grid)                   # noqa: E731
    want, got = held_back(rig, "correlate_tomo", inputs, correlate, waits=True)
    assert len(got) == len(want) and not [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
