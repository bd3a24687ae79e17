"""Section 21 on a held-back non-blocking stream, with the rig of tests/test_streams_gpu.py: the two entry points take their
stream inside a job struct, as section 20's do (tests/test_zz_piv_tomo_streams_gpu.py), so the inventory of `void *stream`
prototypes does not see them; its purpose is met here, for the entry points -- their zeroing of the accumulators included,
which has to be on the caller's stream -- and for the drivers.  The module sorts behind test_streams_gpu.py for the reason
tests/test_zz_piv_stereo_streams_gpu.py gives."""
import pytest

import piv_mart_cases as cases
import test_streams_gpu as ts
from photon_amd import piv_tomo as pt
from test_zz_piv_stereo_streams_gpu import held_back

pytestmark = pytest.mark.gpu

SHAPE = pt.shape_of(cases.VOLUME)
NVOX = SHAPE[0] * SHAPE[1] * SHAPE[2]
MAX_PIXELS = max(h * w for h, w in cases.SENSORS)


@pytest.fixture(scope="module")
def rig(photon):
    return ts.Rig()


def test_volume_mart_on_a_held_back_stream(photon, rig):
    import torch
    poly, grids, _ = cases.geometry()
    inputs = {f"f{c}": f for c, f in enumerate(cases.frames(2))}
    inputs.update(poly=poly, vol=cases.volumes(2), mask=cases.mask())

    def call(t, stream):
        d_vol = t["vol"].clone()                                                        # on the current stream: ahead of the launches on it
        d_acc = torch.full((2, 2, MAX_PIXELS), -1, dtype=torch.int64, device="cuda")
        photon.piv_volume_mart([t[f"f{c}"].data_ptr() for c in range(3)], [h * w for h, w in cases.SENSORS], 2, cases.SENSORS, grids, t["poly"].data_ptr(),
                               cases.VOLUME, NVOX, d_vol.data_ptr(), d_acc.data_ptr(), 3, 1, 0.05, cases.scale(2), t["mask"].data_ptr(), stream)
        return d_vol
    want, got = held_back(rig, "photon_piv_volume_mart", inputs, call, waits=False)
    assert got == want
    assert want[2] == cases.mart_want(2, 1, 0.05, 3).tobytes()                         # ts.flatten: dtype, shape, bytes


def test_volume_project_on_a_held_back_stream(photon, rig):
    import torch
    poly, grids, _ = cases.geometry()

    def call(t, stream):
        d_acc = [torch.full((2, h, w), -1, dtype=torch.int64, device="cuda") for h, w in cases.SENSORS]
        d_img = [torch.full((2, h, w), float("nan"), dtype=torch.float32, device="cuda") for h, w in cases.SENSORS]
        photon.piv_volume_project(t["vol"].data_ptr(), NVOX, 2, cases.SENSORS, grids, t["poly"].data_ptr(), cases.VOLUME, [a.data_ptr() for a in d_acc],
                                  [h * w for h, w in cases.SENSORS], cases.PROJECT_SCALE, [i.data_ptr() for i in d_img], stream)
        return tuple(d_acc) + tuple(d_img)
    want, got = held_back(rig, "photon_piv_volume_project", dict(poly=poly, vol=cases.volumes(2)), call, waits=False)
    assert got == want
    assert want[2] == cases.project_want(2)[0][0].tobytes()


def test_the_mart_drivers_on_a_held_back_current_stream(photon, rig):
    m = cases.chain_model("three")
    inputs = {f"f{c}": f for c, f in enumerate(m["frames"])}
    grid = dict(pt.CASE_GRID, win_z=8, step_z=8, radius_z=1)
    settings = dict(iterations=2, threshold=2e-4, scale_log2=27)                        # given: the frames are not read back on the host
    reconstruct = lambda t, _: photon.reconstruct_volume([t[k] for k in inputs], m["cameras"], pt.CASE_VOLUME, method="mart", **settings)     # noqa: E731
    want, got = held_back(rig, "reconstruct_volume", inputs, reconstruct, waits=True)   # the table's upload is a copy on the current stream
    assert got == want
    correlate = lambda t, _: photon.correlate_tomo([t[k] for k in inputs], m["cameras"], pt.CASE_VOLUME, reconstruction="mart", **settings, **grid)     # noqa: E731
    want, got = held_back(rig, "correlate_tomo", inputs, correlate, waits=True)
    assert len(got) == len(want) and not [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
