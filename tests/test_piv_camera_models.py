"""The host models that share one point function (piv_stereo.sensor_points) and one f64 16-tap sum (piv_stereo.bspline_sample)
against recordings of what each returned while it still carried its own copy (tests/golden/piv_camera_*.npz, taken at the
commit before the models were merged).  Equality is of the raw bits, NaN positions included.  The inputs -- a 9 x 11 sensor, a
5 x 7 plane, a 3 x 5 x 7 volume -- hold the three places a slip in the point function would show: nodes outside the sensor,
a node exactly on the last pixel (x = W - 1, y = H - 1), and a coordinate that is NaN."""
import os

import numpy as np
import pytest

from photon_amd import piv_mart as pm
from photon_amd import piv_stereo as ps
from photon_amd import piv_tomo as pt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POLYS = ("edge", "outside", "nan")


def same_bits(got, want) -> bool:
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def test_the_inputs_hold_the_three_edge_cases():
    g = load("piv_camera_footprint.npz")
    sensor, plane = tuple(g["sensor"]), tuple(g["plane"])
    assert sensor == (9, 11) and plane == (5, 7)
    with np.errstate(all="ignore"):
        x, y = ps.folded_points(g["poly_edge"], g["grid"], plane)
        assert x[0, 6] == sensor[1] - 1 and y[4, 0] == sensor[0] - 1 and not ps.outside_mask(g["poly_edge"], g["grid"], plane, sensor).any()
        out = ps.outside_mask(g["poly_outside"], g["grid"], plane, sensor)
        assert out.any() and not out.all()
        x, _ = ps.folded_points(g["poly_nan"], g["grid"], plane)
        out = ps.outside_mask(g["poly_nan"], g["grid"], plane, sensor)
        assert np.isnan(x).any() and out[np.isnan(x)].all() and not out.all()


@pytest.mark.parametrize("name", POLYS)
def test_footprint_on_the_shared_point_function_returns_the_recorded_bits(name):
    g = load("piv_camera_footprint.npz")
    with np.errstate(all="ignore"):
        for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
            inside, index, weights = pm.footprint(g[f"poly_{name}"], g["grid"], tuple(g["plane"]), tuple(g["sensor"]), dtype)
            assert same_bits(inside, g[f"{name}_{tag}_inside"]) and same_bits(index, g[f"{name}_{tag}_index"]), tag
            assert same_bits(weights, g[f"{name}_{tag}_weights"]), tag


@pytest.mark.parametrize("name", POLYS)
def test_dewarp_models_on_the_shared_sum_return_the_recorded_bits(name):
    g = load("piv_camera_dewarp.npz")
    with np.errstate(all="ignore"):
        frames, mask = ps.dewarp_model(g["frames"], g[f"poly_{name}"], g["grid"], tuple(g["plane"]))
        frames32, mask32 = ps.dewarp_model_f32(g["coef"], g[f"poly_{name}"], g["grid"], tuple(g["plane"]))
    assert same_bits(frames, g[f"{name}_frames"]) and same_bits(mask, g[f"{name}_mask"])
    assert same_bits(frames32, g[f"{name}_frames_f32"]) and same_bits(mask32, g[f"{name}_mask_f32"])        # its own f32 sum, the shared point


def test_los_samples_on_the_shared_sum_return_the_recorded_bits():
    g = load("piv_camera_los.npz")
    (nz, ny, nx), sensor = tuple(g["shape"]), g["frames0"].shape[-2:]
    with np.errstate(all="ignore"):
        # per camera, some slice holds a node on the last pixel, some slice a NaN coordinate, some slice nodes outside
        for c in range(2):
            xy = [ps.folded_points(g["poly"][c][k], g["grids"][c], (ny, nx)) for k in range(nz)]
            assert any((x == sensor[1] - 1).any() and (y == sensor[0] - 1).any() for x, y in xy), c
            assert any(np.isnan(x).any() for x, _ in xy) and any((x < 0).any() for x, _ in xy), c
        samples, outside = pt.los_samples([g["frames0"], g["frames1"]], g["poly"], g["grids"], tuple(g["shape"]))
    assert outside.any() and not outside.all()
    assert same_bits(samples, g["samples"]) and same_bits(outside, g["outside"])
