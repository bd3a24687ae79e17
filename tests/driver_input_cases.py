"""Case tables of tests/test_driver_inputs.py (CPU) and tests/test_driver_inputs_gpu.py: the arrays callers hold.

  variants(a, tmp_path)   (name, object) pairs that all hold the values of the C-contiguous numpy array `a` in another layout,
                          dtype, byte order or container; check_variant asserts that each really is what it is named for.
  DRIVERS                 the public methods of PhotonLibrary that take arrays, with the dimensions each argument must have.
  ROWS                    one small call per driver and argument: the 14 PIPELINES of tests/test_streams_gpu.py (imported, not
                          copied) and the rows that complete DRIVERS.  `vary` names the arguments a row runs the variants on.

Importing this module needs no GPU; torch is imported only where a variant is a tensor.
"""
import functools
import inspect
import itertools
import sys

import numpy as np

import deflection_cases as dc
import stream_cases as sc
import test_streams_gpu as ts
from photon_amd import piv_weighting as pw

SWAPPED = ">" if sys.byteorder == "little" else "<"
_FILE_NUMBER = itertools.count()


# ---- the variants --------------------------------------------------------------------------------------------------------------
def wider_float(a):
    """`a` in a float dtype that holds every value of a's own: f32 -> f64, f64 -> long double, anything else -> f64."""
    return a.astype(np.longdouble if a.dtype == np.float64 else np.float64)


def variants(a, tmp_path, tensors=True):
    """(name, object) pairs that hold the values of `a` (numpy, C-contiguous, native, at least 1-d).  The layouts that need
    two axes are left out for a 1-d array; the integer dtypes are added where every value is a whole number that fits."""
    a = np.ascontiguousarray(a)
    nd, shape = a.ndim, a.shape
    if nd >= 2:
        yield "fortran", np.asfortranarray(a)
        big = np.full(shape[:-2] + (shape[-2] + 7, shape[-1] + 9), 3, a.dtype)
        big[..., 3:3 + shape[-2], 5:5 + shape[-1]] = a
        yield "crop", big[..., 3:3 + shape[-2], 5:5 + shape[-1]]
        yield "rot90", np.rot90(np.ascontiguousarray(np.rot90(a, -1)))
    wide = np.full(shape[:-1] + (2 * shape[-1],), 3, a.dtype)
    wide[..., ::2] = a
    yield "every_second_column", wide[..., ::2]
    yield "flipud", np.flipud(np.ascontiguousarray(np.flipud(a)))
    yield "fliplr", np.ascontiguousarray(a[..., ::-1])[..., ::-1]
    yield "byte_order", a.astype((np.dtype("u2") if a.dtype.itemsize == 1 else a.dtype).newbyteorder(SWAPPED))
    ro = a.copy()
    ro.setflags(write=False)
    yield "read_only", ro
    path = tmp_path / f"variant_{next(_FILE_NUMBER)}.bin"          # a file of its own: an earlier map may still be open
    a.tofile(path)
    yield "memmap", np.memmap(path, dtype=a.dtype, mode="r", shape=shape)
    if a.dtype.kind == "f":
        yield "wider_float", wider_float(a)
    yield "nested_list", a.tolist()
    if a.dtype.kind != "b" and (a == np.rint(a)).all():
        for name, dt in (("uint8", np.uint8), ("uint16", np.uint16), ("int32", np.int32)):
            if a.dtype != dt and a.min() >= np.iinfo(dt).min and a.max() <= np.iinfo(dt).max:
                yield name, a.astype(dt)
    if tensors:
        import torch
        yield "torch_cpu", torch.from_numpy(a.copy())
        if nd >= 2:
            yield "torch_cpu_view", torch.from_numpy(np.ascontiguousarray(a.transpose())).permute(*reversed(range(nd)))
        else:
            yield "torch_cpu_view", torch.from_numpy(np.repeat(a, 2))[::2]


NEGATIVE_STRIDE = ("flipud", "fliplr", "rot90")


def values_of(v):
    """A variant's values as a base numpy array (a tensor through numpy(), which handles its strides)."""
    return np.asarray(v.numpy() if type(v).__module__.startswith("torch") else v)


def check_variant(name, v, a):
    """`v` holds the values of `a` and really has the property it is named for."""
    got = values_of(v)
    assert got.shape == a.shape and np.array_equal(got.astype(np.longdouble if a.dtype.kind == "f" else np.int64),
                                                   a.astype(np.longdouble if a.dtype.kind == "f" else np.int64)), name
    if name == "fortran":
        assert v.flags.f_contiguous and not v.flags.c_contiguous
    elif name in ("crop", "every_second_column"):
        assert not v.flags.c_contiguous and not v.flags.f_contiguous and all(s > 0 for s in v.strides) and v.base is not None
    elif name in NEGATIVE_STRIDE:
        assert min(v.strides) < 0 and not v.flags.c_contiguous
    elif name == "byte_order":
        assert v.dtype.byteorder == SWAPPED and not v.dtype.isnative
    elif name == "read_only":
        assert not v.flags.writeable and v.flags.c_contiguous and v.dtype == a.dtype
    elif name == "memmap":
        assert isinstance(v, np.memmap) and not v.flags.writeable and v.dtype == a.dtype
    elif name == "wider_float":
        assert v.dtype.kind == "f" and v.dtype.itemsize > a.dtype.itemsize
    elif name == "nested_list":
        assert isinstance(v, list) and (a.ndim == 1 or isinstance(v[0], list))
    elif name in ("uint8", "uint16", "int32"):
        assert v.dtype == np.dtype(name) and v.dtype != a.dtype
    elif name == "torch_cpu":
        assert v.device.type == "cpu" and v.is_contiguous()
    elif name == "torch_cpu_view":
        assert v.device.type == "cpu" and not v.is_contiguous()
    else:
        raise AssertionError(f"no property check for the variant {name}")


ALL_VARIANTS = ("fortran", "crop", "rot90", "every_second_column", "flipud", "fliplr", "byte_order", "read_only", "memmap",
                "wider_float", "nested_list", "uint8", "uint16", "int32", "torch_cpu", "torch_cpu_view")


def refused(a):
    """(name, object, exception) of what the ingest rule refuses whatever the argument: complex and object dtypes."""
    a = np.asarray(a)
    yield "complex", a.astype(np.complex64), TypeError
    yield "object", a.astype(object), TypeError


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
# method -> {array argument: the number of dimensions the helper asks for (None: any; the solver reshapes)}
_PAIR = {"im1": 2, "im2": 2}
_WINDOWED = {**_PAIR, "mask": 2, "weighting": 2}
_RAYS = {"origins": None, "dirs": None, "w": None, "support": 3}
DRIVERS = {
    "correlate": _WINDOWED,
    "correlate_deform": _WINDOWED,
    "correlate_multigrid": _WINDOWED,
    "correlation_predictor": _WINDOWED,
    "correlate_ensemble": {"frames1": 3, "frames2": 3},
    "preprocess_series": {"frames1": 3, "frames2": 3, "background": 2},
    "displacement_uncertainty": {**_PAIR, "field": 3},
    "optical_flow": {**_PAIR, "predictor": 3},
    "track_dots": {**_PAIR, "predictor": 3},
    "integrate_gradient": {"gx": 2, "gy": 2, "w": 2, "fixed": 2, "value": 2},
    "tomo_reconstruct": {"p": None, **_RAYS},
    "tomo_reconstruct_deflections": {"g1": None, "g2": None, "t1": None, "t2": None, **_RAYS},
}

# public methods that take host arrays for the C library's host-side arguments (np.ascontiguousarray at the call, no device
# tensor is made of them) or a RayTracingCall: not drivers, and outside the ingest rule
HOST_ARRAY_METHODS = ("morton_order", "sources_missing_sensor", "render", "render_moments", "volume_from_density", "sources_bos",
                      "sources_piv", "sources_piv_advected", "flow_from_grid", "tomo_project", "tomo_backproject", "tomo_deflect",
                      "tomo_deflect_adjoint", "tomo_reconstruct_ptr", "tomo_reconstruct_deflections_ptr")


def array_parameter_names():
    return sorted({p for params in DRIVERS.values() for p in params})


def methods_with_array_parameters(cls):
    """Public methods of `cls` with a parameter that carries one of the drivers' array names."""
    names = set(array_parameter_names())
    out = {}
    for name, f in inspect.getmembers(cls, inspect.isfunction):
        if name.startswith("_"):
            continue
        hit = [p for p, spec in inspect.signature(f).parameters.items()          # (track_dots' background is a float, by annotation)
               if p in names and str(spec.annotation) not in ("float", "int", "bool", "str")]
        if hit:
            out[name] = hit
    return out


# ---- the rows ------------------------------------------------------------------------------------------------------------------
class Row:
    """method: the driver; make_inputs() -> {key: numpy}; run(photon, {key: object}); vary: {key: the driver's argument} for
    the keys that the variants are run on (every key is an array argument; a row that repeats another's images varies only
    what it adds)."""
    def __init__(self, method, make_inputs, run, vary):
        self.method, self.make_inputs, self.run, self.vary = method, make_inputs, run, vary


_METHOD_OF_PIPELINE = {"correlate_two_passes": "correlate", "correlate_multigrid_mask": "correlate_multigrid",
                       "correlate_multigrid_phase": "correlate_multigrid", "correlate_multigrid_gaussian": "correlate_multigrid"}
_ARGUMENT_OF_KEY = {("track_dots", "field"): "predictor", ("preprocess_series", "frames"): "frames1"}


def _pipeline_rows():
    rows = {}
    for name, (_, make_inputs, run) in ts.PIPELINES.items():
        method = _METHOD_OF_PIPELINE.get(name, name)
        assert method in DRIVERS, f"the pipeline {name} is no driver by that name: give it a line in _METHOD_OF_PIPELINE"
        make = functools.lru_cache(maxsize=None)(make_inputs)
        rows[name] = Row(method, make, run, {k: _ARGUMENT_OF_KEY.get((method, k), k) for k in make()})
    return rows


def _window_table():
    return pw.window_weights(32, "gaussian", 9.0).astype(np.float32)


def _mask():
    return ts._mask()


def _deflection_inputs():
    """tomography's exact family (deflection_cases.runs_case): whole-number deflections on rays whose weights are multiples
    of 2^-7, whole-number weights, so that no sum of the one iteration depends on the order of its atomics."""
    c = dc.runs_case()
    rng = np.random.default_rng(71)
    support = np.ones(c.shape, np.uint8)
    support[0, :2, :3] = 0
    return dict(g1=c.y1, g2=c.y2, origins=c.origins, dirs=c.dirs, t1=c.t1, t2=c.t2, w=rng.integers(1, 4, c.n_rays).astype(np.float64),
                support=support)


def _tomo_more():
    rng = np.random.default_rng(72)
    k, j, i = np.meshgrid(*(np.arange(sc.TOMO_N),) * 3, indexing="ij")
    support = (((i - 5.5) ** 2 + (j - 5.5) ** 2 + (k - 5.5) ** 2) <= 30.0).astype(np.uint8)
    return dict(**ts._tomo_inputs(), w=rng.integers(1, 4, 2 * sc.TOMO_N ** 2).astype(np.float64), support=support)


def _gradient_more():
    g = ts._gradient_inputs()
    fixed = np.zeros(g["gx"].shape, np.uint8)
    fixed[0, :] = fixed[:, 0] = fixed[16, 20] = 1
    value = np.random.default_rng(73).normal(0.0, 1.0, g["gx"].shape)
    return dict(gx=g["gx"], gy=g["gy"], fixed=fixed, value=value)


def _background_inputs():
    frames = ts._frames()
    return dict(frames=frames, frames2=frames[::-1].copy(), background=(frames.min(axis=0) * np.float32(0.75)).astype(np.float32))


def _more_rows():
    pair, deflect = ts._pair_inputs, dc.runs_case
    return {
        "tomo_reconstruct_deflections": Row(
            "tomo_reconstruct_deflections", _deflection_inputs,
            lambda p, t: p.tomo_reconstruct_deflections(t["g1"], t["g2"], *deflect().grid, t["origins"], t["dirs"], t["t1"], t["t2"],
                                                        w=t["w"], support=t["support"], lam=1.0, tol=0.0, max_iter=1),
            {k: k for k in ("g1", "g2", "origins", "dirs", "t1", "t2", "w", "support")}),
        "tomo_reconstruct_w_support": Row(
            "tomo_reconstruct", _tomo_more,
            lambda p, t: p.tomo_reconstruct(t["p"], *sc.TOMO_GRID, t["origins"], t["dirs"], w=t["w"], support=t["support"], lam=0.5,
                                            tol=0.0, max_iter=sc.SOLVER_ITERATIONS), {"w": "w", "support": "support"}),
        "integrate_gradient_fixed_value": Row(
            "integrate_gradient", _gradient_more,
            lambda p, t: p.integrate_gradient(t["gx"], t["gy"], fixed=t["fixed"], value=t["value"], tol=0.0, max_iter=sc.SOLVER_ITERATIONS),
            {"fixed": "fixed", "value": "value"}),
        "correlate_mask": Row("correlate", lambda: pair(mask=_mask()),
                              lambda p, t: p.correlate(t["im1"], t["im2"], win=32, step=16, radius=8, mask=t["mask"]), {"mask": "mask"}),
        "correlate_weighting": Row("correlate", lambda: pair(weighting=_window_table()),
                                   lambda p, t: p.correlate(t["im1"], t["im2"], win=32, step=16, radius=8, weighting=t["weighting"]),
                                   {"weighting": "weighting"}),
        "correlate_deform_mask": Row("correlate_deform", lambda: pair(mask=_mask()),
                                     lambda p, t: p.correlate_deform(t["im1"], t["im2"], win=32, step=16, radius=8, iterations=1,
                                                                     mask=t["mask"]), {"mask": "mask"}),
        "correlate_deform_weighting": Row("correlate_deform", lambda: pair(weighting=_window_table()),
                                          lambda p, t: p.correlate_deform(t["im1"], t["im2"], win=32, step=16, radius=8, iterations=1,
                                                                          weighting=t["weighting"]), {"weighting": "weighting"}),
        "correlate_multigrid_weighting": Row("correlate_multigrid", lambda: pair(weighting=_window_table()),
                                             lambda p, t: p.correlate_multigrid(t["im1"], t["im2"], schedule=((32, 16),), iterations=(1,),
                                                                                radius=8, weighting=t["weighting"]),
                                             {"weighting": "weighting"}),
        "correlation_predictor_mask": Row("correlation_predictor", lambda: pair(mask=_mask()),
                                          lambda p, t: p.correlation_predictor(t["im1"], t["im2"], win=32, step=16, radius=8, mask=t["mask"]),
                                          {"mask": "mask"}),
        "correlation_predictor_weighting": Row("correlation_predictor", lambda: pair(weighting=_window_table()),
                                               lambda p, t: p.correlation_predictor(t["im1"], t["im2"], win=32, step=16, radius=8,
                                                                                    weighting=t["weighting"]), {"weighting": "weighting"}),
        "optical_flow_predictor": Row("optical_flow", lambda: pair(sc.SMALL, predictor=sc.grid_field(sc.SMALL, 32, 16, seed=6)),
                                      lambda p, t: p.optical_flow(t["im1"], t["im2"], t["predictor"], win=32, step=16, warps=1, iterations=8),
                                      {"predictor": "predictor"}),
        "preprocess_series_background": Row("preprocess_series", _background_inputs,
                                            lambda p, t: p.preprocess_series(t["frames"], t["frames2"], background=t["background"],
                                                                             minmax_radius=2, floor=0.05),
                                            {"frames2": "frames2", "background": "background"}),
    }


@functools.lru_cache(maxsize=None)
def rows():
    out = _pipeline_rows()
    more = _more_rows()
    assert not set(out) & set(more)
    for row in more.values():
        row.make_inputs = functools.lru_cache(maxsize=None)(row.make_inputs)
    out.update(more)
    return out


def covered_arguments():
    """{(method, argument)} that some row runs the variants on."""
    return {(row.method, arg) for row in rows().values() for arg in row.vary.values()}


# what a mask= is run as besides its layouts: the same exclusion in four dtypes and two nonzero values
def mask_forms(m):
    m = np.asarray(m) != 0
    return (("bool", m.copy()), ("uint8_0_1", m.astype(np.uint8)), ("uint8_0_255", m.astype(np.uint8) * np.uint8(255)),
            ("float32", m.astype(np.float32) * np.float32(0.5)))


# ---- camera counts -------------------------------------------------------------------------------------------------------------
# name -> (gain, pedestal, dtype): rint(pedestal + gain im), saturating at the dtype's top as a sensor does
CAMERA_SETTINGS = {"8bit": (200.0, 20.0, np.uint8), "12bit": (3000.0, 64.0, np.uint16), "16bit_high_pedestal": (4000.0, 61000.0, np.uint16)}


def counts(im, setting):
    gain, pedestal, dtype = CAMERA_SETTINGS[setting]
    return np.clip(np.rint(pedestal + gain * np.asarray(im, np.float64)), 0, np.iinfo(dtype).max).astype(dtype)


def direct_correlator_cases():
    """test_piv_correlation_gpu.CASES at its smallest image of each window size: (70, 90) / 16, (100, 75) / 32, (130, 170) / 64."""
    import test_piv_correlation_gpu as tg
    picked = [c for c in tg.CASES if (c[0], c[3]) in ((16, (70, 90)), (32, (100, 75)), (64, (130, 170)))]
    assert len(picked) == 3
    return picked


@functools.lru_cache(maxsize=None)
def direct_correlator_counts(index, setting):
    """(counts 1, counts 2, win, step, R, offsets or None, the f64 model on the counts as f64 with planes)."""
    import test_piv_correlation_gpu as tg
    from photon_amd import piv_correlation as pc
    win, R, step, shape, shift, with_off = direct_correlator_cases()[index]
    im1, im2 = tg.particle_pair(shape, shift, seed=win * 100 + R + step)
    off = np.random.default_rng(R).integers(-3, 4, size=(*pc.grid_shape(shape, win, step), 2)).astype(np.int32) if with_off else None
    c1, c2 = counts(im1, setting), counts(im2, setting)
    want = pc.correlate_model(c1.astype(np.float64), c2.astype(np.float64), win, step, R, offset=off, planes=True)
    return c1, c2, win, step, R, off, want


# ---- camera counts: the other measurement drivers, each with its module's smallest model-test images -----------------------------
def gain_of(setting):
    return CAMERA_SETTINGS[setting][0]


def pedestal_of(setting):
    return CAMERA_SETTINGS[setting][1]


def uniform_rms(vectors, shift):
    """RMS of |measured - the uniform shift| over the interior nodes (the outer ring left out, as piv_deformation_cases.interior_rms)."""
    e = np.asarray(vectors, np.float64)[1:-1, 1:-1, :2] - np.asarray(shift, np.float64)
    return float(np.sqrt(np.nanmean((e * e).sum(axis=-1))))


PAIR_SHAPE, PAIR_SHIFT, PAIR_WIN, PAIR_STEP, PAIR_RADIUS = (100, 75), (-4.6, 2.2), 32, 16, 8       # test_piv_correlation_gpu.CASES[4]
DEFORM = dict(win=PAIR_WIN, step=PAIR_STEP, radius=PAIR_RADIUS, iterations=2)
PHASE_MULTIGRID = dict(schedule=((32, 16), (16, 8)), iterations=(1, 1), method="phase")


@functools.lru_cache(maxsize=None)
def pair_counts(setting):
    """The (100, 75) / win 32 pair of the direct correlator's cases, as counts (None: unscaled f32)."""
    import test_piv_correlation_gpu as tg
    im1, im2 = tg.particle_pair(PAIR_SHAPE, PAIR_SHIFT, seed=32 * 100 + 8 + 16)
    return (im1, im2) if setting is None else (counts(im1, setting), counts(im2, setting))


@functools.lru_cache(maxsize=None)
def deform_model(setting):
    from photon_amd import piv_deformation as pd
    c1, c2 = pair_counts(setting)
    return pd.correlate_deform_model(c1.astype(np.float64), c2.astype(np.float64), **DEFORM)[:2]


@functools.lru_cache(maxsize=None)
def phase_multigrid_model(setting):
    from photon_amd import piv_multigrid as pm
    c1, c2 = pair_counts(setting)
    return pm.correlate_multigrid_model(c1.astype(np.float64), c2.astype(np.float64), **PHASE_MULTIGRID)[:2]


@functools.lru_cache(maxsize=None)
def ensemble_counts(setting):
    """piv_ensemble_cases.PARTICLE_STACKS[0] ((64, 100), win 16, with offsets) as counts: (stack 1, stack 2, case, offsets, the
    f64 model with planes)."""
    import piv_ensemble_cases as ec
    from photon_amd import piv_correlation as pc
    from photon_amd import piv_ensemble as pe
    case = ec.PARTICLE_STACKS[0]
    win, R, step, shape, shift, with_off = case
    s1, s2 = ec.particle_stack(shape, shift, ec.PARTICLE_PAIRS, seed=win + R)
    if setting is not None:
        s1, s2 = counts(s1, setting), counts(s2, setting)
    off = np.random.default_rng(R).integers(-3, 4, size=pc.grid_shape(shape, win, step) + (2,)).astype(np.int32) if with_off else None
    want = pe.correlate_ensemble_model(s1.astype(np.float64), s2.astype(np.float64), win, step, R, offset=off, planes=True)
    return s1, s2, case, off, want


UNCERTAINTY_CASE = ((64, 64), 16, 8, 2)                                  # piv_uncertainty_cases.GRIDS[0] at the default reach


def window_energies(a, b, win, step):
    """piv_uncertainty_cases.energies on any pair: sqrt(sum A^2 sum B^2) per window, the scale of C0 and C1."""
    a, b = (np.lib.stride_tricks.sliding_window_view(np.asarray(im, np.float64), (win, win))[::step, ::step] for im in (a, b))
    A, B = (x - x.mean(axis=(-2, -1), keepdims=True) for x in (a, b))
    return np.sqrt((A * A).sum(axis=(-2, -1)) * (B * B).sum(axis=(-2, -1)))


@functools.lru_cache(maxsize=None)
def uncertainty_counts(setting):
    """piv_uncertainty_cases.matched_pair((64, 64)) as counts: (c1, c2, the model's (sigma, flags, stats, T))."""
    import piv_uncertainty_cases as uc
    from photon_amd import piv_uncertainty as pu
    shape, win, step, reach = UNCERTAINTY_CASE
    c1, c2 = uc.matched_pair(shape)
    if setting is not None:
        c1, c2 = counts(c1, setting), counts(c2, setting)
    return c1, c2, pu.uncertainty_model(c1.astype(np.float64), c2.astype(np.float64), win, step, reach)


FLOW_SHAPE, FLOW_SHIFT = (64, 80), (0.6, -0.4)
FLOW = dict(win=32, step=16, alpha2=5.0, warps=2, iterations=20)


@functools.lru_cache(maxsize=None)
def flow_counts(setting):
    """A (64, 80) particle pair as counts, the grid predictor (one model iteration of correlate_deform on it, f32) and the f64
    flow model from that predictor.  optical_flow_cases has no small image pair of its own: its SHAPES below (130, 97) serve
    the terms and sweeps on random fields, and its analytic pairs are 256 x 256, whose f64 models take seconds per setting.  A
    particle pair is what the 3e-5 px bar was derived for (test_the_device_follows_the_model), and (64, 80) is the smallest
    size with more than one window a side at win 32."""
    import test_piv_correlation_gpu as tg
    from photon_amd import optical_flow as of
    from photon_amd import piv_deformation as pd
    im1, im2 = tg.particle_pair(FLOW_SHAPE, FLOW_SHIFT, seed=77, per_px=0.03)
    if setting is not None:
        im1, im2 = counts(im1, setting), counts(im2, setting)
    f1, f2 = im1.astype(np.float64), im2.astype(np.float64)
    grid = pd.correlate_deform_model(f1, f2, FLOW["win"], FLOW["step"], iterations=1)[0][..., :2].astype(np.float32)
    return im1, im2, grid, of.optical_flow_model(f1, f2, grid, **FLOW)


DOTS_THRESHOLD, DOTS_BACKGROUND = 0.25, 0.0                              # of the unscaled image, as test_dot_tracking_gpu fits it


@functools.lru_cache(maxsize=None)
def dots_counts(setting):
    """dot_tracking_cases.detection_image((64, 64)) without its NaN pixels (an integer frame has none) as counts, with the
    parameters that carry intensity: background -> gain background + pedestal, and the relative threshold that cuts the
    same intensity, (pedestal + gain threshold max) / (pedestal + gain max).  Returns (frame, threshold, background, the
    model's peaks, the f64 model's result)."""
    import dot_tracking_cases as cs
    from photon_amd import dot_tracking as dt
    im = np.nan_to_num(cs.detection_image((64, 64), seed=128)).astype(np.float32)
    top = float(im.max())
    if setting is None:
        frame, thr, bg = im, DOTS_THRESHOLD, DOTS_BACKGROUND
    else:
        g, p = gain_of(setting), pedestal_of(setting)
        frame = counts(im, setting)
        thr, bg = (p + g * DOTS_THRESHOLD * top) / float(frame.max()), g * DOTS_BACKGROUND + p
    f = frame.astype(np.float64)
    peaks, total = dt.detect_model(f, thr, dt.image_max_model(f))
    return frame, thr, bg, peaks, dt.track_dots_model(f, f, thr, relative=True, background=bg)


PREPROCESS = dict(radius=3, floor=0.05)


@functools.lru_cache(maxsize=None)
def preprocess_counts(setting):
    """piv_preprocess_cases.particle_frames((70, 90), 3) as counts, the floor scaled with the gain: (frames, floor, the f32
    model held bit for bit, the f64 model)."""
    import piv_preprocess_cases as pcs
    from photon_amd import piv_preprocess as pp
    frames = np.array(pcs.particle_frames((70, 90), 3, seed=3))
    floor = PREPROCESS["floor"]
    if setting is not None:
        frames, floor = counts(frames, setting), floor * gain_of(setting)
    f32 = frames.astype(np.float32)
    bg = pp.background_model(f32, pp.MODE_MIN)
    return (frames, floor, pp.preprocess_model_f32(f32, bg, PREPROCESS["radius"], floor),
            pp.preprocess_model(f32.astype(np.float64), bg.astype(np.float64), PREPROCESS["radius"], floor))


# ---- exact scale: im 2^k as f32 ---------------------------------------------------------------------------------------------------
SCALE_EXPONENTS = (8, 12)
PHASE_SCALE_CASES = (0, 4, 7)                                            # piv_phase_cases.DEVICE_CASES: win 16, 32 and 64, phase mode with filter


@functools.lru_cache(maxsize=None)
def phase_scaled(index, k):
    """piv_phase_cases.device_case(index) with both frames times 2^k: (im1, im2, offsets, the f32 model on the scaled frames)."""
    import piv_phase_cases as phc
    from photon_amd import piv_phase as pp
    win, R, step, shape, _, with_off, mode, sigma, diameter = phc.DEVICE_CASES[index]
    im1, im2, off, _ = phc.device_case(index)
    s = np.float32(2.0 ** k)
    a, b = im1 * s, im2 * s
    return a, b, off, pp.correlate_phase_model_f32(a, b, win, step, R, offset=off, mode=mode, window_sigma=sigma, diameter=diameter, planes=True)


@functools.lru_cache(maxsize=None)
def preprocess_scaled(k):
    import piv_preprocess_cases as pcs
    from photon_amd import piv_preprocess as pp
    s = np.float32(2.0 ** k)
    frames = np.array(pcs.particle_frames((70, 90), 3, seed=3)) * s
    floor = float(np.float32(PREPROCESS["floor"]) * s)
    bg = pp.background_model(frames, pp.MODE_MIN)
    return frames, bg, floor, pp.preprocess_model_f32(frames, bg, PREPROCESS["radius"], floor)


@functools.lru_cache(maxsize=None)
def terms_scaled(k):
    """optical_flow_cases.random_pair((37, 53)) times 2^k with alpha2 4^k at a fixed gain: (w1, w2, u0, gain, alpha2, the f32
    terms model)."""
    import optical_flow_cases as oc
    from photon_amd import optical_flow as of
    w1, w2, u0 = oc.random_pair((37, 53), 21)
    gain = float(np.float32(1.0 / max(float(w1.std()), 1.0)))
    s = np.float32(2.0 ** k)
    a, b, alpha2 = w1 * s, w2 * s, oc.ALPHA2 * 4.0 ** k
    return a, b, u0, gain, alpha2, of.terms_model(a, b, u0, gain, alpha2)


SCALED_SWEEPS = 9                                                        # one more than the default 8 a launch: two launches, through d_tmp


@functools.lru_cache(maxsize=None)
def sweeps_scaled(k):
    """SCALED_SWEEPS Jacobi sweeps of the f32 model on terms_scaled(k)'s terms from its field u0."""
    from photon_amd import optical_flow as of
    _, _, u0, _, _, terms = terms_scaled(k)
    return of.iterate_model(terms, u0, SCALED_SWEEPS)
