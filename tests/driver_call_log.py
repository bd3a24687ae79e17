"""The C calls a driver of photon_amd/library.py makes, in order, as plain data: what tests/test_driver_calls_gpu.py holds
against tests/driver_calls.json.

  recorded(photon)    with recorded(photon) as log: photon.lib is a proxy for the duration of the block; every entry point
                      reached appends [name, argument, ...] to log.  Ints and floats are logged by value, a c_void_p (or the
                      None that stands for NULL) as "null" or "ptr", a byref as "out".
  rows()              name -> Row: the 14 PIPELINES of tests/test_streams_gpu.py, the rows of driver_input_cases.rows(), and
                      the branches of the window-correlation drivers that those miss, at the same shapes.
  --write COMMIT [PATH]   run every row on the GPU and write the log (default: tests/driver_calls.json) with the name of the
                      commit whose library.py made the calls.  The committed file was written before the drivers were
                      restructured; it is rewritten only by a change that moves a C call on purpose.

Importing this module needs no GPU.
"""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LOG_PATH = os.path.join(HERE, "driver_calls.json")
_BYREF = type(ctypes.byref(ctypes.c_int(0)))


def plain(arg):
    """One argument as the log holds it."""
    if arg is None:
        return "null"
    if isinstance(arg, ctypes.c_void_p):
        return "ptr" if arg.value else "null"
    if isinstance(arg, _BYREF):
        return "out"
    if isinstance(arg, (bool, np.bool_)):
        return int(arg)
    if isinstance(arg, (int, np.integer)):
        return int(arg)
    if isinstance(arg, (float, np.floating)):
        return float(arg)
    if isinstance(arg, bytes):
        return arg.decode()
    return type(arg).__name__            # a struct by pointer, a host buffer: its type


class _Proxy:
    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        f = getattr(self._lib, name)      # AttributeError for a missing symbol, as the library raises it

        def call(*args):
            self._log.append([name, *(plain(a) for a in args)])
            return f(*args)
        return call


@contextlib.contextmanager
def recorded(photon):
    log, lib = [], photon.lib
    photon.lib = _Proxy(lib, log)
    try:
        yield log
    finally:
        photon.lib = lib


# ---- the rows ------------------------------------------------------------------------------------------------------------------
class Row:
    """driver: the public method the row calls; make_inputs() -> {key: numpy}; run(photon, {key: device tensor})."""
    def __init__(self, driver, make_inputs, run):
        self.driver, self.make_inputs, self.run = driver, make_inputs, run


def _more_rows():
    import driver_input_cases as cases
    import stream_cases as sc
    import test_streams_gpu as ts
    pair = ts._pair_inputs

    def two_masks():
        m2 = np.zeros(sc.ODD, np.uint8)
        m2[10:40, 80:120] = 1
        return pair(mask=ts._mask(), mask2=m2)

    def series():
        return dict(frames1=np.stack([sc.pair(sc.SMALL, seed=10 + k)[k & 1] for k in range(4)]))

    ensemble = ts.PIPELINES["correlate_ensemble"][1]
    grid = dict(win=32, step=16, radius=8)
    out = {}
    branches = {
        "mask": (lambda: pair(mask=ts._mask()), lambda t: dict(mask=t["mask"])),
        "two_masks": (two_masks, lambda t: dict(mask=(t["mask"], t["mask2"]))),
        "gaussian": (pair, lambda t: dict(weighting="gaussian")),
        "table": (lambda: pair(weighting=cases._window_table()), lambda t: dict(weighting=t["weighting"])),
        "phase": (pair, lambda t: dict(method="phase", radius=None)),
    }
    for branch, (make, more) in branches.items():
        for passes in (1, 2):
            out[f"correlate_{branch}_passes{passes}"] = Row(
                "correlate", make, lambda p, t, more=more, passes=passes: p.correlate(t["im1"], t["im2"], **{**grid, "passes": passes, **more(t)}))
    out["correlate_ensemble_two_passes"] = Row(
        "correlate_ensemble", ensemble, lambda p, t: p.correlate_ensemble(t["frames1"], t["frames2"], win=16, step=8, radius=4, passes=2))
    out["correlate_ensemble_series"] = Row("correlate_ensemble", series, lambda p, t: p.correlate_ensemble(t["frames1"], win=16, step=8, radius=4))
    for fill in (False, True):
        out[f"correlate_deform_mask_fill_{fill}"] = Row(
            "correlate_deform", lambda: pair(mask=ts._mask()),
            lambda p, t, fill=fill: p.correlate_deform(t["im1"], t["im2"], **grid, iterations=2, mask=t["mask"], fill_masked=fill))
    out["correlate_multigrid_no_iteration_on_level_0"] = Row(
        "correlate_multigrid", pair, lambda p, t: p.correlate_multigrid(t["im1"], t["im2"], schedule=((32, 16), (16, 8)), iterations=(0, 1), radius=8))
    out["correlation_predictor_mask_filled"] = Row(
        "correlation_predictor", lambda: pair(mask=ts._mask()),
        lambda p, t: p.correlation_predictor(t["im1"], t["im2"], **grid, mask=t["mask"], fill_masked=True))
    out["correlation_predictor_gaussian"] = Row(
        "correlation_predictor", pair, lambda p, t: p.correlation_predictor(t["im1"], t["im2"], **grid, weighting=("gaussian", 7.0)))
    out["correlation_predictor_phase"] = Row(
        "correlation_predictor", pair, lambda p, t: p.correlation_predictor(t["im1"], t["im2"], win=32, step=16, method="phase"))
    return out


def rows():
    import driver_input_cases as cases
    out = {name: Row(row.method, row.make_inputs, row.run) for name, row in cases.rows().items()}    # the 14 pipelines among them
    more = _more_rows()
    assert not set(out) & set(more)
    out.update(more)
    return out


def device_inputs(row):
    import torch
    return {k: torch.from_numpy(np.array(a, order="C")).cuda() for k, a in row.make_inputs().items()}


def log_of(photon, row):
    """(the calls of one run of the row on device tensors, the driver's result).  The current stream is a side stream, so that
    the log tells a call that was handed the stream ("ptr") from one that was not ("null")."""
    import torch
    tensors = device_inputs(row)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()), recorded(photon) as log:
        result = row.run(photon, tensors)
        torch.cuda.current_stream().synchronize()
    return log, result


def read_log(path=LOG_PATH):
    with open(path, encoding="utf-8") as f:
        return json.load(f)


def main(argv):
    if len(argv) < 2 or argv[0] != "--write":
        raise SystemExit("usage: driver_call_log.py --write COMMIT [PATH]")
    commit, path = argv[1], argv[2] if len(argv) > 2 else LOG_PATH
    root = os.path.dirname(HERE)
    for p in (root, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch  # noqa: F401  -- before the library: one HIP runtime per process
    from photon_amd.library import PhotonLibrary
    photon = PhotonLibrary()
    photon.set_device(0)
    out = {"commit": commit, "rows": {}}
    for name, row in rows().items():
        log, _ = log_of(photon, row)
        out["rows"][name] = {"driver": row.driver, "calls": log}
        print(f"{name}: {len(log)} calls")
    with open(path, "w", encoding="utf-8") as f:
        f.write("{\n" + f' "commit": {json.dumps(commit)},\n "rows": {{\n')
        f.write(",\n".join(f'  {json.dumps(name)}: {{"driver": {json.dumps(r["driver"])}, "calls": [\n'
                           + ",\n".join("   " + json.dumps(c) for c in r["calls"]) + "]}" for name, r in out["rows"].items()))
        f.write("\n }\n}\n")
    assert read_log(path) == out


if __name__ == "__main__":
    main(sys.argv[1:])
