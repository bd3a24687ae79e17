"""The sequence of C calls behind every driver of photon_amd/library.py, held against tests/driver_calls.json: the log that
driver_call_log.py --write took at the commit the file names, before the window-correlation drivers were restructured
(one grid-call helper, one bound correlator, one deformation chain).  A driver that drops, adds, reorders or re-arguments a
call differs from it literally: the size query's NULLs, every win, step, radius and min_valid, which optional outputs are
asked for and which calls get the stream."""
import pytest

import driver_call_log as dl

gpu = pytest.mark.gpu

# the drivers of the window-correlation family, and the entry points their rows have to reach between them
DRIVERS = ("correlate", "correlate_ensemble", "correlate_deform", "correlate_multigrid", "correlation_predictor",
           "displacement_uncertainty", "optical_flow")
ENTRY_POINTS = ("photon_piv_correlate", "photon_piv_correlate_phase", "photon_piv_correlate_masked", "photon_piv_correlate_weighted",
                "photon_piv_correlate_ensemble", "photon_piv_uncertainty", "photon_piv_regrid", "photon_piv_validate", "photon_piv_deform",
                "photon_piv_bspline_coefficients", "photon_piv_deform_dense", "photon_optflow_terms", "photon_optflow_iterate")


@gpu
@pytest.mark.parametrize("name", list(dl.rows()))
def test_the_driver_makes_the_recorded_calls(photon, name):
    want = dl.read_log()["rows"][name]["calls"]
    lib = photon.lib
    got, _ = dl.log_of(photon, dl.rows()[name])
    assert photon.lib is lib
    assert len(got) == len(want), (name, [c[0] for c in got], [c[0] for c in want])
    differ = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not differ, f"{name}: calls (index, made, recorded) differ from the log: {differ[:4]}"


def test_the_log_has_a_row_for_every_driver_and_reaches_every_entry_point():
    log = dl.read_log()
    assert log["commit"] == "728155c"
    assert set(log["rows"]) == set(dl.rows()), "driver_calls.json and driver_call_log.rows() name different rows"
    for name, row in dl.rows().items():
        assert log["rows"][name]["driver"] == row.driver and log["rows"][name]["calls"], name
    drivers = {row["driver"] for row in log["rows"].values()}
    assert not [d for d in DRIVERS if d not in drivers]
    reached = {call[0] for row in log["rows"].values() for call in row["calls"]}
    assert not [e for e in ENTRY_POINTS if e not in reached]
    # the query of a grid call passes no offsets, no outputs and no stream, and asks for rows and cols
    queries = [c for row in log["rows"].values() for c in row["calls"] if c[0] == "photon_piv_correlate" and c[-3:-1] == ["out", "out"]]
    assert queries and all(c[8:] == ["null"] * 4 + ["out", "out", "null"] for c in queries)


def test_the_recorder_logs_values_and_kinds_and_puts_the_library_back():
    import ctypes

    class Lib:
        @staticmethod
        def photon_entry(*args):
            return 0

    class Photon:
        lib = Lib()

    p = Photon()
    n = ctypes.c_int(0)
    with dl.recorded(p) as log:
        assert p.lib.photon_entry(ctypes.c_void_p(16), None, ctypes.c_void_p(0), 3, 0.25, True, ctypes.byref(n)) == 0
        with pytest.raises(AttributeError):
            p.lib.photon_missing
    assert p.lib is Photon.lib
    assert log == [["photon_entry", "ptr", "null", "null", 3, 0.25, 1, "out"]]
