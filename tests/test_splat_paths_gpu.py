"""Every route of the sensor stage (device_optics.hpp: erf_splat_wave and its three fall-backs to erf_splat_lane,
bilinear_splat_wave on both LDS layouts; photon_sensor.hip: the six sensor_kernel instantiations, with and without the
moments) per pixel against the oracle, on the scene families of tests/splat_families.py whose images straddle the sensor's
edges and corners.  Bars (tests/test_splat_paths.py shows the oracle meets them against itself across summation orders):
rays_on_sensor and sensor_taps equal as integers; ray dumps bit-equal, NaN for exactly the same rays; erf and isolated
4-pixel images bit-equal at every pixel; overlapping 4-pixel images lit in the same pixels, within one f32 ulp everywhere,
at most 0.5 % of the lit pixels differing at all.  The splat-path counters (enum SplatSlot, a -DPHOTON_PATH_STATS=1 build,
run in a child process: tests/_splat_paths_worker.py) prove that the families reach the branches they were built for."""
import json
import os
import pickle
import signal
import subprocess
import sys

import pytest

import splat_families as sf
from _splat_paths_worker import run_families
from photon_amd import build as _build
from photon_amd.path_stats import PATH_STATS_FLAGS, SPLAT_SLOTS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANT_DIR = os.path.join(_build.ROOT, "build", "variants")
CHILD_TIMEOUT = 300

# Slots that no family can reach, and why.  They must count zero.
UNREACHABLE = {}


@pytest.fixture(scope="module")
def want(oracle, tmp_path_factory):
    """(families, {name: the oracle's render with every ray dumped}, working directory)"""
    d = str(tmp_path_factory.mktemp("splat_paths_gpu"))
    fams = sf.build_families(oracle, d)
    return fams, {f.name: sf.oracle_render(oracle, f, d) for f in fams}, d


def test_default_library_meets_the_bars_on_every_family(photon, want):
    fams, out, d = want
    bad, _ = run_families(photon, fams, out, d)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:30])


@pytest.fixture(scope="module")
def pathstats_lib():
    """The path-stats build the sampler-path tests use (same file, same objects: whoever comes second only links)."""
    os.makedirs(VARIANT_DIR, exist_ok=True)
    return _build.build_library(verbose=False, extra_flags=PATH_STATS_FLAGS, out_path=os.path.join(VARIANT_DIR, "lib_test_pathstats.so"))


_child_died = []


def _run_child(lib, want, tmp_path, name):
    """One child, under a time limit; after one that died by a signal or ran out of time no further child starts."""
    if _child_died:
        pytest.fail(f"not started: an earlier child ({_child_died[0]}) died")
    fams, out, _ = want
    pkl, res = str(tmp_path / "families.pkl"), str(tmp_path / f"{name}.json")
    with open(pkl, "wb") as f:
        pickle.dump((fams, out), f)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_splat_paths_worker.py"), lib, pkl, str(tmp_path), res],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _child_died.append(name)
        pytest.fail(f"{name}: the child ran out of time ({CHILD_TIMEOUT} s)\n{e.stdout}\n{e.stderr}")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_died.append(name)
        sig = signal.Signals(-r.returncode).name if r.returncode < 0 else r.returncode
        pytest.fail(f"{name}: the child died ({sig})\n{r.stdout}\n{r.stderr}")
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    print(r.stdout.strip())
    with open(res) as f:
        got = json.load(f)
    assert not got["mismatches"], f"{name}: {len(got['mismatches'])} mismatches:\n" + "\n".join(got["mismatches"][:30])
    return got["counts"]


def _check_identities(fams, counts):
    """What the counters must satisfy by construction, per family: every wave with a live erf ray went one of the two ways,
    and a fall-back had a reason; every tile with a contributing ray was summed by one of the two loops; every 4-pixel wave
    went one of the two ways; every ray on the sensor of a 4-pixel family has four taps, landed or dropped."""
    for f in fams:
        t = counts[f.name]
        assert t["E_COOP"] + t["E_FALLBACK"] == t["E_WAVES"], f.name
        assert t["E_FALLBACK"] <= t["E_FB_WIDE"] + t["E_FB_TILES"] + t["E_FB_RADIUS"], f.name
        assert t["E_TILES_SAME"] + t["E_TILES_MIXED"] == t["E_TILES"], f.name
        assert t["E_TILES"] >= t["E_COOP"], f.name                      # (a ray on the sensor renders the pixel it hits, at least)
        assert t["T_COOP"] + t["T_LANE_ROUTE"] == t["T_WAVES"], f.name
        assert t["T_TAPS_WRAPPED"] <= t["T_TAPS_LANDED"], f.name
        kernels = [k for k in SPLAT_SLOTS if k.startswith("K_")]
        assert sum(t[k] > 0 for k in kernels) == 1, (f.name, {k: t[k] for k in kernels})   # one trace, one instantiation
        if f.erf:
            assert t["T_WAVES"] == 0 and t["T_TAPS_LANDED"] + t["T_TAPS_DROPPED"] == 0, f.name
            assert t["E_SHARED_X_LANES"] + t["E_BOTH_X_LANES"] == t["E_SHARED_Y_LANES"] + t["E_BOTH_Y_LANES"], f.name
        else:
            assert t["E_WAVES"] == 0, f.name
            assert t["T_TAPS_LANDED"] + t["T_TAPS_DROPPED"] == 4 * t["rays_on_sensor"], f.name


def _print_table(title, fams, counts, tot):
    print(f"\n{title}\n{'slot':24s}{'all families':>14s}   families that count it")
    for k in SPLAT_SLOTS:
        who = [f.name for f in fams if counts[f.name][k] > 0]
        note = f"unreachable ({UNREACHABLE[k]})" if k in UNREACHABLE else f"{len(who)}: " + " ".join(who[:4]) + (" ..." if len(who) > 4 else "")
        print(f"{k:24s}{tot[k]:14d}   {note}")


def test_every_splat_path_is_taken(want, pathstats_lib, tmp_path):
    fams = want[0]
    counts = _run_child(pathstats_lib, want, tmp_path, "pathstats")
    _check_identities(fams, counts)
    tot = {k: sum(counts[f.name][k] for f in fams) for k in SPLAT_SLOTS}
    _print_table("splat-path counters, one default trace per family (sum over the families)", fams, counts, tot)
    for k, why in UNREACHABLE.items():
        assert tot[k] == 0, f"{k} counted although listed unreachable ({why})"
    missing = [k for k in SPLAT_SLOTS if tot[k] == 0 and k not in UNREACHABLE]
    assert not missing, "slots no family reached: " + " ".join(missing)
    short = [f"{f.name}: {k}" for f in fams for k in f.slots if counts[f.name][k] == 0]
    assert not short, "families that miss a slot they name:\n" + "\n".join(short)
