"""Every route of the wave-cooperative samplers (device_volume_coop.hpp) and every tuning switch, bit-exact against the oracle,
with the sampler-path counters (enum PathSlot, a -DPHOTON_PATH_STATS=1 build) proving that the families of
tests/sampler_families.py reach the branches they were built for.  The matrix: every family through the plain grid
(positions, directions, iteration counts) and the queued launch in 1, 3 and 7 pieces (positions and directions: that launch
reports no iteration counts), for trilinear 8-bit and exact weights and tricubic, Euler and RK4.  Debug and switch-variant
builds run in child processes (tests/_sampler_paths_worker.py), one at a time; they also march the adversarial fuzz rays
and render a BOS and a PIV scene through the volume (sensor moments against the oracle's ray dumps)."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import sampler_families as sf
from _sampler_paths_worker import run_matrix
from photon_amd import build as _build
from photon_amd.path_stats import PATH_STATS_FLAGS, SLOTS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANT_DIR = os.path.join(_build.ROOT, "build", "variants")
VARIANTS = {
    "pathstats": PATH_STATS_FLAGS,
    "VA": PATH_STATS_FLAGS + ("-DPHOTON_BRICK_PASSES=0", "-DPHOTON_CUBIC_TILE_LAYERS=4", "-DPHOTON_LINEAR_TILES=1",
                              "-DPHOTON_LINEAR_TILE_LAYERS=4", "-DPHOTON_DPP_SLABS=1"),
    "VB": PATH_STATS_FLAGS + ("-DPHOTON_BRICK_PASSES=1", "-DPHOTON_CUBIC_TILE_LAYERS=8", "-DPHOTON_LINEAR_TILE_LAYERS=8",
                              "-DPHOTON_TILE_RETRY_MASK=0", "-DPHOTON_SPINS_IN_LDS=0", "-DPHOTON_DPP_SLABS=4", "-DPHOTON_BRICK_PITCH=8",
                              "-DPHOTON_PRIO_BASE=0", "-DPHOTON_PRIO_TAPS_DPP=0", "-DPHOTON_PRIO_BRICK=0"),
}

# Slots that cannot be taken with the default switches, and why; (slot, algorithm or None for both).  Every other slot of a
# sampler must count for each of its weight modes and algorithms.
# Keys (slot, sampler or None for every sampler, algorithm or None for both).
_EXACT_NOT_LOW = ("exact weights: each lerp is fmaf(t, b - a, a) with t < 1 -- or t rounded up to 1 on two equal clamped "
                  "texels -- and lies between its corners, so no blend falls below data_min")
UNREACHABLE = {
    ("C_SPIN_CAP", None, None): "kSpinMax (2^20 spins) is out of reach at test sizes",
    ("L_SPIN_CAP", None, None): "kSpinMax (2^20 spins) is out of reach at test sizes",
    ("C_SPIN_OUTSIDE", None, 1): "the tricubic Euler march does not test its first lookup (only the linear branch guards, .h:821)",
    ("L_LOW", "L0", None): _EXACT_NOT_LOW,
    ("L_REPAIR_LANES", "L0", None): _EXACT_NOT_LOW,
    ("L_KEEP_PREV_LANES", "L0", None): _EXACT_NOT_LOW,
}
CHILD_TIMEOUT = 300


def _unreachable(k, s, a):
    return any((k, ss, aa) in UNREACHABLE for ss in (s, None) for aa in (a, None))


@pytest.fixture(scope="module")
def want(oracle):
    """(families, the oracle's results of the families)"""
    fams, out = sf.oracle_results(oracle)
    for f in fams:                                       # the families do what they say in the oracle too
        for s, _, _ in sf.SAMPLERS:
            for a in sf.ALGORITHMS:
                st = out[f"{f.name}/{s}/{a}/steps"]
                assert (st[f.enters] > 0).all() and (st[~f.enters] == 0).all(), (f.name, s, a)
    return fams, out


@pytest.fixture(scope="module")
def child_inputs(want, oracle, tmp_path_factory):
    """(oracle.npz, volume.nrrd): what the children compare with -- families, fuzz rays, render records -- computed once."""
    d = tmp_path_factory.mktemp("sampler_paths")
    nrrd = sf.render_volume(str(d / "render_40.nrrd"))
    out = dict(want[1])
    out.update(sf.oracle_adversarial(oracle))
    out.update(sf.oracle_render_records(oracle, nrrd, str(d)))
    path = str(d / "oracle.npz")
    np.savez(path, **out)
    return path, nrrd


def test_default_library_bit_exact_on_every_family(photon, want):
    bad, _ = run_matrix(photon, want[1])
    assert not bad, "\n".join(bad[:20])


@pytest.fixture(scope="session")
def variant_libs():
    """The path-stats build and the switch variants, compiled one after another (each build runs its units in parallel)."""
    os.makedirs(VARIANT_DIR, exist_ok=True)
    return {name: _build.build_library(verbose=False, extra_flags=flags, out_path=os.path.join(VARIANT_DIR, f"lib_test_{name}.so"))
            for name, flags in VARIANTS.items()}


_child_died = []


def _run_child(lib, inputs, tmp_path, name):
    """One child at a time, under a time limit; after one that died by a signal or ran out of time no further child starts."""
    if _child_died:
        pytest.fail(f"not started: an earlier child ({_child_died[0]}) died")
    out = str(tmp_path / f"{name}.json")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_sampler_paths_worker.py"), lib, inputs[0], inputs[1], out],
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
    with open(out) as f:
        res = json.load(f)
    assert not res["mismatches"], f"{name}:\n" + "\n".join(res["mismatches"][:20])
    return res["counts"]


def _check_identities(counts):
    """What the counters must satisfy by construction, per family and combination: every coherent tricubic sample took one of
    its four routes; every brick pass fetched or reused; every trilinear sample that went to the bricks came from one of
    three routes, and every coherent one from the first test, B's test or a fetch that reached every lane; and every
    incoherent sampling lane was served by one brick or by the gather."""
    for name, per in counts.items():
        for combo, t in per.items():
            w = f"{name} {combo}"
            assert t["C_COHERENT"] == t["C_HIT_CELL"] + t["C_CELL_IN_TILE"] + t["C_FETCH_UP"] + t["C_FETCH_DOWN"], w
            assert t["L_INCOHERENT"] == t["L_NO_FREE_TILE"] + t["L_OUT_OF_REACH"] + t["L_TILES_SKIPPED"], w
            assert t["L_COHERENT"] == t["L_HIT_A"] + t["L_HIT_B"] + t["L_FETCH"] - t["L_FETCH_TWO"] - t["L_OUT_OF_REACH"], w
            assert t["L_REPAIR_LANES"] + t["L_KEEP_PREV_LANES"] >= t["L_LOW"], w
            for p in ("C_", "L_"):
                assert t[p + "BRICK_PASS"] == t[p + "BRICK_FETCH"] + t[p + "BRICK_REUSED"], w
                assert t[p + "BRICK_LANES"] + t[p + "GATHER_LANES"] == t[p + "INCOHERENT_LANES"], w


def _totals(counts, adversarial=False):
    """{sampler/algorithm: {slot: sum over the families (adversarial: over the seeds of the fuzz)}}"""
    tot = {}
    for name, per in counts.items():
        if name.startswith("adv") != adversarial:
            continue
        for combo, c in per.items():
            t = tot.setdefault(combo, dict.fromkeys(SLOTS, 0))
            for k, v in c.items():
                t[k] += v
    return tot


def _print_table(title, tot):
    combos = [f"{s}/{a}" for s, _, _ in sf.SAMPLERS for a in sf.ALGORITHMS]
    print(f"\n{title}\n{'slot':22s}" + "".join(f"{c:>12s}" for c in combos))
    for k in SLOTS:
        why = [f"{ss or 'all'}/{aa or 'both'}: {r}" for (slot, ss, aa), r in UNREACHABLE.items() if slot == k]
        note = f"   unreachable ({why[0]})" if why else ""
        print(f"{k:22s}" + "".join(f"{tot[c][k]:12d}" for c in combos) + note)


def test_every_sampler_path_is_taken(want, child_inputs, variant_libs, tmp_path):
    counts = _run_child(variant_libs["pathstats"], child_inputs, tmp_path, "pathstats")
    _check_identities(counts)
    tot = _totals(counts)
    _print_table("sampler-path counters, default switches (sum over the families)", tot)
    missing = []
    for s, _, _ in sf.SAMPLERS:
        other = "L_" if s == "C" else "C_"
        for a in sf.ALGORITHMS:
            t = tot[f"{s}/{a}"]
            for k in SLOTS:
                if k.startswith(other):
                    assert t[k] == 0, (s, a, k)
                elif _unreachable(k, s, a):
                    assert t[k] == 0, f"{s}/{a}: {k} counted although listed unreachable"
                elif t[k] == 0:
                    missing.append(f"{s}/{a}: {k}")
    assert not missing, "slots no family reached:\n" + "\n".join(missing)
    # each family reaches what it was built for, with every weight mode where the branch can be taken (and one algorithm at
    # least: an Euler trip is one sample, an RK4 trip three, so a family's trips need not meet the retry ticks in both)
    for f in want[0]:
        for s, _, _ in sf.SAMPLERS:
            for k in f.slots["C" if s == "C" else "L"]:
                if _unreachable(k, s, None):
                    continue
                assert any(counts[f.name][f"{s}/{a}"][k] > 0 for a in sf.ALGORITHMS), f"family {f.name}: {k} not reached by {s}"
    # the adversarial fuzz (tests/test_parity_gpu.py) through the same build: the tile, brick and gather paths it is said to mix
    adv = _totals(counts, adversarial=True)
    _print_table("the adversarial fuzz rays of tests/test_parity_gpu.py (sum over its seeds)", adv)
    for combo, t in adv.items():
        p = "C_" if combo.startswith("C/") else "L_"
        assert t[p + "COHERENT"] > 0 and t[p + "BRICK_LANES"] > 0 and t[p + "GATHER_LANES"] > 0, combo


def test_variant_va_gathers_without_bricks(child_inputs, variant_libs, tmp_path):
    """No brick pass: every incoherent sampling lane goes to the gather; one trilinear tile: never tile B."""
    counts = _run_child(variant_libs["VA"], child_inputs, tmp_path, "VA")
    _check_identities(counts)
    tot = _totals(counts)
    _print_table("VA " + " ".join(VARIANTS["VA"][1:]), tot)
    for combo, t in tot.items():
        for p in ("C_", "L_"):
            assert t[p + "BRICK_PASS"] == 0 and t[p + "BRICK_FETCH"] == 0 and t[p + "BRICK_LANES"] == 0, combo
            assert t[p + "GATHER_LANES"] == t[p + "INCOHERENT_LANES"], combo
        assert t["L_TILE_B_LANES"] == 0 and t["L_HIT_B"] == 0 and t["L_FETCH_TO_B"] == 0, combo
        assert t["C_INCOHERENT_LANES"] + t["L_INCOHERENT_LANES"] > 0, combo


def test_variant_vb_retries_every_trip_one_brick_pass(child_inputs, variant_libs, tmp_path):
    """PHOTON_TILE_RETRY_MASK=0: an incoherent wave tries its tiles on every trip; PHOTON_BRICK_PASSES=1: one brick pass per
    incoherent sample."""
    counts = _run_child(variant_libs["VB"], child_inputs, tmp_path, "VB")
    _check_identities(counts)
    tot = _totals(counts)
    _print_table("VB " + " ".join(VARIANTS["VB"][1:]), tot)
    for combo, t in tot.items():
        p = "C_" if combo.startswith("C/") else "L_"
        assert t[p + "BRICK_PASS"] == t[p + "INCOHERENT"] > 0, combo
        assert t[p + "GATHER_LANES"] > 0, combo
        if p == "L_":
            assert t["L_TILES_SKIPPED"] == 0 and t["L_RETRY"] > 0, combo
