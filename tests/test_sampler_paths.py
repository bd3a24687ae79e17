"""CPU side of the sampler-path tests (tests/test_sampler_paths_gpu.py): the counter enum's Python mirror, the debug and
switch-variant builds, and the ray families in the oracle."""
import os
import shutil
import subprocess

import pytest

import sampler_families as sf
from photon_amd import build as _build
from photon_amd import path_stats


def test_python_mirror_matches_the_header():
    assert path_stats.header_slots() == path_stats.SLOTS


def test_families_march_in_the_oracle(oracle):
    fams, out = sf.oracle_results(oracle)
    names = [f.name for f in fams]
    assert len(set(names)) == len(names)
    for f in fams:
        assert len(f.pos) == len(f.dir) == len(f.enters) and f.slots
        for s, _, _ in sf.SAMPLERS:
            for a in sf.ALGORITHMS:
                st = out[f"{f.name}/{s}/{a}/steps"]
                assert (st[f.enters] > 0).all(), f"{f.name} {s}/{a}: rays meant to enter take no step"
                assert (st[~f.enters] == 0).all(), f"{f.name} {s}/{a}: rays meant to miss take steps"
    assert any(len(f.pos) % sf.W for f in fams), "no family ends on a partial wave"
    assert any((~f.enters).any() for f in fams), "no family has rays that miss"


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


@pytest.mark.skipif(_hipcc() is None or shutil.which("nm") is None, reason="needs hipcc and nm")
@pytest.mark.parametrize("name", ["pathstats", "VA", "VB"])
def test_debug_and_variant_builds_compile(name, tmp_path):
    from test_sampler_paths_gpu import VARIANTS
    out = _build.build_library(verbose=False, extra_flags=VARIANTS[name], out_path=str(tmp_path / f"lib_{name}.so"))
    syms = subprocess.run(["nm", "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert " photon_debug_path_stats" in syms
    assert os.path.getsize(out) > 0
