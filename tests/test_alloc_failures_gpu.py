"""Every device allocation of a call failed in turn (photon_selftest_fail_alloc): the procedure of tests/alloc_failure_cases.py
on every case of its table.  What a failed call returns, prints and leaves untouched, what a call that only lost its
first attempt computes, that nothing leaks and that the long-lived objects still work afterwards: see that module."""
import json
import os
import subprocess
import sys

import pytest

import alloc_failure_cases as afc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_alloc_failure_worker.py")

# The requests of one clean call where the source states them outright: the pooled scratch of the three solvers
# (photon_density.hip: eight vectors of N, the partial sums, the mask; photon_tomo.hip: r, q, s, the weights, one or two
# data vectors, the partial sums, the counters).
REQUESTS = dict(integrate_gradient=10, tomo_reconstruct=7, tomo_reconstruct_deflections=8)

# A failed request the call survives: the two of the source cull on the volume-free path (its scratch and its list: it only
# saves work, photon_cull.hip, ensure_live_sources), one after the other.  Everywhere else a failed request fails the call.
SWALLOWS_THE_CULL = {name for name in afc.CASES if "without_volume" in name} | {"driver_piv_pair_frame"}


def check_report(name, report, shards=1):
    print(f"{name}: {json.dumps(report)}")
    if name in REQUESTS:
        assert report["A"] == REQUESTS[name], (name, report)
    assert report["A"] <= 64, f"{name}: {report['A']} requests per call: the sweep is no longer a few seconds"
    everything = list(range(1, report["A"] + 1))
    assert report["swallowed"]["first_attempt"] == report["failed"]["first_attempt"] == [], (name, report)
    swallowed = report["swallowed"]["single"]
    assert sorted(report["failed"]["single"] + swallowed) == everything, (name, report)
    if shards > 1:
        # every shard has a cull of its own, and which request of which worker thread draws number n differs from call to call
        assert report["failed"]["single"] and report["failed"]["full"][:1] == [1], (name, report)
        assert name in SWALLOWS_THE_CULL or (swallowed == [] and report["failed"]["full"] == everything), (name, report)
    elif name in SWALLOWS_THE_CULL:
        assert len(swallowed) == 2 and swallowed[1] == swallowed[0] + 1, (name, report)
        # with the device full from n on, the call fails unless nothing but the cull is left to ask for
        assert report["swallowed"]["full"] == (swallowed if swallowed[1] == report["A"] else []), (name, report)
    else:
        assert swallowed == [] and report["failed"]["full"] == everything, (name, report)


@pytest.mark.parametrize("name", list(afc.CASES))
def test_every_allocation_of_the_call_failed_in_turn(photon, workdir, name):
    case = afc.CASES[name](photon, workdir)
    if name in afc.WARM:
        afc.warm_up(case)
    check_report(name, afc.sweep(photon, case, name))


@pytest.mark.parametrize("name", ["start_ray_tracing_warm_volume", "start_ray_tracing_moments_without_volume"])
def test_three_shards_on_one_device_with_every_allocation_failed_in_turn(workdir, name):
    """PHOTON_DEVICES=0,0,0: three worker threads, a rendezvous, the sum on the first device.  Which worker draws the failing
    request varies; every outcome must pass the procedure.  In a child process with a time limit: a worker that never
    reaches the rendezvous fails this test with the child's stderr and does not stall the suite."""
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU in this environment (/dev/kfd absent)")
    env = dict(os.environ, PHOTON_DEVICES="0,0,0")
    child = subprocess.Popen([sys.executable, WORKER, name, workdir], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = child.communicate(timeout=120)
    except subprocess.TimeoutExpired:
        child.kill()
        out, err = child.communicate()
        pytest.fail(f"{name} under PHOTON_DEVICES=0,0,0 did not finish in 120 s (a hang: a worker that never arrived?)\n{out[-2000:]}\n{err[-4000:]}")
    assert child.returncode == 0, f"{name} under PHOTON_DEVICES=0,0,0 failed:\n{out[-2000:]}\n{err[-6000:]}"
    check_report(name, json.loads(out.strip().splitlines()[-1]), shards=3)
