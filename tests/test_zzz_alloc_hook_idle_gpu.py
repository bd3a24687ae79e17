"""Runs last: the allocation hook has shown nowhere but in the sweeps that armed it."""
import pytest

import alloc_failure_cases as afc

pytestmark = pytest.mark.gpu


def test_no_failure_was_injected_and_no_retry_taken_outside_the_sweeps(photon):
    """photon_selftest_alloc_stats over the whole process: every injected failure and every out-of-memory retry is one that a
    sweep of tests/alloc_failure_cases.py caused and counted (none at all when tests/test_alloc_failures_gpu.py did not
    run) -- the hook is disarmed everywhere else, and no test met a device that was really full."""
    stats = photon.alloc_stats()
    assert stats["requests"] > 0
    tally = afc.tally_of(photon)
    assert {k: stats[k] for k in tally} == tally
