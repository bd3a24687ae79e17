"""The procedure of tests/alloc_failure_cases.py can fail: run on a fake library (a Python object with a request counter and
the hook's two calls) it passes a sound call and fails each planted bug.  No GPU."""
import os

import numpy as np
import pytest

import alloc_failure_cases as afc


class FakeLibrary:
    """photon_pool.hip in miniature: numbered requests, a cache of freed pool blocks, the failure hook and its counters."""
    def __init__(self):
        self.requests = self.injected = self.retries = self.retry_blocks = self.outstanding = 0
        self.idle = []
        self.first = self.last = 0
        self.first_attempt_only = False

    def fail_alloc(self, first, count=1, first_attempt_only=False):
        self.first = self.requests + first if first else 0
        self.last = min(self.first + count - 1, afc.LLONG_MAX)
        self.first_attempt_only = bool(first_attempt_only)

    def alloc_stats(self):
        return dict(requests=self.requests, injected_failures=self.injected, oom_retries=self.retries, retry_blocks_returned=self.retry_blocks,
                    idle_blocks=len(self.idle), idle_bytes=64 * len(self.idle), outstanding_blocks=self.outstanding,
                    outstanding_bytes=64 * self.outstanding)

    def malloc(self, pooled, retries=True):
        self.requests += 1
        hit = self.first and self.first <= self.requests <= self.last
        if hit:
            self.injected += 1
            if not self.first_attempt_only or not retries:
                return False
            self.retries += 1
            self.retry_blocks += len(self.idle)
            self.idle.clear()
        elif pooled and self.idle:
            self.idle.pop()
        self.outstanding += 1
        return True

    def free(self, pooled):
        self.outstanding -= 1
        if pooled:
            self.idle.append(object())


BUGS = {
    "leaks_a_block": "a block leaked",
    "writes_before_it_fails": "was written although the call failed",
    "fails_silently": "said nothing on stderr",
    "returns_0_with_other_bits": "differs from the clean run in bits",
    "unusable_afterwards": "unusable after a failure",
    "never_retries": "no retry",
}


class FakeCase(afc.AllocCase):
    """out = 2 x through three pooled scratch blocks, on a long-lived direct block; `bug` plants one defect."""
    def __init__(self, lib, bug=None):
        self.lib, self.bug, self.broken = lib, bug, False
        self.x = np.arange(1.0, 9.0)

    def setup(self):
        assert self.lib.malloc(pooled=False)

    def teardown(self):
        self.lib.free(pooled=False)

    def fill(self):
        self.out = np.frombuffer(bytes([afc.SENTINEL_BYTE]) * 64, np.float64).copy()
        self.count = np.frombuffer(bytes([afc.SENTINEL_BYTE]) * 4, np.int32).copy()

    def call(self):
        if self.broken:
            os.write(2, b"photon: fake: the object is in a failed state\n")
            return 5, None
        held = 0
        for k in range(3):
            if k == 1 and self.bug == "writes_before_it_fails":
                self.out[0] = 2.0 * self.x[0]
            if not self.lib.malloc(pooled=True, retries=self.bug != "never_retries"):
                if k == 2 and self.bug == "returns_0_with_other_bits":
                    self.out[:] = 2.0 * self.x + 1.0
                    self.count[0] = 8
                    for _ in range(held):
                        self.lib.free(pooled=True)
                    return 0, (8,)
                if self.bug != "fails_silently":
                    os.write(2, b"photon: fake: device allocation failed\n")
                for _ in range(held - 1 if self.bug == "leaks_a_block" and held else held):
                    self.lib.free(pooled=True)
                self.broken = self.bug == "unusable_afterwards"
                return 3, None
            held += 1
        self.out[:] = 2.0 * self.x
        self.count[0] = 8
        for _ in range(held):
            self.lib.free(pooled=True)
        return 0, (8,)

    def outputs(self):
        return dict(out=self.out.copy(), count=self.count.copy())


def test_the_procedure_passes_a_sound_call_and_fails_every_bug():
    lib = FakeLibrary()
    report = afc.sweep(lib, FakeCase(lib), "sound")
    assert report["A"] == 3
    assert report["failed"] == dict(single=[1, 2, 3], full=[1, 2, 3], first_attempt=[])
    assert not any(report["swallowed"].values())
    assert lib.outstanding == 0 and lib.injected == 3 * 3 and lib.retries == 3      # a sound call stops at its first failed request
    for bug, message in BUGS.items():
        lib = FakeLibrary()
        with pytest.raises(AssertionError, match=message):
            afc.sweep(lib, FakeCase(lib, bug), bug)
        assert lib.first == 0, f"{bug}: the hook is still armed after the procedure failed"


def test_a_swallowed_failure_with_the_clean_bits_passes_and_one_with_a_hip_error_line_fails():
    class Swallows(FakeCase):
        def call(self):
            if not self.lib.malloc(pooled=True):                   # an optional scratch: the work is done without it
                os.write(2, self.line)
            else:
                self.lib.free(pooled=True)
            self.out[:] = 2.0 * self.x
            self.count[0] = 8
            return 0, (8,)

    lib = FakeLibrary()
    case = Swallows(lib)
    case.line = b"photon: fake: no scratch, the slow path is taken\n"
    report = afc.sweep(lib, case, "swallows")
    assert report["A"] == 1 and report["swallowed"]["single"] == [1] and report["failed"]["single"] == []
    case.line = b"photon: HIP error 2 (out of memory) at fake.hip:1: scratch.alloc(n)\n"
    with pytest.raises(AssertionError, match="the call succeeded and printed"):
        afc.sweep(lib, case, "swallows loudly")


def test_a_call_whose_requests_do_not_repeat_is_reported():
    class Keeps(FakeCase):
        """Allocates in its first call only (a scene that has grown): request n of a later call would never be made."""
        grown = False

        def call(self):
            if self.grown:
                self.out[:] = 2.0 * self.x
                self.count[0] = 8
                return 0, (8,)
            self.grown = True
            return FakeCase.call(self)

    lib = FakeLibrary()
    with pytest.raises(AssertionError, match="does not make 3 requests"):
        afc.sweep(lib, Keeps(lib), "keeps")


def test_stderr_of_the_c_level_is_captured_and_handed_back():
    with afc.captured_stderr() as err:
        os.write(2, b"photon: one line\n")
    assert err == ["photon: one line\n"]
    assert afc.holds_sentinel(np.full(3, afc.SENTINEL, np.int8)) and not afc.holds_sentinel(np.array([afc.SENTINEL], np.int32))
    assert afc.holds_sentinel(np.full(5, afc.SENTINEL_BYTE, np.uint8).view(np.uint8))
