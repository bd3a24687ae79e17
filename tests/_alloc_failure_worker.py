"""The allocation-failure sweep of one case of tests/alloc_failure_cases.py in a process of its own: for the cases that run
under PHOTON_DEVICES (worker threads, a rendezvous), so that a worker that never arrives costs this process and not the
suite.  Usage: python _alloc_failure_worker.py <case> <workdir>; prints the sweep's report as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    name, workdir = sys.argv[1], sys.argv[2]
    import torch  # noqa: F401  -- before the library: one HIP runtime per process (tests/conftest.py)
    import alloc_failure_cases as afc
    from photon_amd.library import PhotonLibrary
    lib = PhotonLibrary(build=False)
    lib.set_device(0)
    case = afc.CASES[name](lib, workdir)
    case.concurrent = len(os.environ.get("PHOTON_DEVICES", "").split(",")) > 1
    if name in afc.WARM:
        afc.warm_up(case)
    print(json.dumps(afc.sweep(lib, case, f"{name} under PHOTON_DEVICES={os.environ.get('PHOTON_DEVICES')}")))


if __name__ == "__main__":
    main()
