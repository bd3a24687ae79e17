"""The march matrix of tests/test_sampler_paths_gpu.py on one build of the library, in a process of its own (a debug or
switch-variant build: PhotonLibrary(path=...)): the ray families, the fuzz rays of the adversarial parity test, and two
renders through start_ray_tracing with sensor moments.
    python _sampler_paths_worker.py <library.so> <oracle.npz> <volume.nrrd> <out.json>
Writes {"mismatches": [...], "counts": {family or "adv<seed>": {sampler/algorithm: {slot: n}}}} (counts: path-stats builds)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import sampler_families as sf  # noqa: E402


def _march(lib, vols, cases, want, read_counts, bad, counts):
    """cases: (name, volume key, {interp: (pos, dir)}).  Each through the plain grid and the queued launch in 1, 3 and 7
    pieces: positions, directions and (plain grid; the queued launch reports none) iteration counts bit for bit."""
    for name, vk, rays in cases:
        counts[name] = {}
        for s, interp, bits in sf.SAMPLERS:
            v = vols[vk][interp]
            if interp == 1:
                v.set_weight_bits(bits)
            pos, d = rays[interp]
            for a in sf.ALGORITHMS:
                key = f"{name}/{s}/{a}"
                wp, wd, ws = want[key + "/pos"], want[key + "/dir"], want[key + "/steps"]
                gp, gd, gs = v.trace_rays(pos, d, a)
                runs = [("plain", gp, gd)]
                if not np.array_equal(gs, ws):
                    bad.append(f"{key} plain: iteration counts differ at rays {np.flatnonzero(gs != ws)[:5].tolist()}")
                for seg in sf.SEGMENTS:
                    qp, qd = v.trace_rays_queued(pos, d, a, seg)
                    runs.append((f"queued/{seg}", qp, qd))
                for how, p, dd in runs:
                    for what, got, ref in (("positions", p, wp), ("directions", dd, wd)):
                        diff = np.any(got.view(np.uint32) != ref.view(np.uint32), axis=1)
                        if diff.any():
                            bad.append(f"{key} {how}: {what} differ in {int(diff.sum())} rays, first {np.flatnonzero(diff)[:5].tolist()}")
                if read_counts:
                    counts[name][f"{s}/{a}"] = read_counts()


def run_matrix(lib, want, read_counts=None, adversarial=False):
    """Every family (and with adversarial=True the fuzz rays of every seed) for every sampler and algorithm, against the
    oracle's results `want` (sf.oracle_results, sf.oracle_adversarial).  Returns (mismatches, counts)."""
    bad, counts = [], {}
    vols = {}
    for k in sf.VOLUMES:
        rho, sp, org = sf.volume_density(k)
        vols[k] = {1: lib.volume_from_density(rho, sp, org, 1), 2: lib.volume_from_density(rho, sp, org, 2)}
    if read_counts:
        read_counts()                                   # clear
    try:
        fams = sf.all_families({k: v[1].info() for k, v in vols.items()})
        _march(lib, vols, [(f.name, f.volume, {1: (f.pos, f.dir), 2: (f.pos, f.dir)}) for f in fams], want, read_counts, bad, counts)
    finally:
        for vv in vols.values():
            for x in vv.values():
                x.free()
    if adversarial:
        for seed in sf.ADVERSARIAL_SEEDS:
            rho, sp, org, _ = sf.adversarial_case(seed)
            vols = {"adv": {1: lib.volume_from_density(rho, sp, org, 1), 2: lib.volume_from_density(rho, sp, org, 2)}}
            try:
                _march(lib, vols, [(f"adv{seed}", "adv", sf.adversarial_rays(seed, vols["adv"][1].info()))], want, read_counts, bad, counts)
            finally:
                for x in vols["adv"].values():
                    x.free()
    return bad, counts


def run_renders(lib, want, nrrd):
    """The BOS and PIV renders through start_ray_tracing with sensor moments, both samplers and algorithms: the exact
    record fields against the host model of the oracle's ray dumps, bit for bit."""
    bad = []
    for name in sf.RENDERS:
        for interp in (1, 2):
            os.environ["PHOTON_INTERP"] = "cubic" if interp == 2 else "linear"
            for a in sf.ALGORITHMS:
                _, rec = lib.render_moments(sf.render_call(name, nrrd, a))
                ref = want[f"render/{name}/{interp}/{a}"]
                g = np.ascontiguousarray(rec[:, sf.RENDER_EXACT]).view(np.uint64)
                w = np.ascontiguousarray(ref[:, sf.RENDER_EXACT]).view(np.uint64)
                if rec.shape != ref.shape or rec[:, 0].sum() == 0:
                    bad.append(f"render {name} interp {interp} algorithm {a}: records {rec.shape}, {rec[:, 0].sum()} rays arrived")
                elif (g != w).any():
                    bad.append(f"render {name} interp {interp} algorithm {a}: {int((g != w).any(axis=1).sum())} records differ")
    return bad


def main():
    lib_path, npz, nrrd, out = sys.argv[1:5]
    import torch  # noqa: F401  -- before the library: one HIP runtime per process (photon_amd/library.py)
    from photon_amd import path_stats
    from photon_amd.library import PhotonLibrary
    lib = PhotonLibrary(path=lib_path, build=False)
    lib.set_device(0)
    want = dict(np.load(npz))
    stats = hasattr(lib.lib, "photon_debug_path_stats")
    bad, counts = run_matrix(lib, want, (lambda: path_stats.read(lib)) if stats else None, adversarial=True)
    bad += run_renders(lib, want, nrrd)
    with open(out, "w") as f:
        json.dump({"mismatches": bad, "counts": counts, "version": lib.version()}, f)
    print(f"{lib.version()}: {len(bad)} mismatches")


if __name__ == "__main__":
    main()
