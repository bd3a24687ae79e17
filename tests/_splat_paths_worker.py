"""The family matrix of tests/test_splat_paths_gpu.py on one build of the library: every family of tests/splat_families.py
through a scene (trace with a statistics window, a second trace on top, trace_moments) and through start_ray_tracing with
every ray dumped, against the oracle's results.  Run in-process on the default library, and in a process of its own on the
path-stats build:
    python _splat_paths_worker.py <library.so> <families.pkl> <workdir> <out.json>
Writes {"mismatches": [...], "counts": {family: {slot: n}}} (counts: path-stats builds; of each family's first trace)."""
import copy
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from test_splat_paths import image_mismatch  # noqa: E402


def _dump_mismatch(name, what, got, want):
    """Bit-equal, NaN exactly where the oracle has NaN (the inside test at the boundary)."""
    if got.shape != want.shape:
        return f"{name} {what}: {got.shape} values dumped, the oracle has {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (gn & wn)
    if same.all():
        return None
    r, c = np.argwhere(~same)[0]
    return (f"{name} {what}: {int((~same).any(axis=1).sum())} of {len(got)} rays differ, {int((gn != wn).any(axis=1).sum())} in where the NaNs are; "
            f"first ray {r} component {c}: {got[r, c]!r} vs {want[r, c]!r}")


def run_families(lib, fams, want, workdir, read_counts=None):
    """Every family against the oracle's results want[name] (splat_families.oracle_render).  Returns (mismatches, counts)."""
    import torch
    bad, counts = [], {}
    volumes = {}
    if read_counts:
        read_counts()                                   # clear
    for f in fams:
        call, w = f.call, want[f.name]
        H, W = call.image_shape
        vol = None
        if f.volume:
            if call.density_grad_filename not in volumes:
                volumes[call.density_grad_filename] = lib.volume_load_nrrd(call.density_grad_filename, 1)
            vol = volumes[call.density_grad_filename]
        alg = int(call.ray_tracing_algorithm) if f.volume else 0
        scene = lib.scene_create(call)
        try:
            if f.train:
                scene.set_element_train(1)
            if f.noise_seed:
                scene.set_noise(add_pos_noise=True, pos_noise_std=call.pos_noise_std, seed=f.noise_seed)
            img = torch.zeros(H * W, dtype=torch.float32, device="cuda")
            scene.stats_begin()
            scene.trace(img.data_ptr(), vol, alg)
            st = scene.stats_end()
            if read_counts:
                counts[f.name] = read_counts()
                counts[f.name]["rays_on_sensor"] = int(st.rays_on_sensor)
            first = img.cpu().numpy().reshape(H, W).copy()
            for what, got, ref in (("rays_on_sensor", st.rays_on_sensor, w["rays_on_sensor"]), ("sensor_taps", st.sensor_taps, w["sensor_taps"])):
                if int(got) != int(ref):
                    bad.append(f"{f.name}: {what} {int(got)}, the oracle has {int(ref)}")
            bad.append(image_mismatch(f, first, w["image"], "trace"))
            scene.trace(img.data_ptr(), vol, alg)           # on top of the first
            if f.erf:
                second = img.cpu().numpy().reshape(H, W)
                m = image_mismatch(f, second, np.float32(2.0) * first, "second trace on top, against twice the first")
                bad.append(m)
            img2 = torch.zeros(H * W, dtype=torch.float32, device="cuda")
            records = torch.zeros(call.num_sources * 8, dtype=torch.float64, device="cuda")
            scene.trace_moments(img2.data_ptr(), records.data_ptr(), vol, alg)
            bad.append(image_mismatch(f, img2.cpu().numpy().reshape(H, W), w["image"], "trace_moments"))
        finally:
            scene.free()
        # start_ray_tracing with every ray dumped (every ray launched, in the reference's order: other waves than the scene's)
        c = copy.copy(call)
        d = os.path.join(workdir, "gpu_" + f.name)
        os.makedirs(d, exist_ok=True)
        c.save_lightrays, c.num_lightrays_save = True, c.num_rays
        c.lightray_position_save_path = c.lightray_direction_save_path = d
        env = {"PHOTON_ELEMENT_TRAIN": "sequential" if f.train else None, "PHOTON_NOISE_SEED": str(f.noise_seed) if f.noise_seed else None,
               "PHOTON_INTERP": "linear"}
        before = {k: os.environ.get(k) for k in env}
        try:
            for k, v in env.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            g = lib.render(c)
        finally:
            for k, v in before.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        bad.append(image_mismatch(f, g, w["image"], "start_ray_tracing"))
        for what, prefix in (("final positions", "pos_"), ("directions", "dir_")):
            got = np.fromfile(os.path.join(d, prefix + "0000.bin"), np.float32).reshape(-1, 3)
            bad.append(_dump_mismatch(f.name, what, got, w[prefix[:3]]))
        if read_counts:
            read_counts()                               # the dumping render's waves are not the family's
    for v in volumes.values():
        v.free()
    return [b for b in bad if b], counts


def main():
    lib_path, pkl, workdir, out = sys.argv[1:5]
    import torch  # noqa: F401  -- before the library: one HIP runtime per process (photon_amd/library.py)
    from photon_amd import path_stats
    from photon_amd.library import PhotonLibrary
    lib = PhotonLibrary(path=lib_path, build=False)
    lib.set_device(0)
    with open(pkl, "rb") as f:
        fams, want = pickle.load(f)
    stats = hasattr(lib.lib, "photon_debug_splat_stats")
    bad, counts = run_families(lib, fams, want, workdir, (lambda: path_stats.read_splat(lib)) if stats else None)
    with open(out, "w") as f:
        json.dump({"mismatches": bad, "counts": counts, "version": lib.version()}, f)
    print(f"{lib.version()}: {len(bad)} mismatches")


if __name__ == "__main__":
    main()
