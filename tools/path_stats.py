"""Which sampler path the waves of a launch take (debug build of the library with -DPHOTON_PATH_STATS=1,
build/variants/lib_pathstats.so): every slot of enum PathSlot (device_volume_coop.hpp) by name, the summary ratios, and
the splat paths of the same trace's sensor stage (enum SplatSlot, device_optics.hpp).
    python tools/build_variant.py pathstats -DPHOTON_PATH_STATS=1
    PHOTON_LIBRARY=build/variants/lib_pathstats.so python tools/path_stats.py [c5 scale | c3] [--linear]"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from photon_amd import path_stats, scenes  # noqa: E402
from photon_amd.library import PhotonLibrary  # noqa: E402

interp = 1 if "--linear" in sys.argv else 2
argv = [a for a in sys.argv if a != "--linear"]
what = argv[1] if len(argv) > 1 else "c5"
scale = float(argv[2]) if len(argv) > 2 else 0.25
lib = PhotonLibrary()
work = os.path.join(tempfile.gettempdir(), "photon_bench")
os.makedirs(work, exist_ok=True)
call = scenes.config("C5", work, scale=scale) if what == "c5" else scenes.config("C3", work)
scene = lib.scene_create(call)
vol = lib.volume_load_nrrd(call.density_grad_filename, interp)
H, W = call.image_shape
img = torch.zeros(H * W, dtype=torch.float32, device="cuda")
scene.trace(img.data_ptr(), vol, 2)
path_stats.read(lib)                                     # clear after the warm-up
path_stats.read_splat(lib)
st = scene.trace(img.data_ptr(), vol, 2, want_stats=True)
c = path_stats.read(lib)
sp = path_stats.read_splat(lib)
p = "L_" if interp == 1 else "C_"
ws = c[p + "COHERENT"] + c[p + "INCOHERENT"]
for k, v in c.items():
    if k.startswith(p):
        print(f"{k:22s} {v:14d}")
for k, v in sp.items():
    print(f"{k:22s} {v:14d}")
print(json.dumps({"workload": what, "interp": interp, "rays_marched": st.rays_marched, "march_ms": round(st.march_ms, 2), "wave_samples": ws,
                  "coherent_frac": round(c[p + "COHERENT"] / max(ws, 1), 4),
                  "tile_fetch_per_coherent": round((c["C_FETCH_UP"] + c["C_FETCH_DOWN"] if interp == 2 else c["L_FETCH"]) / max(c[p + "COHERENT"], 1), 3),
                  "brick_passes_per_incoherent": round(c[p + "BRICK_PASS"] / max(c[p + "INCOHERENT"], 1), 3),
                  "brick_fetch_per_pass": round(c[p + "BRICK_FETCH"] / max(c[p + "BRICK_PASS"], 1), 3),
                  "lanes_per_pass": round(c[p + "BRICK_LANES"] / max(c[p + "BRICK_PASS"], 1), 1),
                  "gathered_lanes_per_incoherent": round(c[p + "GATHER_LANES"] / max(c[p + "INCOHERENT"], 1), 3),
                  "erf_cooperative_frac": round(sp["E_COOP"] / max(sp["E_WAVES"], 1), 4),
                  "erf_same_window_tile_frac": round(sp["E_TILES_SAME"] / max(sp["E_TILES"], 1), 4),
                  "taps_cooperative_frac": round(sp["T_COOP"] / max(sp["T_WAVES"], 1), 4)}))
