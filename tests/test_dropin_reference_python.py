"""The drop-in boundary as photon's Python reaches it: the library is loaded from the path photon always uses --
`ctypes.CDLL(os.path.abspath('../cuda_codes/Debug/libparallel_ray_tracing.so'))` relative to its cwd
(perform_ray_tracing_03.py:1888), a symlink to this repo's library in the layout of INTEGRATION.md -- and
`start_ray_tracing` is called with the arguments photon's own marshalling produced for the two images of its sample BOS
case (captured in tests/golden/abi_bos_im{1,2}.{json,npz}; their struct bytes are pinned by tests/test_abi.py).  Without
a GPU the library must report the HIP error and leave the image untouched -- the contract of the header for a failed
call; with one, both images render."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLER = r"""
import ctypes, json, os, shutil, sys, tempfile
root = sys.argv[1]
sys.path.insert(0, root)
from photon_amd.ray_tracing import RayTracingCall, bind_start_ray_tracing
golden = os.path.join(root, "tests", "golden")
work = tempfile.mkdtemp(prefix="photon_dropin_")
os.makedirs(os.path.join(work, "python_codes"))
os.makedirs(os.path.join(work, "cuda_codes", "Debug"))
os.symlink(os.path.join(root, "photon_amd", "libparallel_ray_tracing.so"),
           os.path.join(work, "cuda_codes", "Debug", "libparallel_ray_tracing.so"))        # INTEGRATION.md step 2
os.chdir(os.path.join(work, "python_codes"))
calls, sums = [], []
for case in ("bos_im1", "bos_im2"):                 # one load per image, as photon's driver does
    path = os.path.abspath("../cuda_codes/Debug/libparallel_ray_tracing.so")
    lib = ctypes.CDLL(path)
    calls.append({"path": path, "resolves_to": os.path.realpath(path), "has_symbol": hasattr(lib, "start_ray_tracing")})
    call = RayTracingCall.from_fixture(os.path.join(golden, f"abi_{case}.json"), os.path.join(golden, f"abi_{case}.npz"),
                                       density_dir=golden)
    image = call.new_image()
    call.invoke(bind_start_ray_tracing(lib), image)
    sums.append(float(image.astype("float64").sum()))
os.chdir(root)
shutil.rmtree(work, ignore_errors=True)
print("DROPIN " + json.dumps({"cdll_calls": calls, "images_returned": len(sums), "raw_image_sums": sums}))
"""


def test_captured_reference_call_through_the_dropin_path():
    from photon_amd import build
    build.build_library()                               # if missing or stale; the library is mapped in the child only
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PHOTON_DEVICES", None)
    r = subprocess.run([sys.executable, "-c", CALLER, ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out, err = r.stdout.decode("utf-8", "replace"), r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, err[-2000:]
    line = [ln for ln in out.splitlines() if ln.startswith("DROPIN ")]
    assert len(line) == 1
    d = json.loads(line[0][len("DROPIN "):])
    lib = os.path.realpath(os.path.join(ROOT, "photon_amd", "libparallel_ray_tracing.so"))
    # the sample BOS case renders two images: two loads through photon's own relative path, both landing on our file
    assert len(d["cdll_calls"]) == 2 and d["images_returned"] == 2
    for c in d["cdll_calls"]:
        assert c["path"].endswith("cuda_codes/Debug/libparallel_ray_tracing.so") and c["resolves_to"] == lib and c["has_symbol"]
    if not os.path.exists("/dev/kfd"):
        # no GPU here: each call says so and hands the caller's image back untouched
        assert err.count("image left untouched") == 2 and "photon: HIP error" in err
        assert d["raw_image_sums"] == [0.0, 0.0]
    else:
        assert all(s > 0 for s in d["raw_image_sums"])
