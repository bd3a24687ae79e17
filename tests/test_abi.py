"""C-ABI checks that need no GPU: struct layouts against what the reference's marshalling code
produced (tests/golden/abi_*.{json,npz}), symbol export, header/library agreement, and the binding's signature table
against the header's prototypes."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture_call
from photon_amd import ray_tracing as rt
from photon_amd.library import DECLARED_SYMBOLS, SIGNATURES, apply_signatures


def test_struct_sizes_match_reference_marshalling():
    for case in ("piv", "bos_im1", "bos_im2"):
        with open(os.path.join(GOLDEN, f"abi_{case}.json")) as f:
            sz = json.load(f)["sizeof"]
        assert ctypes.sizeof(rt.scattering_data_struct) == sz["scattering"] == 72
        assert ctypes.sizeof(rt.lightfield_source_struct) == sz["source"] == 64
        assert ctypes.sizeof(rt.camera_design_struct) == sz["camera"] == 112
        assert ctypes.sizeof(rt.element_data_struct) == sz["element"] == 120


def test_field_offsets():
    # SURVEY.md section 8a row a22 (verified there with g++ and ctypes)
    e, c, s, m = rt.element_data_struct, rt.camera_design_struct, rt.lightfield_source_struct, rt.scattering_data_struct
    assert (e.element_type.offset, e.rotation_angles.offset, e.element_properties.offset) == (80, 88, 56)
    assert (c.implement_diffraction.offset, c.rotation_matrix.offset, c.inverse_rotation_matrix.offset) == (36, 40, 76)
    assert (s.num_particles.offset, s.z_offset.offset, s.object_distance.offset) == (48, 52, 56)
    assert (m.scattering_angle.offset, m.scattering_irradiance.offset, m.num_angles.offset) == (48, 56, 64)
    assert ctypes.sizeof(rt.element_geometry_struct) == 32 and ctypes.sizeof(rt.element_properties_struct) == 24


@pytest.mark.parametrize("case", ["piv", "bos_im1", "bos_im2"])
def test_packed_structs_are_byte_identical_to_the_reference(case):
    """Our mirror of prepare_data_for_cytpes_call must lay the camera / element structs out exactly
    as the reference did (raw bytes captured at its ctypes call)."""
    call = load_fixture_call(case)
    a = np.load(os.path.join(GOLDEN, f"abi_{case}.npz"))
    sd, ls, elems, centers, planes, sysidx, cam = call.pack()

    def same(ours: bytes, ref: np.ndarray, holes):
        ours = np.frombuffer(ours, np.uint8).copy()
        ref = ref.copy()
        for lo, hi in holes:                     # padding bytes are unspecified
            ours[lo:hi] = 0
            ref[lo:hi] = 0
        return np.array_equal(ours, ref)

    assert same(bytes(cam), a["raw_camera"], [(37, 40)])
    assert same(bytes(elems[0]), a["raw_element0"], [(21, 24), (29, 32), (52, 56), (81, 84), (116, 120)])
    assert np.array_equal(centers, a["element_center"]) and np.array_equal(planes, a["element_plane_parameters"])
    assert np.array_equal(sysidx, a["element_system_index"].reshape(-1))
    assert ls.num_particles == a["src_x"].size and ls.source_point_number == 10000


def _header_text():
    """The header without its comments."""
    with open(os.path.join(ROOT, "include", "parallel_ray_tracing.h")) as f:
        text = f.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _header_functions():
    return set(re.findall(r"\b((?:start_ray_tracing|photon_[a-z0-9_]+))\s*\(", _header_text()))


_C_KINDS = {"int": "int", "unsigned": "unsigned", "unsigned int": "unsigned", "long long": "int64", "int64_t": "int64",
            "unsigned long long": "uint64", "uint64_t": "uint64", "size_t": "uint64", "float": "float", "double": "double",
            "bool": "bool"}


def _c_kind(decl: str, is_return: bool = False) -> str:
    """Kind of one parameter ('const double spacing[3]', 'int nx') or of a return type ('const char *')."""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    base = " ".join(words if is_return else words[:-1])         # a parameter ends with its name
    if is_return and base == "void":
        return "void"
    assert base in _C_KINDS, f"unknown C type in {decl!r}"
    return _C_KINDS[base]


def _header_prototypes():
    """{name: (return kind, [parameter kinds])} of every function the header declares: what is left between two ';' once
    comments, preprocessor lines, struct bodies, typedefs and the extern "C" braces are gone must read `ret name(params)`."""
    text = re.sub(r"^\s*#.*$", "", _header_text(), flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", text)
    text = text.replace('extern "C" {', "").replace("}", "")
    out = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"
        ret, name, params = m.groups()
        assert name not in out, name
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        out[name] = (_c_kind(ret, is_return=True), [_c_kind(p) for p in params])
    return out


def _ctypes_kind(t) -> str:
    if t is None:
        return "void"
    if issubclass(t, ctypes._Pointer):
        return "pointer"
    code = t._type_                                              # the struct-module code of a simple ctypes type
    if code in "zP":
        return "pointer"
    if code in "fd?":
        return {"f": "float", "d": "double", "?": "bool"}[code]
    assert code in "iIlLqQ", f"no kind for {t}"
    return {(4, True): "int", (4, False): "unsigned", (8, True): "int64", (8, False): "uint64"}[ctypes.sizeof(t), code.islower()]


_PROTOTYPES = _header_prototypes()


def test_header_and_python_binding_declare_the_same_symbols():
    assert _header_functions() == set(DECLARED_SYMBOLS) == set(SIGNATURES) == set(_PROTOTYPES)
    assert len(DECLARED_SYMBOLS) == len(set(DECLARED_SYMBOLS))


@pytest.mark.parametrize("name", sorted(_header_functions()))
def test_signature_table_agrees_with_the_header(name):
    """Arity, the kind of every parameter and the kind of the return value, symbol by symbol: a Python int handed to a
    symbol whose pointer or 64-bit parameter is not declared as such is silently cut to a C int."""
    restype, argtypes = SIGNATURES[name]
    assert (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes]) == _PROTOTYPES[name]


def test_library_loads_and_exports_every_declared_symbol():
    """No compute call: just dlopen + dlsym (works without a GPU).  After apply_signatures every symbol is typed."""
    from photon_amd import build
    path = build.build_library()
    lib = ctypes.CDLL(path)
    for name in DECLARED_SYMBOLS:
        assert hasattr(lib, name), name
    assert apply_signatures(lib) is lib
    for name in DECLARED_SYMBOLS:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(SIGNATURES[name][1]), name
        assert f.restype is SIGNATURES[name][0], name
    assert b"gfx950" in lib.photon_version()


def test_apply_signatures_skips_symbols_a_library_lacks():
    """A build from before an entry point existed loads the same way (A/B runs): libc exports none of the table."""
    import ctypes.util
    libc = apply_signatures(ctypes.CDLL(ctypes.util.find_library("c")))
    assert not any(hasattr(libc, name) for name in DECLARED_SYMBOLS)


def test_product_does_not_reference_the_oracle():
    """The product path must not import / link / call anything under oracle/."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "photon_amd")):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                with open(os.path.join(dirpath, fn), errors="replace") as f:
                    text = f.read()
                assert "oracle_lib" not in text and "libphoton_oracle" not in text and "oracle/" not in text, fn
