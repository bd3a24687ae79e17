"""Sampler-path counters of a debug build of the library (-DPHOTON_PATH_STATS=1): the Python mirror of `enum PathSlot`
(photon_amd/csrc/device_volume_coop.hpp, where each slot is described) and a reader.

    lib = PhotonLibrary(path=build_library(extra_flags=("-DPHOTON_PATH_STATS=1",), out_path=...))
    read(lib)           # {slot name: count} since the last read; reading clears the counters

C_ slots count the tricubic sampler's march, L_ slots the trilinear one's (both weight modes).

The same build counts the paths of the sensor stage: `enum SplatSlot` (photon_amd/csrc/device_optics.hpp), mirrored by
SPLAT_SLOTS and read by read_splat().  E_ slots count the erf splat, T_ slots the 4-pixel splat, K_ slots the
sensor_kernel instantiations."""
from __future__ import annotations

import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "device_volume_coop.hpp")

SLOTS = (
    "C_COHERENT", "C_HIT_CELL", "C_CELL_IN_TILE", "C_FETCH_UP", "C_FETCH_DOWN", "C_TILE_CLAMPED",
    "C_INCOHERENT", "C_INCOHERENT_LANES", "C_BRICK_PASS", "C_BRICK_FETCH", "C_BRICK_REUSED", "C_BRICK_CLAMPED",
    "C_BRICK_LANES", "C_GATHER_LANES", "C_SPIN_OUTSIDE", "C_SPIN_LOW", "C_SPIN_CAP",
    "L_COHERENT", "L_HIT_A", "L_HIT_B", "L_TILE_B_LANES", "L_FETCH", "L_FETCH_TWO", "L_FETCH_TO_B", "L_FETCH_DOWN",
    "L_BASE_AHEAD", "L_BASE_BEHIND", "L_TILE_CLAMPED", "L_NO_FREE_TILE", "L_OUT_OF_REACH", "L_MARK_INCOHERENT",
    "L_TILES_SKIPPED", "L_RETRY", "L_COHERENT_AGAIN", "L_INCOHERENT", "L_INCOHERENT_LANES", "L_BRICK_PASS",
    "L_BRICK_FETCH", "L_BRICK_REUSED", "L_BRICK_CLAMPED", "L_BRICK_LANES", "L_GATHER_LANES", "L_SPIN_OUTSIDE",
    "L_SPIN_CAP", "L_LOW", "L_REPAIR_LANES", "L_KEEP_PREV_LANES",
)

OPTICS_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "device_optics.hpp")

SPLAT_SLOTS = (
    "E_WAVES", "E_COOP", "E_FALLBACK", "E_FB_WIDE", "E_FB_TILES", "E_FB_RADIUS",
    "E_SHARED_X_LANES", "E_BOTH_X_LANES", "E_SHARED_Y_LANES", "E_BOTH_Y_LANES", "E_CLIPPED_LANES", "E_LANE_CLIPPED_LANES",
    "E_TILES", "E_TILES_SAME", "E_TILES_MIXED", "E_MULTI_TILE",
    "T_WAVES", "T_COOP", "T_LANE_ROUTE", "T_MULTI_TILE", "T_TAPS_LANDED", "T_TAPS_DROPPED", "T_TAPS_WRAPPED",
    "K_GEN_ERF", "K_STATE_ERF", "K_GEN_TRAIN", "K_STATE_TRAIN", "K_GEN_TAPS", "K_STATE_TAPS",
)

PATH_STATS_FLAGS = ("-DPHOTON_PATH_STATS=1",)


def header_slots(path: str = HEADER):
    """The slot names of `enum PathSlot` as the header spells them (without the PS_ prefix), in order."""
    with open(path) as f:
        text = f.read()
    body = re.search(r"enum PathSlot\s*:\s*int\s*\{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"^\s*PS_(\w+)\s*,", body, re.M)
    assert names and names[-1] != "COUNT"
    return tuple(names)


def header_splat_slots(path: str = OPTICS_HEADER):
    """The slot names of `enum SplatSlot` as the header spells them (without the SS_ prefix), in order."""
    with open(path) as f:
        text = f.read()
    body = re.search(r"enum SplatSlot\s*:\s*int\s*\{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"^\s*SS_(\w+)\s*,", body, re.M)
    assert names and names[-1] != "COUNT"
    return tuple(names)


def read_splat(lib) -> dict:
    """Counters of the sensor unit since the last read (which this one clears), by slot name."""
    f = lib.lib.photon_debug_splat_stats
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    f.restype = ctypes.c_int
    out = (ctypes.c_ulonglong * len(SPLAT_SLOTS))()
    rc = f(ctypes.cast(out, ctypes.c_void_p), len(SPLAT_SLOTS))
    if rc != 0:
        raise RuntimeError(f"photon_debug_splat_stats failed ({rc})")
    return dict(zip(SPLAT_SLOTS, (int(v) for v in out)))


def read(lib) -> dict:
    """Counters of both march units since the last read (which this one clears), by slot name."""
    f = lib.lib.photon_debug_path_stats
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    f.restype = ctypes.c_int
    out = (ctypes.c_ulonglong * len(SLOTS))()
    rc = f(ctypes.cast(out, ctypes.c_void_p), len(SLOTS))
    if rc != 0:
        raise RuntimeError(f"photon_debug_path_stats failed ({rc})")
    return dict(zip(SLOTS, (int(v) for v in out)))
