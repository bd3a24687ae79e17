"""The Python binding of libparallel_ray_tracing.so (C-ABI: include/parallel_ray_tracing.h).

Three layers, top to bottom of the file:
  * ``SIGNATURES``: restype and argtypes of every symbol the header declares, applied by ``apply_signatures`` to any
    loaded library.  The header is the source of truth; tests/test_abi.py holds the table against its prototypes.
  * ``PhotonLibrary``: one method per entry point -- marshalling only, raw device pointers in, return code checked -- and
    on top of those the pipelines that chain several calls on torch-allocated device buffers on the current stream
    (``preprocess_series``, ``correlate``, ``correlate_deform``, ``correlate_stereo``, ``self_calibrate_stereo``, ``reconstruct_volume``, ``correlate_tomo``, ``optical_flow``, ``displacement_uncertainty``, ``correlation_predictor``, ``track_dots``,
    ``integrate_gradient``, the tomography solvers).
  * ``Volume``, ``Sources``, ``Flow``, ``Scene``: the library's handles.
All arithmetic is the HIP library's.  There is no Python or CPU fallback -- if the library is missing or a call fails,
you get an exception.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np

from . import build as _build
from .ray_tracing import (START_RAY_TRACING_ARGTYPES, RayTracingCall, camera_design_struct, element_data_struct,
                          lightfield_source_struct, scattering_data_struct)


class photon_volume_info_t(ctypes.Structure):
    _fields_ = [("min_bound", ctypes.c_float * 3), ("max_bound", ctypes.c_float * 3),
                ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("nz", ctypes.c_int),
                ("grid_spacing", ctypes.c_float * 3), ("step_size", ctypes.c_float),
                ("data_min", ctypes.c_float), ("interpolation", ctypes.c_int)]


class _Stats(ctypes.Structure):
    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class photon_trace_stats_t(_Stats):
    _fields_ = [("rays_launched", ctypes.c_uint64), ("rays_on_sensor", ctypes.c_uint64),
                ("rk_iterations", ctypes.c_uint64), ("volume_samples", ctypes.c_uint64),
                ("sensor_taps", ctypes.c_uint64), ("march_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("rays_marched", ctypes.c_uint64), ("shader_clock_mhz", ctypes.c_float), ("traces", ctypes.c_uint32),
                ("march_wave_ms", ctypes.c_float)]


class photon_integrate_stats_t(_Stats):
    _fields_ = [("iterations", ctypes.c_int), ("converged", ctypes.c_int), ("unknowns", ctypes.c_int),
                ("unreachable", ctypes.c_int), ("residual", ctypes.c_double)]


class photon_tomo_stats_t(_Stats):
    _fields_ = [("iterations", ctypes.c_int), ("converged", ctypes.c_int), ("unknowns", ctypes.c_longlong),
                ("rays_used", ctypes.c_longlong), ("residual", ctypes.c_double)]


class photon_alloc_stats_t(_Stats):
    _fields_ = [(n, ctypes.c_longlong) for n in ("requests", "injected_failures", "oom_retries", "retry_blocks_returned", "idle_blocks",
                                                 "idle_bytes", "outstanding_blocks", "outstanding_bytes")]


class photon_march_profile_t(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("waves", ctypes.c_uint32),
                ("span_ms", ctypes.c_float), ("start_mean_ms", ctypes.c_float), ("start_max_ms", ctypes.c_float),
                ("end_min_ms", ctypes.c_float), ("end_mean_ms", ctypes.c_float)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "struct_size"}
        d["drain_ms"] = d["span_ms"] - d["end_mean_ms"]
        return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}


class photon_march_plan_t(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("segments", ctypes.c_int), ("shape", ctypes.c_int),
                ("seg_begin", ctypes.c_uint * 65), ("groups_per_chunk", ctypes.c_uint), ("grid_blocks", ctypes.c_uint),
                ("block_threads", ctypes.c_uint), ("persistent", ctypes.c_int), ("save", ctypes.c_int), ("noise", ctypes.c_int),
                ("segmented", ctypes.c_int), ("generates_rays", ctypes.c_int)]


class photon_piv_camera_t(ctypes.Structure):
    _fields_ = [("centre", ctypes.c_double * 3), ("scale", ctypes.c_double * 3), ("cx", ctypes.c_double * 19), ("cy", ctypes.c_double * 19)]


class photon_piv_plane_t(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("pitch", ctypes.c_double), ("z", ctypes.c_double),
                ("width", ctypes.c_int), ("height", ctypes.c_int)]


class photon_piv_dewarp_t(ctypes.Structure):
    _fields_ = [("d_coef", ctypes.c_void_p), ("frame_stride", ctypes.c_longlong), ("n_frames", ctypes.c_int), ("width", ctypes.c_int),
                ("height", ctypes.c_int), ("poly", ctypes.c_double * 10 * 2), ("grid", ctypes.c_double * 4), ("out_width", ctypes.c_int),
                ("out_height", ctypes.c_int), ("out_stride", ctypes.c_longlong), ("d_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


class photon_piv_stereo_t(ctypes.Structure):
    _fields_ = [("d_field1", ctypes.c_void_p), ("d_field2", ctypes.c_void_p), ("field_stride", ctypes.c_int), ("d_flags1", ctypes.c_void_p),
                ("d_flags2", ctypes.c_void_p), ("d_sigma1", ctypes.c_void_p), ("d_sigma2", ctypes.c_void_p), ("n_rows", ctypes.c_int),
                ("n_cols", ctypes.c_int), ("win", ctypes.c_int), ("step", ctypes.c_int), ("plane", photon_piv_plane_t),
                ("camera1", photon_piv_camera_t), ("camera2", photon_piv_camera_t), ("d_out", ctypes.c_void_p), ("d_flags", ctypes.c_void_p),
                ("rows_out", ctypes.POINTER(ctypes.c_int)), ("cols_out", ctypes.POINTER(ctypes.c_int)), ("stream", ctypes.c_void_p)]


class photon_piv_triangulate_t(ctypes.Structure):
    _fields_ = [("d_disparity", ctypes.c_void_p), ("field_stride", ctypes.c_int), ("d_flags_in", ctypes.c_void_p), ("n_rows", ctypes.c_int),
                ("n_cols", ctypes.c_int), ("win", ctypes.c_int), ("step", ctypes.c_int), ("iterations", ctypes.c_int),
                ("plane", photon_piv_plane_t), ("camera1", photon_piv_camera_t), ("camera2", photon_piv_camera_t), ("d_out", ctypes.c_void_p),
                ("d_flags", ctypes.c_void_p), ("rows_out", ctypes.POINTER(ctypes.c_int)), ("cols_out", ctypes.POINTER(ctypes.c_int)),
                ("stream", ctypes.c_void_p)]


class photon_piv_volume_t(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("z0", ctypes.c_double), ("pitch", ctypes.c_double),
                ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("nz", ctypes.c_int)]


class photon_piv_volume_los_t(ctypes.Structure):
    _fields_ = [("n_cameras", ctypes.c_int), ("n_frames", ctypes.c_int), ("mode", ctypes.c_int), ("d_coef", ctypes.c_void_p * 8),
                ("frame_stride", ctypes.c_longlong * 8), ("width", ctypes.c_int * 8), ("height", ctypes.c_int * 8),
                ("grid", ctypes.c_double * 4 * 8), ("d_poly", ctypes.c_void_p), ("volume", photon_piv_volume_t),
                ("out_stride", ctypes.c_longlong), ("d_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


class photon_piv_correlate_volume_t(ctypes.Structure):
    _fields_ = [("d_vol1", ctypes.c_void_p), ("d_vol2", ctypes.c_void_p), ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("nz", ctypes.c_int),
                ("win", ctypes.c_int), ("step", ctypes.c_int), ("radius", ctypes.c_int), ("win_z", ctypes.c_int), ("step_z", ctypes.c_int),
                ("radius_z", ctypes.c_int), ("d_offset", ctypes.c_void_p), ("d_vectors", ctypes.c_void_p), ("d_flags", ctypes.c_void_p),
                ("d_planes", ctypes.c_void_p), ("n_slabs", ctypes.POINTER(ctypes.c_int)), ("n_rows", ctypes.POINTER(ctypes.c_int)),
                ("n_cols", ctypes.POINTER(ctypes.c_int)), ("stream", ctypes.c_void_p)]


class photon_piv_volume_project_t(ctypes.Structure):
    _fields_ = [("n_cameras", ctypes.c_int), ("n_frames", ctypes.c_int), ("scale_log2", ctypes.c_int), ("width", ctypes.c_int * 8),
                ("height", ctypes.c_int * 8), ("grid", ctypes.c_double * 4 * 8), ("d_poly", ctypes.c_void_p), ("volume", photon_piv_volume_t),
                ("d_vol", ctypes.c_void_p), ("vol_stride", ctypes.c_longlong), ("d_acc", ctypes.c_void_p * 8),
                ("acc_stride", ctypes.c_longlong * 8), ("d_image", ctypes.c_void_p * 8), ("stream", ctypes.c_void_p)]


class photon_piv_volume_mart_t(ctypes.Structure):
    _fields_ = [("n_cameras", ctypes.c_int), ("n_frames", ctypes.c_int), ("iterations", ctypes.c_int), ("mu_roots", ctypes.c_int),
                ("scale_log2", ctypes.c_int), ("threshold", ctypes.c_float), ("d_frame", ctypes.c_void_p * 8),
                ("frame_stride", ctypes.c_longlong * 8), ("width", ctypes.c_int * 8), ("height", ctypes.c_int * 8),
                ("grid", ctypes.c_double * 4 * 8), ("d_poly", ctypes.c_void_p), ("volume", photon_piv_volume_t),
                ("vol_stride", ctypes.c_longlong), ("d_vol", ctypes.c_void_p), ("d_mask", ctypes.c_void_p), ("d_acc", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


def _signatures():
    """(restype, argtypes) of every symbol include/parallel_ray_tracing.h declares, in the header's order.  Device and host
    arrays, handles and streams are c_void_p; a struct or a scalar the call writes through is a POINTER."""
    vp, cs, ci, cu, cf, cd = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double
    i64, u64, ll, sz, P = ctypes.c_int64, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_size_t, ctypes.POINTER
    scene = [cf, cf, P(scattering_data_struct), cs, P(lightfield_source_struct), ci, cf, cf, ci, vp, P(element_data_struct), vp, vp,
             P(camera_design_struct), cf, P(vp)]           # photon_scene_create; _from_sources: the sources after the fifth
    piv = [u64, ll, vp, vp, cd, cd, cd, vp, ci]            # seed, n, box_min, box_max, z_object, beam_fwhm, irradiance_constant, cdf, n_diameters
    grid_rays = [ci, ci, ci, vp, vp, vp, vp, ll]           # nx, ny, nz, spacing, origin, d_origins, d_dirs, n_rays
    grid_frames = grid_rays[:-1] + [vp, vp, ll]            # ..., d_dirs, d_t1, d_t2, n_rays
    solve = [cd, cd, ci, vp, P(photon_tomo_stats_t), vp]   # lambda, tol, max_iter, d_f, stats, stream
    return {
        "start_ray_tracing": (None, START_RAY_TRACING_ARGTYPES),
        "photon_set_device": (ci, [ci]),
        "photon_device_pci_bus_id": (ci, [cs, ci]),
        "photon_rand_table": (ci, [ci, vp, vp]),
        "photon_volume_load_nrrd": (ci, [cs, ci, P(vp)]),
        "photon_volume_from_density": (ci, [vp, ci, ci, ci, vp, vp, ci, P(vp)]),
        "photon_volume_info": (ci, [vp, P(photon_volume_info_t)]),
        "photon_volume_set_weight_bits": (ci, [vp, ci]),
        "photon_volume_download": (ci, [vp, ci, vp]),
        "photon_volume_sample": (ci, [vp, ci, vp, vp]),
        "photon_volume_free": (None, [vp]),
        "photon_scene_create": (ci, scene),
        "photon_scene_free": (None, [vp]),
        "photon_scene_set_noise": (ci, [vp, ci, cf, ci, cf, u64]),
        "photon_scene_set_element_train": (ci, [vp, ci]),
        "photon_scene_set_ray_order": (ci, [vp, ci]),
        "photon_scene_set_skip_doomed": (ci, [vp, ci]),
        "photon_scene_live_rays": (ci, [vp]),
        "photon_scene_live_samples": (ci, [vp, vp, ci]),
        "photon_scene_live_sources": (ll, [vp, vp, ll]),
        "photon_sources_missing_sensor": (ci, [vp, vp, ci, cf, cf, ci] + [vp] * 8 + [ll, vp]),
        "photon_scene_set_source_base": (ci, [vp, i64]),
        "photon_march_queue_group": (cu, [cu] * 4),
        "photon_march_queue_count": (cu, []),
        "photon_march_queue_chunk": (cu, [ci]),
        "photon_march_queue_size": (cu, [cu] * 4),
        "photon_scene_set_march_segments": (ci, [vp, ci]),
        "photon_march_segments_plan": (ci, [cu, ci, ci, ci, ci, P(ci)]),
        "photon_march_launch_plan": (ci, [cu] + [ci] * 8 + [P(photon_march_plan_t)]),
        "photon_trim_caches": (None, []),
        "photon_trace": (ci, [vp, vp, ci, i64, i64, vp, vp, P(photon_trace_stats_t)]),
        "photon_trace_moments": (ci, [vp, vp, ci, i64, i64, vp, vp, vp]),
        # start_ray_tracing's 29 arguments + double *source_moments (host f64[num_particles][8])
        "photon_start_ray_tracing_moments": (ci, START_RAY_TRACING_ARGTYPES + [vp]),
        "photon_scene_stats_begin": (ci, [vp, vp]),
        "photon_scene_stats_end": (ci, [vp, vp, P(photon_trace_stats_t)]),
        "photon_scene_check": (ci, [vp, vp]),
        "photon_scene_set_march_profile": (ci, [vp, ci]),
        "photon_scene_march_profile": (ci, [vp, P(photon_march_profile_t)]),
        "photon_scene_march_profile_raw": (ci, [vp, cu, vp]),
        "photon_trace_volume_rays": (ci, [vp, ci, ci, vp, vp, vp]),
        "photon_trace_volume_rays_queued": (ci, [vp, ci, ci, vp, vp, ci]),
        "photon_version": (cs, []),
        # section 3: scene generation on the device
        "photon_sources_bos": (ci, [vp, vp, ci, vp, vp, ci, cd, cd, P(vp)]),
        "photon_sources_piv": (ci, piv + [P(vp)]),
        "photon_flow_from_grid": (ci, [vp] * 3 + [ci] * 3 + [vp, vp, P(vp)]),
        "photon_flow_free": (None, [vp]),
        "photon_sources_piv_advected": (ci, piv + [vp, cd, ci, vp, P(vp)]),
        "photon_sources_count": (ll, [vp]),
        "photon_sources_download": (ci, [vp] * 6),
        "photon_sources_free": (None, [vp]),
        "photon_scene_create_from_sources": (ci, scene[:5] + [vp] + scene[5:]),
        "photon_volume_gaussian": (ci, [ci, ci, ci, vp, vp, cd, cd, vp, cd, ci, P(vp)]),
        "photon_density_gaussian_write_nrrd": (ci, [cs, ci, ci, ci, vp, vp, cd, cd, vp, cd]),
        # section 4: sensor post-processing on the device
        "photon_postprocess_u16": (ci, [vp, ci, ci, cf, ci, ci, cf, u64, ci, ci, vp, P(ci), P(ci), vp]),
        "photon_measure_copy_gbs": (ci, [sz, ci, P(cd)]),
        "photon_selftest_normal_range_math": (ci, [ci] + [vp] * 5),
        "photon_selftest_morton_order": (ci, [vp, vp, ll, ll, ll, vp]),
        "photon_selftest_fail_alloc": (ci, [ll, ll, ci]),
        "photon_selftest_alloc_stats": (ci, [P(photon_alloc_stats_t)]),
        # section 5: image-pair cross-correlation on the device
        "photon_piv_correlate": (ci, [vp, vp] + [ci] * 5 + [vp] * 4 + [P(ci), P(ci), vp]),
        # section 6: gradient-field integration on the device
        "photon_integrate_gradient": (ci, [vp] * 5 + [ci, ci, cd, cd, cd, ci, vp, P(photon_integrate_stats_t), vp]),
        # section 7: iterative image-deformation correlation
        "photon_piv_bspline_coefficients": (ci, [vp, ci, ci, vp, vp]),
        "photon_piv_deform": (ci, [vp, ci, ci, vp] + [ci] * 5 + [cf, vp, vp]),
        "photon_piv_validate": (ci, [vp] * 3 + [ci, ci, cd, cd] + [vp] * 4),
        # section 8: dot tracking
        "photon_dots_detect_scratch_bytes": (sz, [ci, ci]),
        "photon_dots_match_scratch_bytes": (sz, [ci, ci, cf, ci, ci]),
        "photon_dots_image_max": (ci, [vp, ci, ci, vp, vp]),
        "photon_dots_detect": (ci, [vp, ci, ci, cf, vp, ci, vp, vp, vp, sz, vp]),
        "photon_dots_fit": (ci, [vp, ci, ci, vp, vp, ci, ci, cd, ci, cd, vp, vp, vp]),
        "photon_dots_match": (ci, [vp, vp, vp, ci, vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, cf, ci, ci, vp, vp, vp, vp, sz, vp]),
        "photon_dots_window_means": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]),
        # section 9: tomography
        "photon_tomo_project": (ci, [vp] + grid_rays + [vp, vp]),
        "photon_tomo_backproject": (ci, [vp] + grid_rays + [vp, vp]),
        "photon_tomo_reconstruct": (ci, [vp, vp, vp] + grid_rays + solve),
        # section 10: tomography from deflections
        "photon_tomo_deflect": (ci, [vp] + grid_frames + [vp, vp, vp]),
        "photon_tomo_deflect_adjoint": (ci, [vp, vp] + grid_frames + [vp, vp]),
        "photon_tomo_reconstruct_deflections": (ci, [vp, vp, vp, vp] + grid_frames + solve),
        # section 11: displacement uncertainty from correlation statistics
        "photon_piv_uncertainty": (ci, [vp, vp] + [ci] * 5 + [vp] * 3 + [P(ci), P(ci), vp]),
        # section 12: dense optical flow
        "photon_piv_field_to_pixels": (ci, [vp] + [ci] * 7 + [vp, vp]),
        "photon_piv_deform_dense": (ci, [vp, ci, ci, vp, cf, vp, vp]),
        "photon_optflow_terms": (ci, [vp, vp, ci, ci, vp, cf, cf, vp, vp]),
        "photon_optflow_iterate": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
        "photon_optflow_iterations_per_launch": (ci, []),
        # section 13: FFT correlation (circular / phase)
        "photon_piv_correlate_phase": (ci, [vp, vp] + [ci] * 5 + [vp, ci, cf, cf] + [vp] * 3 + [P(ci), P(ci), vp]),
        "photon_piv_phase_tables": (ci, [ci, cf, cf, vp, vp, vp]),
        # section 14: ensemble correlation
        "photon_piv_correlate_ensemble": (ci, [vp, vp, ll] + [ci] * 6 + [vp] * 5 + [P(ci), P(ci), vp]),
        # section 15: image pre-processing
        "photon_piv_background": (ci, [vp, ll, ci, ci, ci, ci, vp, vp]),
        "photon_piv_background_path": (ci, [vp, ll, vp]),
        "photon_piv_preprocess": (ci, [vp, ll, ci, ci, ci, vp, ci, cf, vp, ll, vp]),
        # section 16: a field from one window grid to another
        "photon_piv_regrid": (ci, [vp] + [ci] * 9 + [vp, P(ci), P(ci), vp]),
        # section 17: direct correlation with excluded pixels
        "photon_piv_correlate_masked": (ci, [vp] * 4 + [ci] * 6 + [vp] * 5 + [P(ci), P(ci), vp]),
        # section 18: direct correlation with a weight per window pixel
        "photon_piv_correlate_weighted": (ci, [vp] * 3 + [ci] * 5 + [vp] * 4 + [P(ci), P(ci), vp]),
        "photon_piv_window_weights": (ci, [ci, ci, cf, vp]),
        # section 19: stereo PIV (one job struct each; its last member is the stream)
        "photon_piv_dewarp": (ci, [P(photon_piv_dewarp_t)]),
        "photon_piv_stereo_reconstruct": (ci, [P(photon_piv_stereo_t)]),
        "photon_piv_stereo_triangulate": (ci, [P(photon_piv_triangulate_t)]),
        # section 20: tomographic PIV (job structs as section 19's)
        "photon_piv_volume_los": (ci, [P(photon_piv_volume_los_t)]),
        "photon_piv_correlate_volume": (ci, [P(photon_piv_correlate_volume_t)]),
        # section 21: MART particle volumes (job structs as section 20's)
        "photon_piv_volume_project": (ci, [P(photon_piv_volume_project_t)]),
        "photon_piv_volume_mart": (ci, [P(photon_piv_volume_mart_t)]),
    }


SIGNATURES = _signatures()
DECLARED_SYMBOLS = tuple(SIGNATURES)    # every symbol include/parallel_ray_tracing.h declares


def apply_signatures(cdll):
    """Declare the types of every header symbol `cdll` exports (a ctypes.CDLL; returned).  A symbol it lacks is skipped:
    builds from before an entry point existed load the same way (A/B runs through PHOTON_LIBRARY)."""
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(cdll, name):
            f = getattr(cdll, name)
            f.restype, f.argtypes = restype, list(argtypes)
    return cdll


class PhotonError(RuntimeError):
    pass


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _vp(ptr: int):
    """A raw pointer or a stream as the C side takes it (0 = NULL)."""
    return ctypes.c_void_p(int(ptr)) if ptr else None


def _f64x3(v, scalar_ok: bool = False):
    """v as contiguous f64 for a `const double[3]` argument; scalar_ok: one value stands for all three."""
    v = np.asarray(v, np.float64)
    return np.ascontiguousarray(np.broadcast_to(v, (3,)) if scalar_ok else v)


def _dims(n):
    """n or (nx, ny, nz) as three ints."""
    nx, ny, nz = (n, n, n) if np.isscalar(n) else n
    return int(nx), int(ny), int(nz)


def _stereo_job(cameras, plane, win: int, step: int, kind=photon_piv_stereo_t):
    """Section 19b's job (kind photon_piv_triangulate_t: 19c's) with its host values -- the two cameras and the plane
    (piv_stereo's dicts), win and step -- and every pointer NULL: as it stands, the size query."""
    job = kind(win=int(win), step=int(step))
    job.plane = photon_piv_plane_t(float(plane["x0"]), float(plane["y0"]), float(plane["pitch"]), float(plane["z"]), int(plane["width"]),
                                   int(plane["height"]))
    if len(cameras) != 2:
        raise ValueError("section 19 takes two cameras")
    for name, cam in zip(("camera1", "camera2"), cameras):
        c = getattr(job, name)
        for key, n in (("centre", 3), ("scale", 3), ("cx", 19), ("cy", 19)):
            v = np.ascontiguousarray(cam[key], np.float64)
            if v.shape != (n,):
                raise ValueError(f"a camera's {key} must have {n} values, not shape {v.shape}")
            ctypes.memmove(getattr(c, key), v.ctypes.data, v.nbytes)
    return job


def _gaussian_args(n, spacing, origin, rho0, amp, centre, sigma):
    """What volume_gaussian and density_gaussian_write_nrrd share: the grid, then the field (_ptr keeps its array alive)."""
    return (*_dims(n), _ptr(_f64x3(spacing, scalar_ok=True)), _ptr(_f64x3(origin)), float(rho0), float(amp), _ptr(_f64x3(centre)),
            float(sigma))


def _piv_args(seed, n, box_min, box_max, z_object, beam_fwhm, irradiance_constant, diameter_cdf):
    """What sources_piv and sources_piv_advected share: seed, count, box, sheet and the diameter CDF (None = NULL, 0)."""
    cdf = None if diameter_cdf is None else np.ascontiguousarray(diameter_cdf, dtype=np.float64)
    return (int(seed), int(n), _ptr(_f64x3(box_min)), _ptr(_f64x3(box_max)), float(z_object), float(beam_fwhm),
            float(irradiance_constant), None if cdf is None else _ptr(cdf), 0 if cdf is None else int(cdf.size))


def _checked(x, name: str, ndim=None):
    """The first half of the drivers' ingest rule (PhotonLibrary's docstring), on the host alone: `x` as the caller's torch
    tensor or as a base-class numpy array (np.asarray: memmaps, lists, scalars' sequences), or the refusal that names
    the argument -- TypeError for a dtype that is not real numeric or bool (complex, object, strings), ValueError for
    what numpy cannot make an array of and for a number of dimensions other than `ndim` (None: any).  Nothing is copied,
    allocated or launched; None stays None."""
    import sys
    if x is None:
        return None
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(x, torch.Tensor):
        if x.is_complex():
            raise TypeError(f"{name} must hold real numbers, not {x.dtype}")
        a = x
    else:
        try:
            a = np.asarray(x)
        except ValueError as e:
            raise ValueError(f"{name} is not an array: {e}") from e
        if a.dtype.kind not in "biuf":
            raise TypeError(f"{name} must hold real numbers, not dtype {a.dtype}")
    if ndim is not None and a.ndim != int(ndim):
        raise ValueError(f"{name} must have {int(ndim)} dimensions, not {a.ndim} (shape {tuple(a.shape)})")
    return a


def _on_device(x, dtype, dev, name: str = "array", ndim=None, nonzero: bool = False):
    """The drivers' ingest rule (PhotonLibrary's docstring), the one way a caller's array reaches the device: `x` (what
    _checked accepts; None stays None) as a contiguous torch tensor of the torch dtype `dtype` on `dev` that holds
    np.asarray(x).astype(dtype) in C order -- numpy's conversion, made on the host for whatever lives there; a device
    tensor is converted where it is, by the same round-to-nearest.  nonzero: the value is (x != 0) instead, the masks'
    reading.  A tensor that is already of `dtype`, contiguous and on `dev` is returned as it is, uncopied (nonzero: never);
    no driver writes to what this returns.  The caller's object is never written and no warning is raised: a read-only
    or foreign-endian array is copied on the host first."""
    import torch
    a = _checked(x, name, ndim)
    if a is None:
        return None
    dev = torch.device(dev)
    if isinstance(a, torch.Tensor):
        a = a.detach()
        if a.device.type != "cpu":
            if nonzero:
                return (a.to(device=dev) != 0).to(dtype).contiguous()
            if a.dtype == dtype and a.device == dev and a.is_contiguous():
                return a
            return a.to(device=dev, dtype=dtype).contiguous()
        if dev.type == "cpu" and a.dtype == dtype and a.is_contiguous() and not nonzero:
            return a
        if a.dtype == torch.bfloat16:
            a = a.to(torch.float32)                     # numpy has no bfloat16; every bfloat16 is an f32
        a = a.numpy()                                   # strides and all; converted below as numpy does
    if nonzero:
        a = a != 0
    targets = {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8}       # what the drivers ask for
    c = np.ascontiguousarray(a, dtype=targets[dtype])   # native byte order, C order, positive strides
    if not c.flags.writeable:
        c = c.copy()            # torch warns about tensors over read-only memory
    return torch.from_numpy(c).to(device=dev)


def _current_device():
    """torch's current device: where every wrapper that allocates its own outputs puts them."""
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _device_and_stream():
    """torch's current device and the raw handle of its current stream: where every pipeline allocates and runs."""
    import torch
    dev = _current_device()
    return dev, torch.cuda.current_stream(dev).cuda_stream


def _checked_mask(mask, shape):
    """The drivers' mask= (piv_mask.mask_pair: one plane, or a tuple or list of two) checked on the host against the image
    shape (height, width): the tuple of its one or two planes as _checked returns them.  None stays None."""
    if mask is None:
        return None
    two = isinstance(mask, (tuple, list)) and len(mask) == 2
    pair = tuple(_checked(m, "mask", 2) for m in (mask if two else (mask,)))
    for m in pair:
        if tuple(m.shape) != tuple(int(v) for v in shape):
            raise ValueError(f"a mask of shape {tuple(m.shape)} does not cover a {shape[0]} x {shape[1]} image")
    return pair


def _checked_pair(im1, im2, mask=None):
    """Every refusal of an image pair and its mask=, on the host, before anything is allocated or queued: (a, b, mask) as
    _checked and _checked_mask return them."""
    a, b = _checked(im1, "im1", 2), _checked(im2, "im2", 2)
    if a is None or b is None:
        raise TypeError("im1 and im2 must be two images, not None")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"im1 and im2 must be two 2-d images of one shape, not {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b, _checked_mask(mask, a.shape)


def _image_pair(im1, im2):
    """(dev, stream, a, b, h, w): the two images, checked (_checked_pair), as contiguous f32 device tensors [h, w] on the
    current device."""
    a, b, _ = _checked_pair(im1, im2)
    return _pair_on_device(a, b)


def _pair_on_device(a, b):
    """_image_pair's device half, for the two images as _checked_pair returned them: the drivers with a mask= or a
    weighting= raise their other refusals between the two."""
    import torch
    dev, stream = _device_and_stream()
    a, b = _on_device(a, torch.float32, dev, "im1", 2), _on_device(b, torch.float32, dev, "im2", 2)
    return (dev, stream, a, b, *a.shape)


def _mask_pair(mask, shape, dev):
    """The drivers' mask= (piv_mask.mask_pair: one plane, or a tuple or list of two) as two contiguous u8 device tensors
    [h, w], 1 = excluded; one tensor twice for one plane."""
    import torch
    out = tuple(_on_device(m, torch.uint8, dev, "mask", 2, nonzero=True) for m in _checked_mask(mask, shape))
    return out[0], out[-1]


def _checked_weighting(weighting):
    """The drivers' weighting= on the host: the named forms as they are, an array [win, win] as a numpy array that _checked
    passed (a device tensor is copied back: piv_weighting.check_weights reads every weight before any table is made)."""
    if weighting is None or isinstance(weighting, str) or (isinstance(weighting, (tuple, list)) and len(weighting) == 2
                                                           and isinstance(weighting[0], str)):
        return weighting
    a = _checked(weighting, "weighting", 2)
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _weight_tables(tables, dev):
    """The drivers' weighting= on the device: `tables` {win: f32 table [win, win]}, what piv_weighting.resolve made of it for
    every window size (_Correlator), as {win: contiguous f32 device tensor [win, win]}; None stays None."""
    import torch
    return None if tables is None else {win: _on_device(t, torch.float32, dev, "weighting", 2) for win, t in tables.items()}


def _nan_where_masked_out(x, status):
    """The device tensor x [n_rows, n_cols, k] with NaN where status [n_rows, n_cols] has bit 16, the masked-out nodes
    (piv_mask.fill_masked); queued on the current stream, nothing waits."""
    import torch
    return torch.where(((status & 16) != 0)[..., None], torch.full((), float("nan"), dtype=x.dtype, device=x.device), x)


def _checked_passes(passes) -> int:
    if int(passes) not in (1, 2):
        raise ValueError(f"passes must be 1 or 2, not {passes}")
    return int(passes)


def _two_passes(correlate, passes: int, dev):
    """What correlate and correlate_ensemble share behind their first pass.  correlate(d_offset_ptr) -> (vec, flg, ...), device
    tensors: pass 1 without offsets; passes == 2: the normalised median test and the predictor on the host
    (photon_amd.piv_correlation), then pass 2 with the integer window offsets.  Returns (vectors, flags, what the last pass
    returned), the first two as numpy."""
    import torch
    from . import piv_correlation as pc
    out = correlate(0)
    vectors, flags = out[0].cpu().numpy(), out[1].cpu().numpy()
    if passes == 2:
        offsets = pc.predictor(vectors, flags, pc.normalized_median_test(vectors))
        d_off = torch.from_numpy(offsets).to(dev)
        out = correlate(d_off.data_ptr())
        vectors, flags = out[0].cpu().numpy(), out[1].cpu().numpy()
    return vectors, flags, out


def _replace_masked(im, m):
    """piv_mask.replace_masked on the device, queued on the current stream: the frame with its masked pixels at the mean of
    the unmasked ones."""
    import torch
    hidden = m != 0
    free = torch.where(hidden, torch.zeros((), dtype=im.dtype, device=im.device), im)
    return torch.where(hidden, free.sum() / (im.numel() - hidden.sum()).clamp(min=1), im).contiguous()


class _DeformSettings(NamedTuple):
    """What the deformation chain takes besides its correlator: pass 0's radius (None: the correlator's default), the
    iterations' radius, whether the smoothed field is the next predictor, and photon_piv_validate's eps and threshold.
    The defaults are the drivers'."""
    radius: Optional[int] = None
    residual_radius: int = 4
    smooth: bool = True
    eps: float = 0.1
    threshold: float = 2.0


class _Correlator:
    """What the drivers' method=, window_sigma=, diameter=, mask=, min_valid_fraction= and weighting= select, for the window
    sizes `wins` a driver will correlate with, resolved in two steps.
    The host step, the constructor, raises every refusal and touches no device: mask= and weighting= need "direct" and
    exclude each other (piv_mask.check_method, piv_weighting.check_method), weighting= is one of piv_weighting.resolve's
    forms with a table for every win, method is "direct" or "phase", min_valid_fraction lies in (0, 1].  The mask's planes
    are checked with the images, by _checked_pair, before.
    The device step, on_device, brings the masks (_mask_pair) and one weight table per win (_weight_tables) over and binds
    the library.  After it, at(win, radius) answers with (a callable with piv_correlate's signature, the radius, the
    argument check): "direct" is section 5, radius None = win // 2; with a mask section 17 with the two masks and
    min_valid = ceil(min_valid_fraction win^2) bound; with weighting section 18 with win's table bound; "phase" is
    section 13's mode 1 with window_sigma (None = win / 4) and diameter bound, radius None or win // 2 = win // 2 - 1."""

    def __init__(self, wins, method: str = "direct", window_sigma: Optional[float] = None, diameter: float = 2.5, mask=None,
                 min_valid_fraction: float = 0.5, weighting=None):
        from . import piv_mask
        from . import piv_weighting as pw
        piv_mask.check_method(method, mask)
        pw.check_method(method, weighting, mask)
        weighting = _checked_weighting(weighting)
        if method not in ("direct", "phase"):
            raise ValueError(f'method must be "direct" or "phase", not {method!r}')
        self.method, self.window_sigma, self.diameter, self.mask = method, window_sigma, diameter, mask
        self.min_valid = None if mask is None else {int(win): piv_mask.min_valid_for(win, min_valid_fraction) for win in wins}
        self.tables = None if weighting is None else {int(win): pw.resolve(weighting, win) for win in wins}
        self.lib = None

    def on_device(self, lib, shape, dev):
        """The device step for images of `shape` on `dev`; returns the correlator."""
        self.lib = lib
        if self.mask is not None:
            self.mask = _mask_pair(self.mask, shape, dev)
        self.tables = _weight_tables(self.tables, dev)
        return self

    def at(self, win: int, radius=None):
        lib = self.lib
        if self.method == "phase":
            from . import piv_phase as pp
            sigma, diameter = int(win) / 4.0 if self.window_sigma is None else float(self.window_sigma), self.diameter

            def correlate(*args, **kwargs):
                return lib.piv_correlate_phase(*args, mode=pp.MODE_PHASE, window_sigma=sigma, diameter=float(diameter), **kwargs)

            def check(shape, win, step, radius):
                pp.check_arguments(shape, win, step, radius, pp.MODE_PHASE, sigma, diameter)
            return correlate, pp.default_radius(win, radius), check
        correlate = lib.piv_correlate
        if self.tables is not None:
            table = self.tables[int(win)]

            def correlate(d_im1_ptr, d_im2_ptr, width, height, win, step, radius, d_offset_ptr=0, planes=False, stream=0):
                return lib.piv_correlate_weighted(d_im1_ptr, d_im2_ptr, table.data_ptr(), width, height, win, step, radius, d_offset_ptr,
                                                  planes, stream)
        elif self.mask is not None:
            (m1, m2), min_valid = self.mask, self.min_valid[int(win)]

            def correlate(d_im1_ptr, d_im2_ptr, width, height, win, step, radius, d_offset_ptr=0, planes=False, stream=0):
                return lib.piv_correlate_masked(d_im1_ptr, d_im2_ptr, m1.data_ptr(), m2.data_ptr(), width, height, win, step, radius,
                                                min_valid, d_offset_ptr, planes, False, stream)[:3]
        from . import piv_correlation as pc
        return correlate, (int(win) // 2 if radius is None else int(radius)), pc.check_arguments


# the outputs of the window correlators as _grid_call takes them
_VECTORS, _FLAGS = ((4,), "float32", True), ((), "int32", True)


def _planes(radius: int, asked: bool):
    return (2 * int(radius) + 1,) * 2, "float32", asked


def bind_march_launch_plan(lib):
    """photon_march_launch_plan of a loaded library (host arithmetic: needs no GPU), as
    f(n_rays, dims, algorithm, interpolation, num_cus=256, scene_segments=-1, flags=0) -> photon_march_plan_t."""
    f = lib.photon_march_launch_plan
    f.restype, f.argtypes = SIGNATURES["photon_march_launch_plan"]

    def plan(n_rays, dims, algorithm, interpolation, num_cus=256, scene_segments=-1, flags=0):
        out = photon_march_plan_t(struct_size=ctypes.sizeof(photon_march_plan_t))
        rc = f(int(n_rays), *_dims(dims), int(algorithm), int(interpolation), int(num_cus), int(scene_segments), int(flags),
               ctypes.byref(out))
        if rc != 0:
            raise PhotonError(f"photon_march_launch_plan failed with code {rc} (see stderr)")
        return out
    return plan


def _one_hip_runtime_per_process():
    """PyTorch-ROCm bundles its own libamdhip64; the library's RUNPATH names the system's.  A process that ends up with
    both mapped has two HIP runtimes, and whichever touches the GPU second finds no device (seen both ways round on
    the MI355X boxes).  Whoever shares torch device tensors with the library (this repo's tests, bench.py, smoke())
    therefore imports torch FIRST, explicitly: the library then binds to torch's copy by SONAME.  The library itself
    never imports torch behind the caller's back -- photon's own Python has none and gets the system runtime the library
    was built against.  PHOTON_PRELOAD_TORCH=1 asks for the import here (a caller that cannot order its imports)."""
    import sys
    if "torch" in sys.modules or not os.environ.get("PHOTON_PRELOAD_TORCH"):
        return
    try:
        import torch  # noqa: F401
    except Exception:       # noqa: BLE001  -- a broken torch must not keep the library from loading
        pass


def mapped_hip_runtimes():
    """Paths of every libamdhip64 mapped into this process (more than one = the two-runtime trap above)."""
    found = []
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                path = ln.rsplit(" ", 1)[-1].strip()
                if "libamdhip64" in path and path not in found:
                    found.append(path)
    except OSError:
        pass
    return found


class PhotonLibrary:
    """The loaded library: one method per entry point (raw device pointers) and the drivers that chain them.

    The ingest rule -- how every driver takes an array argument (images, stacks, masks, weights, fields, predictors,
    gradients, solver data, rays), through _on_device alone:
      * accepted: a numpy array or whatever np.asarray takes (a memmap, nested lists), of any real numeric or bool dtype, any
        byte order, any strides (views, crops, Fortran order, np.flipud / np.rot90 / a[::-1]), writable or read-only; a torch
        tensor on any device, of any real dtype, with any strides;
      * the value: the device tensor holds np.asarray(x).astype(target) -- numpy's conversion, round to nearest -- in C order,
        target f32 for images, stacks, fields and weights, f64 for gradients, solver data and rays; a mask (mask=, fixed=,
        support=) holds x != 0.  Integer frames (uint8 / uint16 camera counts) are taken as they are, no scaling.  No warning
        is raised and the caller's array is never written;
      * refused: complex, object and string dtypes with a TypeError, what numpy makes no array of and a wrong number of
        dimensions with a ValueError; the message names the argument, and the refusal -- like that of two images of
        different shapes or a mask of another shape -- comes before anything is allocated or queued on the device;
      * device tensors: one that is already of the target dtype, contiguous and on the current device is used in place,
        uncopied, so work queued on the current stream that fills it is waited for by the driver's kernels and by nothing
        else; every other tensor is converted on its device, on the current stream.  No driver writes to an input, and no
        result shares storage with one."""

    def __init__(self, path: Optional[str] = None, build: bool = True):
        if path is None:
            path = os.environ.get("PHOTON_LIBRARY")
            if not path:                    # the in-tree library: (re)built when missing or older than its sources
                path = _build.LIB_PATH
                if build:
                    try:
                        _build.build_library(verbose=False)
                    except Exception as e:  # no hipcc on this box: a library that travelled with the tree is used as is
                        if not os.path.exists(path):
                            raise PhotonError(f"cannot build {path}: {e}") from e
        if not os.path.exists(path):
            raise PhotonError(f"{path} not found: build it with `python -m photon_amd.build` "
                              "(there is no CPU fallback)")
        self.path = path
        _one_hip_runtime_per_process()
        self.lib = L = apply_signatures(ctypes.CDLL(path))
        self.hip_runtimes = mapped_hip_runtimes()
        if os.environ.get("PHOTON_VERBOSE") or len(self.hip_runtimes) > 1:
            import sys
            print(f"photon: {path} runs on {', '.join(self.hip_runtimes) or 'an unidentified HIP runtime'}"
                  + (" -- TWO HIP runtimes in one process: import torch before the library" if len(self.hip_runtimes) > 1 else ""),
                  file=sys.stderr)
        self.start_ray_tracing = L.start_ray_tracing
        self.start_ray_tracing_moments = L.photon_start_ray_tracing_moments       # returns 0 or non-zero
        self.has_stats_window = hasattr(L, "photon_scene_stats_begin")     # absent from libraries built before round 3 (A/B runs)
        if hasattr(L, "photon_march_launch_plan"):                           # absent from older libraries (A/B runs)
            self.march_launch_plan = bind_march_launch_plan(L)
        self.has_march_profile = hasattr(L, "photon_scene_march_profile")  # round 4

    # ---- helpers --------------------------------------------------------------------------
    @staticmethod
    def _check(rc: int, what: str):
        if rc != 0:
            raise PhotonError(f"{what} failed with code {rc} (see stderr)")

    def _call(self, entry: str, *args):
        """One call of an entry point that returns 0 or an error code."""
        self._check(getattr(self.lib, entry)(*args), entry)

    def _grid_call(self, entry: str, head, outputs, stream: int, offset=(), after_offset=()):
        """An entry point that sizes its own window grid: the query with NULL outputs for (n_rows, n_cols), the outputs allocated
        on the current device, then the launch on `stream`.  head: the arguments before d_offset; offset: (d_offset_ptr,), NULL
        in the query, or () for an entry without one; after_offset: the arguments between it and the outputs.  outputs: per
        output of the entry, in its order, (the shape after [n_rows, n_cols], the torch dtype's name, whether the caller asked
        for it).  Returns the tuple of device tensors, None where not asked for, filled asynchronously."""
        import torch
        rows, cols = ctypes.c_int(0), ctypes.c_int(0)
        self._call(entry, *head, *[None] * len(offset), *after_offset, *[None] * len(outputs), ctypes.byref(rows), ctypes.byref(cols), None)
        dev, grid = _current_device(), (rows.value, cols.value)
        made = [torch.empty(grid + shape, dtype=getattr(torch, dtype), device=dev) if asked else None for shape, dtype, asked in outputs]
        pointers = [None if t is None else _vp(t.data_ptr()) for t in made]
        self._call(entry, *head, *[_vp(p) for p in offset], *after_offset, *pointers, None, None, _vp(stream))
        return tuple(made)

    def version(self) -> str:
        return self.lib.photon_version().decode()

    def set_device(self, device: int):
        self._call("photon_set_device", int(device))

    def rand_table(self, n: int):
        r1 = np.empty(n, np.float32)
        r2 = np.empty(n, np.float32)
        self._call("photon_rand_table", n, _ptr(r1), _ptr(r2))
        return r1, r2

    def fail_alloc(self, first: int, count: int = 1, first_attempt_only: bool = False):
        """photon_selftest_fail_alloc: device allocation requests first .. first + count - 1 from now fail (0 disarms)."""
        self._call("photon_selftest_fail_alloc", int(first), int(count), int(bool(first_attempt_only)))

    def alloc_stats(self) -> dict:
        """photon_selftest_alloc_stats: requests, injected failures, retries, cached and outstanding blocks of this process."""
        st = photon_alloc_stats_t()
        self._call("photon_selftest_alloc_stats", ctypes.byref(st))
        return st.as_dict()

    def morton_order(self, x, y, first: int = 0, n: Optional[int] = None):
        """photon_selftest_morton_order: the spatial order of sources first .. first + n - 1, as the device computes it."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        n = x.size - first if n is None else int(n)
        out = np.empty(n, np.int32)
        self._call("photon_selftest_morton_order", _ptr(x), _ptr(y), int(x.size), int(first), n, _ptr(out))
        return out

    def sources_missing_sensor(self, call: RayTracingCall, lens_x, lens_y):
        """photon_sources_missing_sensor (host arithmetic, no GPU needed): bool[num_sources], True = no ray of that source
        through any of the given lens samples can reach a pixel; None when the call's geometry is not covered."""
        sd, ls, elems, centers, planes, sysidx, cam = call.pack()
        lx = np.ascontiguousarray(lens_x, np.float32)
        ly = np.ascontiguousarray(lens_y, np.float32)
        x, y, z = (np.ascontiguousarray(a, np.float32) for a in (call.src_x, call.src_y, call.src_z))
        off = np.zeros(x.size, np.uint8)
        rc = self.lib.photon_sources_missing_sensor(
            _ptr(lx), _ptr(ly), int(lx.size), float(call.image_distance), float(call.beam_wavelength), len(call.elements),
            ctypes.cast(elems, ctypes.c_void_p), _ptr(centers), _ptr(planes), _ptr(sysidx), ctypes.addressof(cam), _ptr(x), _ptr(y), _ptr(z),
            int(x.size), _ptr(off))
        if rc == 1:
            return None
        self._check(rc, "photon_sources_missing_sensor")
        return off.astype(bool)

    # ---- the reference's entry point ----------------------------------------------------------
    def render(self, call: RayTracingCall, image: Optional[np.ndarray] = None) -> np.ndarray:
        """One start_ray_tracing call (host image in, host image out)."""
        if image is None:
            image = call.new_image()
        call.invoke(self.start_ray_tracing, image)
        return image

    def render_moments(self, call: RayTracingCall, image: Optional[np.ndarray] = None):
        """start_ray_tracing plus the per-source sensor moments (photon_start_ray_tracing_moments): returns (image, records),
        records f64[num_sources][8] in the layout of photon_amd.deflections.RECORD_FIELDS."""
        if image is None:
            image = call.new_image()
        records = np.zeros((call.num_sources, 8), np.float64)
        status = []
        call.invoke(lambda *args: status.append(self.start_ray_tracing_moments(*args)), image, extra=(_ptr(records),))
        self._check(status[0], "photon_start_ray_tracing_moments")
        return image, records

    def pci_bus_id(self) -> str:
        """PCI bus id of the current device, lower case as sysfs spells it ('0000:c1:00.0'); '' if unavailable."""
        if not hasattr(self.lib, "photon_device_pci_bus_id"):
            return ""
        buf = ctypes.create_string_buffer(64)
        return buf.value.decode().lower() if self.lib.photon_device_pci_bus_id(buf, 64) == 0 else ""

    def measure_copy_gbs(self, nbytes: int = 1 << 30, reps: int = 5) -> float:
        """Device-to-device float4 copy rate (read + write), GB/s."""
        out = ctypes.c_double(0.0)
        self._call("photon_measure_copy_gbs", int(nbytes), int(reps), ctypes.byref(out))
        return out.value

    # ---- sensor post-processing on the device (perform_ray_tracing_03.py:2190-2259) -----------------
    def postprocess_u16(self, d_image_ptr: int, width: int, height: int, d_out_ptr: int, pixel_gain: float,
                        pixel_bit_depth: int, intensity_rescaling: bool = True, image_noise: float = 0.0, noise_seed: int = 0,
                        crop_rows: int = 0, crop_cols: int = 0, stream: int = 0):
        """Device f32 image -> device uint16 picture (raw pointers); returns (rows, cols) of the result."""
        r, c = ctypes.c_int(0), ctypes.c_int(0)
        self._call("photon_postprocess_u16", _vp(d_image_ptr), int(width), int(height), float(pixel_gain), int(pixel_bit_depth),
                   int(bool(intensity_rescaling)), float(image_noise), int(noise_seed), int(crop_rows), int(crop_cols), _vp(d_out_ptr),
                   ctypes.byref(r), ctypes.byref(c), _vp(stream))
        return r.value, c.value

    # ---- image-pair cross-correlation on the device (photon_piv_correlate) ------------------------------
    def piv_correlate(self, d_im1_ptr: int, d_im2_ptr: int, width: int, height: int, win: int, step: int, radius: int,
                      d_offset_ptr: int = 0, planes: bool = False, stream: int = 0):
        """Correlate two device f32 images (raw pointers, row-major height x width) window by window; d_offset_ptr: device
        int32 [n][2] integer offsets, or 0.  Returns torch device tensors (vectors [n_rows, n_cols, 4] = dx, dy, peak,
        ratio; flags [n_rows, n_cols] int32; planes [n_rows, n_cols, 2R+1, 2R+1] or None), filled asynchronously on
        `stream`.  The definition: include/parallel_ray_tracing.h, section 5 (photon_amd.piv_correlation: host model)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), int(width), int(height), int(win), int(step), int(radius))
        return self._grid_call("photon_piv_correlate", head, (_VECTORS, _FLAGS, _planes(radius, planes)), stream, (d_offset_ptr,))

    def piv_correlate_phase(self, d_im1_ptr: int, d_im2_ptr: int, width: int, height: int, win: int, step: int, radius: int,
                            d_offset_ptr: int = 0, planes: bool = False, stream: int = 0, mode: int = 1, window_sigma: float = 0.0,
                            diameter: float = 0.0):
        """photon_piv_correlate_phase on raw device pointers: piv_correlate's arguments and results, by FFT -- mode 0 the
        circular cross-correlation, mode 1 the phase correlation -- of windows weighted by a Gaussian of `window_sigma` px
        (0: none), with the spectral filter for particles of e^-2 diameter `diameter` px (0: none).  The definition:
        include/parallel_ray_tracing.h, section 13 (photon_amd.piv_phase: host models)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), int(width), int(height), int(win), int(step), int(radius))
        return self._grid_call("photon_piv_correlate_phase", head, (_VECTORS, _FLAGS, _planes(radius, planes)), stream, (d_offset_ptr,),
                               after_offset=(int(mode), float(window_sigma), float(diameter)))

    def piv_phase_tables(self, win: int, window_sigma: float, diameter: float):
        """photon_piv_phase_tables: the library's own (twiddles f32 [win/2, 2], window f32 [win], filter f32 [win]) for
        section 13, host arrays; needs no GPU."""
        n = max(int(win), 2)
        tw, g, w = np.zeros((n // 2, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._call("photon_piv_phase_tables", int(win), float(window_sigma), float(diameter), _ptr(tw), _ptr(g), _ptr(w))
        return tw, g, w

    def piv_correlate_masked(self, d_im1_ptr: int, d_im2_ptr: int, d_mask1_ptr: int, d_mask2_ptr: int, width: int, height: int, win: int,
                             step: int, radius: int, min_valid: int = 1, d_offset_ptr: int = 0, planes: bool = False, valid: bool = True,
                             stream: int = 0):
        """photon_piv_correlate_masked on raw device pointers: piv_correlate's arguments and results with two u8 masks
        [height, width] (nonzero = excluded; 0 = NULL, nothing excluded; they may be one pointer) and the fewest valid pixels
        a window may keep.  Returns (vectors, flags, planes or None, valid int32 [n_rows, n_cols, 2] = (n_a, n_b) or None),
        filled asynchronously on `stream`; flags carry bit 16 (masked out: every output NaN) and bit 32 (partially masked:
        the overlap-normalised plane).  The definition: include/parallel_ray_tracing.h, section 17 (photon_amd.piv_mask:
        host model)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), _vp(d_mask1_ptr), _vp(d_mask2_ptr), int(width), int(height), int(win), int(step), int(radius),
                int(min_valid))
        outputs = (_VECTORS, _FLAGS, ((2,), "int32", valid), _planes(radius, planes))
        vectors, flags, val, pl = self._grid_call("photon_piv_correlate_masked", head, outputs, stream, (d_offset_ptr,))
        return vectors, flags, pl, val

    def piv_correlate_weighted(self, d_im1_ptr: int, d_im2_ptr: int, d_weight_ptr: int, width: int, height: int, win: int, step: int,
                               radius: int, d_offset_ptr: int = 0, planes: bool = False, stream: int = 0):
        """photon_piv_correlate_weighted on raw device pointers: piv_correlate's arguments and results with a device f32 table
        [win, win] of weights on frame 1's window (row y, column x; entries that are not above 0 count as 0), one table for all
        windows.  A table of ones returns piv_correlate's bits.  The definition: include/parallel_ray_tracing.h, section 18
        (photon_amd.piv_weighting: host model and tables)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), _vp(d_weight_ptr), int(width), int(height), int(win), int(step), int(radius))
        return self._grid_call("photon_piv_correlate_weighted", head, (_VECTORS, _FLAGS, _planes(radius, planes)), stream, (d_offset_ptr,))

    def piv_window_weights(self, win: int, kind: str = "gaussian", sigma: Optional[float] = None) -> np.ndarray:
        """photon_piv_window_weights: the library's own table f32 [win, win] for section 18 ("uniform", or "gaussian" with
        sigma pixels, None = win / 4), a host array; needs no GPU.  photon_amd.piv_weighting.window_weights is the same
        table."""
        from . import piv_weighting as pw
        if kind not in pw.KINDS:
            raise ValueError(f'kind must be "uniform" or "gaussian", not {kind!r}')
        n = max(int(win), 1)
        out = np.zeros((n, n), np.float32)
        self._call("photon_piv_window_weights", int(win), pw.KINDS[kind], float(pw.default_sigma(win) if sigma is None else sigma), _ptr(out))
        return out

    def correlate(self, im1, im2, win: int = 32, step: int = 16, radius: Optional[int] = None, passes: int = 1,
                  method: str = "direct", window_sigma: Optional[float] = None, diameter: float = 2.5, mask=None,
                  min_valid_fraction: float = 0.5, fill_masked: bool = False, weighting=None):
        """Displacement field of an image pair (torch tensors on the device or numpy arrays, [height, width]): returns numpy
        (vectors [n_rows, n_cols, 4] = dx, dy, peak, ratio; flags [n_rows, n_cols]).  radius None = win // 2.  passes=2:
        pass 1, the normalised median test and the predictor on the host (photon_amd.piv_correlation), then pass 2 with
        the integer window offsets.  method="phase": section 13's phase correlation instead of section 5's direct sums
        (window_sigma None = win / 4; diameter: the e^-2 particle diameter; radius None or win // 2 = win // 2 - 1).
        mask: pixels to leave out (a bool / u8 array or device tensor [height, width], nonzero = excluded, or a tuple of two
        for the two frames): section 17 instead of section 5, "direct" alone.  A window that keeps fewer than
        min_valid_fraction of its pixels in either frame is masked out (flag 16, NaN vector); fill_masked=True gives those
        nodes the median of their finite 3 x 3 neighbours instead (photon_amd.piv_mask.fill_masked).  A partially masked
        window (flag 32) measures its free pixels: its vector sits at their centroid (piv_mask.window_valid).
        weighting: a weight per window pixel on frame 1's window, section 18 instead of section 5: "gaussian" (sigma = win /
        4), ("gaussian", sigma), or an array [win, win] of finite weights >= 0 (photon_amd.piv_weighting); "direct" without a
        mask alone.  A Gaussian window keeps the response to displacement wavelengths below the window size positive."""
        passes = _checked_passes(passes)
        im1, im2, _ = _checked_pair(im1, im2, mask)
        correlator = _Correlator((win,), method, window_sigma=window_sigma, diameter=diameter, mask=mask,
                                 min_valid_fraction=min_valid_fraction, weighting=weighting)
        dev, stream, a, b, h, w = _pair_on_device(im1, im2)
        correlate, radius, _ = correlator.on_device(self, (h, w), dev).at(win, radius)
        vectors, flags, _ = _two_passes(lambda off: correlate(a.data_ptr(), b.data_ptr(), w, h, win, step, radius, off, stream=stream),
                                        passes, dev)
        if mask is not None and fill_masked:
            from . import piv_mask
            vectors = piv_mask.fill_masked(vectors, flags, True).astype(np.float32)
        return vectors, flags

    # ---- ensemble correlation: one field from many image pairs (section 14) ---------------------------------------------
    def piv_correlate_ensemble(self, d_im1_ptr: int, d_im2_ptr: int, pair_stride: int, n_pairs: int, width: int, height: int, win: int,
                               step: int, radius: int, d_offset_ptr: int = 0, planes: bool = False, stream: int = 0):
        """photon_piv_correlate_ensemble on raw device pointers: pair k is (d_im1_ptr, d_im2_ptr) + k pair_stride floats, each
        f32 [height, width]; the planes and energies of the pairs are summed per window before the peak is read.  Returns
        torch device tensors (vectors [n_rows, n_cols, 4], flags [n_rows, n_cols] int32, count [n_rows, n_cols] int32 -- the
        contributing pairs per window --, planes [n_rows, n_cols, 2R+1, 2R+1] or None) as piv_correlate does, filled
        asynchronously on `stream`.  The definition: include/parallel_ray_tracing.h, section 14 (photon_amd.piv_ensemble:
        host model)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), int(pair_stride), int(n_pairs), int(width), int(height), int(win), int(step), int(radius))
        outputs = (_VECTORS, _FLAGS, ((), "int32", True), _planes(radius, planes))
        return self._grid_call("photon_piv_correlate_ensemble", head, outputs, stream, (d_offset_ptr,))

    def correlate_ensemble(self, frames1, frames2=None, win: int = 32, step: int = 16, radius: Optional[int] = None, passes: int = 1):
        """One displacement field from a stack of image pairs (torch tensors on the device or numpy arrays): frames1 and
        frames2 [N, height, width] hold pair k as (frames1[k], frames2[k]); frames2 None: frames1 is a time series of N + 1
        frames, pair k = (frames1[k], frames1[k + 1]).  Returns numpy (vectors [n_rows, n_cols, 4] = dx, dy, peak, ratio;
        flags [n_rows, n_cols]; count [n_rows, n_cols], the pairs that contributed to each window).  radius None = win // 2.
        passes=2: the ensemble pass, the normalised median test and the predictor on the host as ``correlate`` runs them,
        then a second ensemble pass with the integer window offsets."""
        import torch
        from . import piv_correlation as pc
        passes = _checked_passes(passes)
        radius = int(win) // 2 if radius is None else int(radius)
        frames1, frames2 = _checked(frames1, "frames1", 3), _checked(frames2, "frames2", 3)      # [N, height, width]
        if frames1 is None:
            raise TypeError("frames1 must be a stack of frames, not None")
        if frames2 is not None and tuple(frames2.shape) != tuple(frames1.shape):
            raise ValueError("frames1 and frames2 must be two stacks of one shape")
        dev, stream = _device_and_stream()
        a = _on_device(frames1, torch.float32, dev, "frames1", 3)
        if frames2 is None:
            if a.shape[0] < 2:
                raise ValueError("a time series needs at least two frames")
            n, b_ptr = a.shape[0] - 1, a[1].data_ptr()
        else:
            b = _on_device(frames2, torch.float32, dev, "frames2", 3)
            n, b_ptr = a.shape[0], b.data_ptr()
        h, w = int(a.shape[1]), int(a.shape[2])
        pc.check_arguments((h, w), win, step, radius)
        if n < 1:
            raise ValueError("an ensemble needs at least one pair")
        vectors, flags, (_, _, cnt, _) = _two_passes(
            lambda off: self.piv_correlate_ensemble(a.data_ptr(), b_ptr, h * w, n, w, h, win, step, radius, off, stream=stream), passes, dev)
        return vectors, flags, cnt.cpu().numpy()

    # ---- image pre-processing: background removal, min-max filter (section 15) -----------------------------------------
    def piv_background(self, d_frames_ptr: int, frame_stride: int, n_frames: int, width: int, height: int, mode: int = 0, stream: int = 0):
        """photon_piv_background on a raw device pointer: frame k is d_frames_ptr + k frame_stride floats, f32 [height, width].
        Returns the per-pixel minimum (mode 0) or mean (mode 1) of the frames as a torch device tensor [height, width], filled
        asynchronously on `stream`.  The definition: include/parallel_ray_tracing.h, section 15 (photon_amd.piv_preprocess:
        host models)."""
        import torch
        dev, _ = _device_and_stream()
        out = torch.empty((max(int(height), 0), max(int(width), 0)), dtype=torch.float32, device=dev)
        self._call("photon_piv_background", _vp(d_frames_ptr), int(frame_stride), int(n_frames), int(width), int(height), int(mode),
                   _vp(out.data_ptr()), _vp(stream))
        return out

    def piv_background_path(self, d_frames_ptr: int, frame_stride: int, d_out_ptr: int) -> int:
        """1 when photon_piv_background reads these buffers 16 bytes per lane, 0 when pixel by pixel (the same bits)."""
        return int(self.lib.photon_piv_background_path(_vp(d_frames_ptr), int(frame_stride), _vp(d_out_ptr)))

    def piv_preprocess(self, d_frames_ptr: int, frame_stride: int, n_frames: int, width: int, height: int, d_background_ptr: int = 0,
                       radius: int = 0, floor: float = 0.0, stream: int = 0):
        """photon_piv_preprocess on raw device pointers: per frame max(frame - background, 0) (d_background_ptr 0: the frame
        as it is), then the min-max filter of `radius` (0: none) with the absolute contrast floor `floor`.  Returns a new
        torch device stack [n_frames, height, width], filled asynchronously on `stream`."""
        import torch
        dev, _ = _device_and_stream()
        out = torch.empty((max(int(n_frames), 0), max(int(height), 0), max(int(width), 0)), dtype=torch.float32, device=dev)
        self._call("photon_piv_preprocess", _vp(d_frames_ptr), int(frame_stride), int(n_frames), int(width), int(height),
                   _vp(d_background_ptr), int(radius), float(floor), _vp(out.data_ptr()), int(width) * int(height), _vp(stream))
        return out

    def preprocess_series(self, frames1, frames2=None, background="min", minmax_radius: int = 0, floor: Optional[float] = None):
        """Background removal and min-max filter of a stack or a time series (torch tensors on the device or numpy arrays,
        [N, height, width]) on the current stream, no host wait inside.  background: "min" or "mean" of the stack itself, an
        array or tensor [height, width], or None (no subtraction).  With frames2 each stack gets its own background (the two
        exposures of a camera differ); a series in one buffer has one background over all its frames.  minmax_radius 0: no
        filter; above 0 `floor` is required -- an absolute intensity just above the noise that remains after the
        subtraction, which cannot be guessed from one image.  Returns the processed device stack, or the two stacks, that
        ``correlate_ensemble`` takes as they are (``correlate`` and ``correlate_deform``: one frame of each)."""
        import torch
        from . import piv_preprocess as pp
        modes = {"min": pp.MODE_MIN, "mean": pp.MODE_MEAN}
        if isinstance(background, str) and background not in modes:
            raise ValueError(f'background must be "min", "mean", None or a [height, width] plane, not "{background}"')
        frames1, frames2 = _checked(frames1, "frames1", 3), _checked(frames2, "frames2", 3)      # [N, height, width]
        if frames1 is None:
            raise TypeError("frames1 must be a stack of frames, not None")
        if background is not None and not isinstance(background, str):
            background = _checked(background, "background", 2)
            for frames in (frames1, frames2):
                if frames is not None and tuple(background.shape) != tuple(frames.shape[1:]):
                    raise ValueError("the background must be one [height, width] plane")
        dev, stream = _device_and_stream()

        def one(frames, name):
            t = _on_device(frames, torch.float32, dev, name, 3)
            n, h, w = (int(v) for v in t.shape)
            pp.check_arguments((h, w), n, radius=minmax_radius, floor=floor, background=background is not None)
            if background is None:
                bg = None
            elif isinstance(background, str):
                bg = self.piv_background(t.data_ptr(), h * w, n, w, h, modes[background], stream=stream)
            else:
                bg = _on_device(background, torch.float32, dev, "background", 2)
            return self.piv_preprocess(t.data_ptr(), h * w, n, w, h, bg.data_ptr() if bg is not None else 0, minmax_radius,
                                       0.0 if floor is None else float(floor), stream=stream)
        return one(frames1, "frames1") if frames2 is None else (one(frames1, "frames1"), one(frames2, "frames2"))

    # ---- iterative image-deformation correlation on the device (section 7) ---------------------------------------------
    def bspline_coefficients(self, d_im_ptr: int, width: int, height: int, d_coef_ptr: int, stream: int = 0):
        """photon_piv_bspline_coefficients on raw device pointers (f32 [height, width] in and out), asynchronous on `stream`."""
        self._call("photon_piv_bspline_coefficients", _vp(d_im_ptr), int(width), int(height), _vp(d_coef_ptr), _vp(stream))

    def piv_deform(self, d_coef_ptr: int, width: int, height: int, d_field_ptr: int, field_stride: int, n_rows: int, n_cols: int,
                   win: int, step: int, scale: float, d_out_ptr: int, stream: int = 0):
        """photon_piv_deform on raw device pointers: the image of the coefficients warped by scale x the grid's field
        (f32, `field_stride` 2 or 4 floats per vector), asynchronous on `stream`."""
        self._call("photon_piv_deform", _vp(d_coef_ptr), int(width), int(height), _vp(d_field_ptr), int(field_stride), int(n_rows), int(n_cols),
                   int(win), int(step), float(scale), _vp(d_out_ptr), _vp(stream))

    def piv_validate(self, d_pred_ptr: int, d_vectors_ptr: int, d_flags_ptr: int, n_rows: int, n_cols: int, d_field_ptr: int,
                     d_smooth_ptr: int, d_status_ptr: int, eps: float = 0.1, threshold: float = 2.0, stream: int = 0):
        """photon_piv_validate on raw device pointers (d_pred_ptr, d_smooth_ptr: 0 = NULL), asynchronous on `stream`."""
        self._call("photon_piv_validate", _vp(d_pred_ptr), _vp(d_vectors_ptr), _vp(d_flags_ptr), int(n_rows), int(n_cols), float(eps),
                   float(threshold), _vp(d_field_ptr), _vp(d_smooth_ptr), _vp(d_status_ptr), _vp(stream))

    def piv_regrid(self, d_src_ptr: int, src_stride: int, src_rows: int, src_cols: int, src_win: int, src_step: int, width: int,
                   height: int, dst_win: int, dst_step: int, stream: int = 0):
        """photon_piv_regrid on raw device pointers: the field f32 [src_rows, src_cols, src_stride] of the grid (src_win,
        src_step) at the window centres of the grid (dst_win, dst_step) of the same width x height image.  Returns a torch
        device tensor [dst_rows, dst_cols, 2], filled asynchronously on `stream`.  The definition:
        include/parallel_ray_tracing.h, section 16 (photon_amd.piv_multigrid: host models)."""
        head = (_vp(d_src_ptr), int(src_stride), int(src_rows), int(src_cols), int(src_win), int(src_step), int(width), int(height), int(dst_win),
                int(dst_step))
        return self._grid_call("photon_piv_regrid", head, (((2,), "float32", True),), stream)[0]

    def _correlate_validated(self, correlate, a, b, grid, radius: int, settings: _DeformSettings, stream: int):
        """Pass 0 of the deformation chain, all of correlation_predictor: correlate the device images a, b on the grid (win,
        step) with `correlate` (what _Correlator.at returned) and `radius`, then validate with no predictor (settings: eps and
        threshold).  Returns (vec, field, smoothed, status), field and smoothed [n_rows, n_cols, 2]."""
        import torch
        h, w = a.shape
        vec, flg, _ = correlate(a.data_ptr(), b.data_ptr(), w, h, *grid, radius, stream=stream)
        r, c = flg.shape
        field, smoothed = (torch.empty((r, c, 2), dtype=torch.float32, device=a.device) for _ in range(2))
        status = torch.empty((r, c), dtype=torch.int32, device=a.device)
        self.piv_validate(0, vec.data_ptr(), flg.data_ptr(), r, c, field.data_ptr(), smoothed.data_ptr(), status.data_ptr(),
                          eps=settings.eps, threshold=settings.threshold, stream=stream)
        return vec, field, smoothed, status

    def _coefficients_of(self, stack, stream: int):
        """The B-spline coefficients (section 7a) of every frame of the device stack f32 [n, h, w], queued on `stream`."""
        import torch
        n, h, w = (int(v) for v in stack.shape)
        coef = torch.empty((n, h, w), dtype=torch.float32, device=stack.device)
        for k in range(n):
            self.bspline_coefficients(stack[k].data_ptr(), w, h, coef[k].data_ptr(), stream)
        return coef

    def _frame_coefficients(self, a, b, stream: int):
        """(coef, warped), two device tensors [2, h, w]: the B-spline coefficients of the frames a and b, queued on `stream`, and
        the scratch their warps go to."""
        import torch
        h, w = a.shape
        coef, warped = (torch.empty((2, h, w), dtype=torch.float32, device=a.device) for _ in range(2))
        self.bspline_coefficients(a.data_ptr(), w, h, coef[0].data_ptr(), stream)
        self.bspline_coefficients(b.data_ptr(), w, h, coef[1].data_ptr(), stream)
        return coef, warped

    def _deform_chain(self, a, b, schedule, iterations, correlator: _Correlator, settings: _DeformSettings = _DeformSettings()):
        """What correlate_deform (a one-level schedule), correlate_multigrid and optical_flow's default predictor queue on the
        device images a, b, nothing copied back.  schedule, iterations: what piv_multigrid.check_schedule returned;
        correlator: after its device step.  Pass 0 (settings.radius) and iterations[0] deformation iterations at schedule[0];
        per further level the last predictor regridded and iterations[l] deformation iterations there.  An iteration warps
        both frames half-way by the predictor, correlates with settings.residual_radius and validates with the predictor;
        the next predictor is the smoothed field, or with smooth=False the field itself.  The coefficients of both frames
        are computed once, before the first warp.  Returns (field [n_rows, n_cols, 2], vec [n_rows, n_cols, 4] of the last
        correlation, status [n_rows, n_cols]) of the last level as device tensors queued on the current stream.  Under a mask
        every correlation is section 17's in unwarped image coordinates, each level with min_valid from its own win, and
        each frame's masked pixels are at that frame's unmasked mean before the coefficients (no host wait); with weighting
        every correlation of a level is section 18's with the table of its win."""
        import torch
        dev, stream = _device_and_stream()
        h, w = a.shape
        coef = warped = None
        if correlator.mask is not None:
            a, b = _replace_masked(a, correlator.mask[0]), _replace_masked(b, correlator.mask[1])
        for level, ((win, step), n) in enumerate(zip(schedule, iterations)):
            correlate, first_radius, _ = correlator.at(win, settings.radius if level == 0 else None)
            if level == 0:
                vec, field, smoothed, status = self._correlate_validated(correlate, a, b, (win, step), first_radius, settings, stream)
            else:
                r, c = field.shape[:2]
                field = smoothed = self.piv_regrid((smoothed if settings.smooth else field).data_ptr(), 2, r, c, *schedule[level - 1], w, h,
                                                   win, step, stream)
            if n == 0:
                continue
            if coef is None:
                coef, warped = self._frame_coefficients(a, b, stream)
            pred = smoothed if settings.smooth else field
            r, c = pred.shape[:2]
            fields, smooths = (torch.empty((2, r, c, 2), dtype=torch.float32, device=dev) for _ in range(2))   # ping-pong: a predictor is no output
            status = torch.empty((r, c), dtype=torch.int32, device=dev)
            for k in range(n):
                field, smoothed = fields[k & 1], smooths[k & 1]
                self.piv_deform(coef[0].data_ptr(), w, h, pred.data_ptr(), 2, r, c, win, step, -0.5, warped[0].data_ptr(), stream)
                self.piv_deform(coef[1].data_ptr(), w, h, pred.data_ptr(), 2, r, c, win, step, 0.5, warped[1].data_ptr(), stream)
                vec, flg, _ = correlate(warped[0].data_ptr(), warped[1].data_ptr(), w, h, win, step, settings.residual_radius, stream=stream)
                self.piv_validate(pred.data_ptr(), vec.data_ptr(), flg.data_ptr(), r, c, field.data_ptr(), smoothed.data_ptr(),
                                  status.data_ptr(), eps=settings.eps, threshold=settings.threshold, stream=stream)
                pred = smoothed if settings.smooth else field
        return field, vec, status

    def correlate_deform(self, im1, im2, win: int = 32, step: int = 16, radius: Optional[int] = None, iterations: int = 3,
                         residual_radius: int = 4, smooth: bool = True, eps: float = 0.1, threshold: float = 2.0, method: str = "direct",
                         window_sigma: Optional[float] = None, diameter: float = 2.5, mask=None, min_valid_fraction: float = 0.5,
                         fill_masked: bool = False, weighting=None):
        """Displacement field of an image pair by iterative image deformation (section 7; model:
        photon_amd.piv_deformation.correlate_deform_model).  Pass 0 correlates the images with `radius` (None = win // 2);
        every iteration warps both frames half-way by the validated, smoothed field, correlates the warped pair with
        `residual_radius` and adds the residual.  Returns what ``correlate`` returns: numpy (vectors [n_rows, n_cols, 4] =
        dx, dy of the last unsmoothed field, peak and ratio of the last correlation; status [n_rows, n_cols], section 5's
        flags with bit 8 on replaced vectors).  Everything runs on the current stream; the host waits once, for the result.
        method, window_sigma, diameter: the correlator of every pass, as ``correlate`` takes them.
        mask, min_valid_fraction: as ``correlate`` takes them, for every pass.  The mask stays in unwarped image coordinates
        on every iteration (it does not follow the warp), and each frame's masked pixels are set to that frame's unmasked
        mean before the B-spline coefficients, so that a bright body does not ring into the warped free pixels.  Inside the
        loop a masked-out node (status 16 | 8) holds its neighbours' median, a smooth predictor across the hole;
        fill_masked=False returns NaN (dx, dy, peak, ratio) there, True the medians, for callers that pass the field on to
        ``displacement_uncertainty`` or ``optical_flow(predictor=...)``.
        weighting: as ``correlate`` takes it, for every pass: with a top-hat window the loop amplifies the wrong-signed
        response to wavelengths below the window size, with a Gaussian window it converges towards the true amplitude."""
        return self.correlate_multigrid(im1, im2, ((win, step),), (iterations,), radius=radius, residual_radius=residual_radius, smooth=smooth,
                                        eps=eps, threshold=threshold, method=method, window_sigma=window_sigma, diameter=diameter, mask=mask,
                                        min_valid_fraction=min_valid_fraction, fill_masked=fill_masked, weighting=weighting)

    def correlate_multigrid(self, im1, im2, schedule=((64, 32), (32, 16), (16, 8)), iterations=(1, 1, 2), radius: Optional[int] = None,
                            residual_radius: int = 4, smooth: bool = True, eps: float = 0.1, threshold: float = 2.0, method: str = "direct",
                            window_sigma: Optional[float] = None, diameter: float = 2.5, mask=None, min_valid_fraction: float = 0.5,
                            fill_masked: bool = False, weighting=None):
        """Displacement field of an image pair by multigrid window refinement (section 16; model:
        photon_amd.piv_multigrid.correlate_multigrid_model): large windows find the shift, small ones resolve its gradients,
        in one call.  schedule: the (win, step) of every level, any valid pairs; iterations: the deformation iterations per
        level (>= 0 on level 0, >= 1 after).  Level 0 is ``correlate_deform`` at schedule[0] with `radius`; every further
        level takes the previous level's smoothed field (smooth=False: the field itself), regridded to its window centres,
        as the predictor and iterates on its own grid with `residual_radius`.  A one-level schedule is ``correlate_deform``
        bit for bit.  Returns what ``correlate_deform`` returns, on the last level's grid: hand it to
        ``displacement_uncertainty`` or ``optical_flow(predictor=...)`` with the last (win, step).  method, window_sigma
        (None = win / 4 of each level), diameter: the correlator of every pass.  Everything runs on the current stream; the
        host waits once, for the result.  mask, min_valid_fraction, fill_masked: as ``correlate_deform`` takes them; every
        level takes its min_valid from its own win.  weighting: as ``correlate`` takes it; "gaussian" and ("gaussian", sigma)
        make one table per level's win (sigma None = win / 4 of each level), an array is accepted only when every level has
        its win."""
        import torch
        from . import piv_multigrid as pm
        im1, im2, _ = _checked_pair(im1, im2, mask)
        schedule, iterations = pm.check_schedule(tuple(im1.shape), schedule, iterations, radius, residual_radius, method, window_sigma, diameter)
        correlator = _Correlator([win for win, _ in schedule], method, window_sigma=window_sigma, diameter=diameter, mask=mask,
                                 min_valid_fraction=min_valid_fraction, weighting=weighting)
        dev, _, a, b, h, w = _pair_on_device(im1, im2)
        field, vec, status = self._deform_chain(a, b, schedule, iterations, correlator.on_device(self, (h, w), dev),
                                                _DeformSettings(radius, residual_radius, smooth, eps, threshold))
        out = torch.cat([field, vec[..., 2:4]], dim=-1)      # dx, dy of the field, peak and ratio of the last correlation
        if mask is not None and not fill_masked:
            out = _nan_where_masked_out(out, status)         # piv_mask.fill_masked's other half
        return out.cpu().numpy(), status.cpu().numpy()

    # ---- displacement uncertainty from correlation statistics (section 11) -------------------------------------------------
    def piv_uncertainty(self, d_im1_ptr: int, d_im2_ptr: int, width: int, height: int, win: int, step: int, reach: int = 2,
                        stats: bool = False, stream: int = 0):
        """photon_piv_uncertainty on a matched pair of device f32 images (raw pointers, row-major height x width).  Returns
        torch device tensors (sigma [n_rows, n_cols, 2] f32 = sigma_x, sigma_y in pixels; flags [n_rows, n_cols] int32; stats
        [n_rows, n_cols, 2, 4] f64 = (C0, C1, S(0), V) per axis, or None), filled asynchronously on `stream`.  The
        definition: include/parallel_ray_tracing.h, section 11 (photon_amd.piv_uncertainty: host model)."""
        head = (_vp(d_im1_ptr), _vp(d_im2_ptr), int(width), int(height), int(win), int(step), int(reach))
        return self._grid_call("photon_piv_uncertainty", head, (((2,), "float32", True), _FLAGS, ((2, 4), "float64", stats)), stream)

    def displacement_uncertainty(self, im1, im2, field, win: int = 32, step: int = 16, reach: int = 2, return_warped: bool = False):
        """Uncertainty (sigma_x, sigma_y) in pixels of every vector of a displacement field on section 5's grid, whatever
        measured it (``correlate``, ``correlate_deform``, window means of tracked dots): the B-spline coefficients of both
        frames, frame 1 warped by -field / 2 and frame 2 by +field / 2 (photon_piv_deform), photon_piv_uncertainty on the
        warped pair (model: photon_amd.piv_uncertainty.displacement_uncertainty_model).  im1, im2: torch device tensors or
        numpy [height, width]; field [n_rows, n_cols, >= 2] (dx, dy first), numpy or a device tensor; a vector that is not
        finite reads as (0, 0).  Returns numpy (sigma [n_rows, n_cols, 2] f32, flags [n_rows, n_cols] int32: bits 2, 16, 32
        of section 11); with return_warped also the two warped images as torch device tensors.  Everything runs on the
        current stream; the host waits once, for the result."""
        import torch
        from . import piv_correlation as pc
        from . import piv_uncertainty as pu
        field = _checked(field, "field", 3)
        dev, stream, a, b, h, w = _image_pair(im1, im2)
        pu.check_arguments((h, w), win, step, reach)
        fld = _on_device(field, torch.float32, dev, "field", 3)
        r, c = pc.grid_shape((h, w), win, step)
        if fld.dim() != 3 or fld.shape[2] < 2 or tuple(fld.shape[:2]) != (r, c):
            raise ValueError(f"field must be [{r}, {c}, >= 2]: the grid of a {h} x {w} image, win {win}, step {step}")
        fld = (fld if fld.shape[2] in (2, 4) else fld[..., :2]).contiguous()
        sigma, flags, warped = self._uncertainty_chain(a, b, fld, win, step, reach, stream)
        out = (sigma.cpu().numpy(), flags.cpu().numpy())
        return (*out, warped[0], warped[1]) if return_warped else out

    def _uncertainty_chain(self, a, b, fld, win: int, step: int, reach: int, stream: int):
        """What displacement_uncertainty queues on the device images a, b and the contiguous field fld [n_rows, n_cols, 2 or 4]:
        the coefficients, the two half-way warps, photon_piv_uncertainty.  Returns (sigma, flags, warped [2, h, w]), device
        tensors; nothing is copied back."""
        import torch
        h, w = a.shape
        r, c = fld.shape[:2]
        coef, warped = torch.empty((2, h, w), dtype=torch.float32, device=a.device), torch.empty((2, h, w), dtype=torch.float32, device=a.device)
        for k, (im, scale) in enumerate(((a, -0.5), (b, 0.5))):
            self.bspline_coefficients(im.data_ptr(), w, h, coef[k].data_ptr(), stream)
            self.piv_deform(coef[k].data_ptr(), w, h, fld.data_ptr(), int(fld.shape[2]), r, c, win, step, scale, warped[k].data_ptr(), stream)
        sigma, flags, _ = self.piv_uncertainty(warped[0].data_ptr(), warped[1].data_ptr(), w, h, win, step, reach, stream=stream)
        return sigma, flags, warped

    # ---- stereo PIV: dewarp two cameras, recover three components (section 19) ----------------------------------------------
    def piv_dewarp(self, d_coef_ptr: int, frame_stride: int, n_frames: int, width: int, height: int, poly, grid, out_width: int,
                   out_height: int, out_stride: int, d_out_ptr: int, d_mask_ptr: int = 0, stream: int = 0):
        """photon_piv_dewarp on raw device pointers: n_frames coefficient images f32 [height, width], frame_stride floats apart,
        resampled through the folded camera (poly [2, 10] and grid [4], host values from piv_stereo.plane_coefficients) into
        n_frames images f32 [out_height, out_width], out_stride floats apart, and the u8 mask [out_height, out_width] (0 = NULL)
        of the pixels outside the source; asynchronous on `stream`."""
        job = photon_piv_dewarp_t(d_coef=int(d_coef_ptr) or None, frame_stride=int(frame_stride), n_frames=int(n_frames), width=int(width),
                                  height=int(height), out_width=int(out_width), out_height=int(out_height), out_stride=int(out_stride),
                                  d_out=int(d_out_ptr) or None, d_mask=int(d_mask_ptr) or None, stream=int(stream) or None)
        folded, pitches = np.ascontiguousarray(poly, np.float64), np.ascontiguousarray(grid, np.float64)
        if folded.shape != (2, 10) or pitches.shape != (4,):
            raise ValueError("poly must be [2, 10] and grid [4] (piv_stereo.plane_coefficients)")
        ctypes.memmove(job.poly, folded.ctypes.data, folded.nbytes)
        ctypes.memmove(job.grid, pitches.ctypes.data, pitches.nbytes)
        self._call("photon_piv_dewarp", ctypes.byref(job))

    def piv_stereo_reconstruct(self, d_field1_ptr: int, d_field2_ptr: int, field_stride: int, cameras, plane, win: int, step: int,
                               d_flags1_ptr: int = 0, d_flags2_ptr: int = 0, d_sigma1_ptr: int = 0, d_sigma2_ptr: int = 0, stream: int = 0):
        """photon_piv_stereo_reconstruct on raw device pointers: the two cameras' fields f32 [n_rows, n_cols, field_stride] on
        section 5's grid (win, step) of the plane, their flags and their sigmas f32 [n_rows, n_cols, 2] (0 = NULL), the two
        cameras and the plane (piv_stereo's dicts).  Returns torch device tensors (out f64 [n_rows, n_cols, 8] = dX, dY, dZ,
        residual, sigma_X, sigma_Y, sigma_Z, pivot ratio; flags int32 [n_rows, n_cols]), filled asynchronously on `stream`."""

        def fill(job):
            job.d_field1, job.d_field2, job.field_stride = int(d_field1_ptr) or None, int(d_field2_ptr) or None, int(field_stride)
            job.d_flags1, job.d_flags2 = int(d_flags1_ptr) or None, int(d_flags2_ptr) or None
            job.d_sigma1, job.d_sigma2 = int(d_sigma1_ptr) or None, int(d_sigma2_ptr) or None
        return self._stereo_node_call("photon_piv_stereo_reconstruct", _stereo_job(cameras, plane, win, step), 8, fill, stream)

    def piv_stereo_triangulate(self, d_disparity_ptr: int, field_stride: int, cameras, plane, win: int, step: int, iterations: int = 4,
                               d_flags_in_ptr: int = 0, stream: int = 0):
        """photon_piv_stereo_triangulate on raw device pointers: the disparity field f32 [n_rows, n_cols, field_stride] between
        the two cameras' dewarped frames on section 5's grid (win, step) of the plane and its flags (0 = NULL), the two
        cameras and the plane (piv_stereo's dicts).  Returns torch device tensors (out f64 [n_rows, n_cols, 6] = X, Y, Z, the
        triangulation error, the last step's length, the smallest pivot ratio; flags int32 [n_rows, n_cols]), filled
        asynchronously on `stream`."""
        job = _stereo_job(cameras, plane, win, step, photon_piv_triangulate_t)
        job.iterations = int(iterations)

        def fill(job):
            job.d_disparity, job.field_stride, job.d_flags_in = int(d_disparity_ptr) or None, int(field_stride), int(d_flags_in_ptr) or None
        return self._stereo_node_call("photon_piv_stereo_triangulate", job, 6, fill, stream)

    def _stereo_node_call(self, entry: str, job, width: int, fill, stream: int):
        """The two calls of a stereo node entry point: the size query on `job` (plane, cameras, win, step in it), then out f64
        [n_rows, n_cols, width] and flags int32 [n_rows, n_cols], fill(job) for the entry's own members, and the launch."""
        import torch
        rows, cols = ctypes.c_int(0), ctypes.c_int(0)
        job.rows_out, job.cols_out = ctypes.pointer(rows), ctypes.pointer(cols)
        self._call(entry, ctypes.byref(job))                                             # the size query
        dev = _current_device()
        out = torch.empty((rows.value, cols.value, width), dtype=torch.float64, device=dev)
        flags = torch.empty((rows.value, cols.value), dtype=torch.int32, device=dev)
        fill(job)
        job.n_rows, job.n_cols, job.d_out, job.d_flags, job.stream = rows.value, cols.value, out.data_ptr(), flags.data_ptr(), int(stream) or None
        self._call(entry, ctypes.byref(job))
        return out, flags

    def _dewarp_queued(self, stack, camera, plane, stream: int):
        """The device stack f32 [n, h, w] of one camera's frames onto the plane, queued on `stream`: the coefficients of every
        frame (section 7a), then one dewarp launch for all of them.  Returns (frames [n, plane height, plane width], mask u8
        [plane height, plane width], whether any pixel of the plane is outside the source -- decided on the host, from
        piv_stereo.folded_points, the kernel's own f64 operations, so that nothing waits for the device)."""
        import torch
        from . import piv_stereo as ps
        n, h, w = stack.shape
        oh, ow = int(plane["height"]), int(plane["width"])
        poly, grid = ps.plane_coefficients(camera, plane)
        coef = self._coefficients_of(stack, stream)
        frames = torch.empty((n, oh, ow), dtype=torch.float32, device=stack.device)
        outside = torch.empty((oh, ow), dtype=torch.uint8, device=stack.device)
        self.piv_dewarp(coef.data_ptr(), h * w, n, w, h, poly, grid, ow, oh, oh * ow, frames.data_ptr(), outside.data_ptr(), stream)
        return frames, outside, bool(ps.outside_mask(poly, grid, (oh, ow), (h, w)).any())

    def dewarp(self, frames_in, camera, plane):
        """One camera's frames resampled onto the plane's grid (section 19a): frames_in is one frame [height, width] or a
        stack [n, height, width], taken as the ingest rule of this class takes any image; camera and plane are
        piv_stereo's dicts (piv_stereo.fit_camera, piv_stereo.plane).  The B-spline coefficients per frame, then one dewarp
        launch, on the current stream; nothing waits.  Returns device tensors (frames f32 [n, plane height, plane width] or
        [plane height, plane width]; mask u8 [plane height, plane width], 1 where the plane lies outside the camera's
        frame), which every correlator driver takes as they are, the mask as its mask=."""
        import torch
        x = _checked(frames_in, "frames_in")
        if x.ndim not in (2, 3):
            raise ValueError(f"frames_in must be one frame [height, width] or a stack [n, height, width], not shape {tuple(x.shape)}")
        dev, stream = _device_and_stream()
        t = _on_device(x, torch.float32, dev, "frames_in")
        frames, outside, _ = self._dewarp_queued(t.reshape((-1,) + tuple(t.shape[-2:])), camera, plane, stream)
        return (frames[0] if x.ndim == 2 else frames), outside

    def correlate_stereo(self, cam1_frames, cam2_frames, cameras, plane, evaluate: str = "deform", settings: Optional[dict] = None,
                         sigma: bool = False):
        """Three displacement components per node from two cameras on one light sheet (section 19; model:
        photon_amd.piv_stereo.correlate_stereo_model).  cam1_frames, cam2_frames: the two exposures of each camera, a stack
        [2, height, width] each, taken as the ingest rule of this class takes any stack (the cameras' sensors may differ);
        cameras: the two piv_stereo cameras; plane: the piv_stereo plane whose grid both are dewarped to.  On the current
        stream, in this order: the coefficients and one dewarp launch per camera; per camera the chain that `evaluate` names
        on the dewarped pair -- "correlate" (one pass of ``correlate``), "deform" (``correlate_deform``) or "multigrid"
        (``correlate_multigrid``), the same code paths those drivers run -- with the camera's dewarp mask as the chain's mask
        when a pixel of the plane is outside that camera's frame; with sigma=True ``displacement_uncertainty``'s chain per
        camera; the reconstruction.  The host waits once, for the result.
        settings: the chain's options by their names in those drivers -- win (32), step (16), radius, method, window_sigma,
        diameter, min_valid_fraction, weighting; for "deform" and "multigrid" iterations (3, or one per level), residual_radius,
        smooth, eps, threshold; for "multigrid" schedule; reach (2) for sigma.  An unknown name is refused.
        Returns numpy (out f64 [n_rows, n_cols, 8] = dX, dY, dZ in world units, the stereo residual in image pixels,
        sigma_X, sigma_Y, sigma_Z (NaN without sigma=True), the pivot ratio; status int32 [n_rows, n_cols] = the two cameras'
        status or-ed, 64 = degenerate geometry, 128 = a camera's vector is not finite (masked out, flat); the two cameras'
        2-C fields (vectors1, vectors2) [n_rows, n_cols, 4] = dx, dy in dewarped pixels, peak, ratio)."""
        import torch
        from . import piv_multigrid as pm
        from . import piv_uncertainty as pu
        known = {"win": 32, "step": 16, "radius": None, "method": "direct", "window_sigma": None, "diameter": 2.5, "min_valid_fraction": 0.5,
                 "weighting": None, "iterations": None, "residual_radius": 4, "smooth": True, "eps": 0.1, "threshold": 2.0, "schedule": None,
                 "reach": 2}
        unknown = sorted(set(settings or {}) - set(known))
        if unknown:
            raise ValueError(f"correlate_stereo: unknown settings {unknown}; known: {sorted(known)}")
        s = {**known, **(settings or {})}
        if evaluate not in ("correlate", "deform", "multigrid"):
            raise ValueError(f'evaluate must be "correlate", "deform" or "multigrid", not {evaluate!r}')
        if len(cameras) != 2:
            raise ValueError("correlate_stereo takes two cameras")
        stacks = [_checked(x, name, 3) for x, name in ((cam1_frames, "cam1_frames"), (cam2_frames, "cam2_frames"))]
        for x, name in zip(stacks, ("cam1_frames", "cam2_frames")):
            if x is None or x.shape[0] != 2:
                raise ValueError(f"{name} must be the two exposures of a camera, [2, height, width]")
        shape = (int(plane["height"]), int(plane["width"]))
        if evaluate == "multigrid":
            schedule = ((64, 32), (32, 16), (16, 8)) if s["schedule"] is None else s["schedule"]
            iterations = (1, 1, 2) if s["iterations"] is None else s["iterations"]
        else:
            schedule = ((s["win"], s["step"]),)
            iterations = (0 if evaluate == "correlate" else 3 if s["iterations"] is None else s["iterations"],)
        schedule, iterations = pm.check_schedule(shape, schedule, iterations, s["radius"], s["residual_radius"], s["method"], s["window_sigma"],
                                                 s["diameter"])
        win, step = schedule[-1]
        if sigma:
            pu.check_arguments(shape, win, step, s["reach"])
        chain = _DeformSettings(s["radius"], s["residual_radius"], s["smooth"], s["eps"], s["threshold"])
        dev, stream = _device_and_stream()
        fields, statuses, sigmas = [], [], []
        for x, name, camera in zip(stacks, ("cam1_frames", "cam2_frames"), cameras):
            frames, outside, any_outside = self._dewarp_queued(_on_device(x, torch.float32, dev, name, 3), camera, plane, stream)
            correlator = _Correlator([w for w, _ in schedule], s["method"], window_sigma=s["window_sigma"], diameter=s["diameter"],
                                     mask=outside if any_outside else None, min_valid_fraction=s["min_valid_fraction"],
                                     weighting=s["weighting"]).on_device(self, shape, dev)
            if evaluate == "correlate":
                correlate, radius, check = correlator.at(win, s["radius"])
                check(shape, win, step, radius)
                vec, status, _ = correlate(frames[0].data_ptr(), frames[1].data_ptr(), shape[1], shape[0], win, step, radius, stream=stream)
            else:
                field, vec, status = self._deform_chain(frames[0], frames[1], schedule, iterations, correlator, chain)
                vec = torch.cat([field, vec[..., 2:4]], dim=-1)
            if any_outside:
                vec = _nan_where_masked_out(vec, status)
            fields.append(vec.contiguous())
            statuses.append(status)
            if sigma:
                sigmas.append(self._uncertainty_chain(frames[0], frames[1], fields[-1], win, step, s["reach"], stream)[0])
        out, flags = self.piv_stereo_reconstruct(fields[0].data_ptr(), fields[1].data_ptr(), 4, cameras, plane, win, step,
                                                 statuses[0].data_ptr(), statuses[1].data_ptr(), *(t.data_ptr() for t in sigmas), stream=stream)
        return out.cpu().numpy(), flags.cpu().numpy(), (fields[0].cpu().numpy(), fields[1].cpu().numpy())

    def self_calibrate_stereo(self, cam1_frames, cam2_frames, cameras, plane, win: int = 64, step: int = 32, radius: Optional[int] = None,
                              passes: int = 1, rounds: int = 3, iterations: int = 4, tolerance: float = 0.05, timings: Optional[list] = None):
        """The two cameras corrected for a light sheet that is not where the calibration target stood (section 19c; model:
        photon_amd.piv_stereo.self_calibrate_model).  cam1_frames, cam2_frames: stacks [N, height, width], frame k of both
        cameras the same instant, taken as the ingest rule of this class takes any stack; cameras, plane: piv_stereo's
        dicts.  Per round, with the current cameras, on the current stream: the coefficients and one dewarp launch per camera;
        the ensemble correlation of the two dewarped stacks (``piv_correlate_ensemble``, what ``correlate_ensemble`` runs;
        passes=2, for disparities beyond the radius, adds its host step and second pass); the triangulation; one host wait;
        then on the host piv_stereo.selfcal_round -- the nodes under a dewarp mask left out, fit_sheet, sheet_frame,
        move_camera on both cameras.  The rounds end early once the rms disparity is below `tolerance` px.
        Returns (cameras, report) as the model does; hand the cameras to ``correlate_stereo``, which is unchanged.
        timings: a list that receives per round a dict of device milliseconds (dewarp, correlate, triangulate) measured with
        events; the waits this needs are extra, so leave it None outside a tool."""
        import torch
        from . import piv_correlation as pc
        from . import piv_stereo as ps
        passes = _checked_passes(passes)
        radius = int(win) // 2 if radius is None else int(radius)
        if len(cameras) != 2:
            raise ValueError("self_calibrate_stereo takes two cameras")
        if int(rounds) < 1:
            raise ValueError("rounds must be >= 1")
        if not 1 <= int(iterations) <= ps.MAX_TRIANGULATE_ITERATIONS:
            raise ValueError(f"iterations must be within [1, {ps.MAX_TRIANGULATE_ITERATIONS}]")
        names = ("cam1_frames", "cam2_frames")
        stacks = [_checked(x, name, 3) for x, name in zip((cam1_frames, cam2_frames), names)]
        if stacks[0] is None or stacks[1] is None or stacks[0].shape[0] != stacks[1].shape[0] or stacks[0].shape[0] < 1:
            raise ValueError("cam1_frames and cam2_frames must be two stacks [N, height, width] of the same N >= 1 instants")
        oh, ow = int(plane["height"]), int(plane["width"])
        pc.check_arguments((oh, ow), win, step, radius)
        dev, stream = _device_and_stream()
        device_stacks = [_on_device(x, torch.float32, dev, name, 3) for x, name in zip(stacks, names)]
        n = int(device_stacks[0].shape[0])

        def mark():
            if timings is None:
                return None
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            return event
        cameras, frame, entries = tuple(cameras), ps.identity_frame(plane), []
        for _ in range(int(rounds)):
            t0 = mark()
            dewarped = [self._dewarp_queued(x, camera, plane, stream) for x, camera in zip(device_stacks, cameras)]
            t1 = mark()
            correlate = lambda off: self.piv_correlate_ensemble(dewarped[0][0].data_ptr(), dewarped[1][0].data_ptr(), oh * ow, n, ow, oh, win,      # noqa: E731
                                                                step, radius, off, stream=stream)
            found = correlate(0) if passes == 1 else _two_passes(correlate, passes, dev)[2]
            t2 = mark()
            points, flags = self.piv_stereo_triangulate(found[0].data_ptr(), 4, cameras, plane, win, step, iterations, found[1].data_ptr(), stream)
            t3 = mark()
            points, flags, vectors = points.cpu().numpy(), flags.cpu().numpy(), found[0].cpu().numpy()      # the host waits here
            outside = [ps.outside_mask(*ps.plane_coefficients(camera, plane), (oh, ow), tuple(x.shape[1:]))
                       for x, camera in zip(device_stacks, cameras)]
            cameras, moved, entry = ps.selfcal_round(points, flags, vectors, outside, cameras, plane, win, step)
            frame = ps.compose_frames(frame, moved)
            entries.append(entry)
            if timings is not None:
                timings.append(dict(dewarp=t0.elapsed_time(t1), correlate=t1.elapsed_time(t2), triangulate=t2.elapsed_time(t3)))
            if entry["disparity_rms"] < tolerance:
                break
        return cameras, ps.selfcal_report(entries, frame)

    # ---- tomographic PIV: line-of-sight volumes, 3-D correlation (section 20) -------------------------------------------------
    def piv_volume_los(self, d_coef_ptrs, frame_strides, n_frames: int, sensor_shapes, grids, d_poly_ptr: int, vol, out_stride: int,
                       d_out_ptr: int, d_mask_ptr: int = 0, mode: int = 0, stream: int = 0):
        """photon_piv_volume_los on raw device pointers: per camera the pointer of its n_frames coefficient images, their
        stride in floats, the sensor's (height, width) and its grid [4]; d_poly_ptr the device table f64 [N, nz, 2, 10] and
        grids the host table [N, 4] of piv_tomo.los_coefficients; vol a piv_tomo volume.  Writes n_frames volumes f32 [nz, ny,
        nx], out_stride floats apart, and the u8 mask [nz, ny, nx] (0 = NULL); mode 0 the minimum, 1 the product;
        asynchronous on `stream`."""
        job = photon_piv_volume_los_t(n_frames=int(n_frames), mode=int(mode), out_stride=int(out_stride), d_out=int(d_out_ptr) or None,
                                      d_mask=int(d_mask_ptr) or None, stream=int(stream) or None)
        n = len(d_coef_ptrs)
        if not (len(frame_strides) == len(sensor_shapes) == n and 0 < n <= 8):
            raise ValueError("piv_volume_los takes 2 to 8 cameras: one pointer, stride and sensor shape each")
        if np.asarray(grids, np.float64).shape != (n, 4):
            raise ValueError(f"grids must be [{n}, 4] (piv_tomo.los_coefficients)")
        self._volume_cameras(job, sensor_shapes, grids, vol, d_poly_ptr)
        for c in range(n):
            job.d_coef[c], job.frame_stride[c] = int(d_coef_ptrs[c]) or None, int(frame_strides[c])
        self._call("photon_piv_volume_los", ctypes.byref(job))

    def piv_correlate_volume(self, d_vol1_ptr: int, d_vol2_ptr: int, nx: int, ny: int, nz: int, win: int, step: int, radius: int, win_z: int,
                             step_z: int, radius_z: int, d_offset_ptr: int = 0, stream: int = 0):
        """photon_piv_correlate_volume on raw device pointers: two volumes f32 [nz, ny, nx], the int32 offsets [n, 3] (0 =
        NULL).  The size query first, then the launch.  Returns torch device tensors (vectors f32 [n_slabs, n_rows, n_cols, 5] =
        dx, dy, dz, peak, ratio; flags int32 [n_slabs, n_rows, n_cols]; planes f32 [n_slabs, n_rows, n_cols, 2Rz+1, 2R+1,
        2R+1], the call's workspace and on return the normalised planes), filled asynchronously on `stream`."""
        import torch
        slabs, rows, cols = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        job = photon_piv_correlate_volume_t(d_vol1=int(d_vol1_ptr) or None, d_vol2=int(d_vol2_ptr) or None, nx=int(nx), ny=int(ny), nz=int(nz),
                                            win=int(win), step=int(step), radius=int(radius), win_z=int(win_z), step_z=int(step_z),
                                            radius_z=int(radius_z), n_slabs=ctypes.pointer(slabs), n_rows=ctypes.pointer(rows),
                                            n_cols=ctypes.pointer(cols))
        self._call("photon_piv_correlate_volume", ctypes.byref(job))                     # the size query
        dev, grid = _current_device(), (slabs.value, rows.value, cols.value)
        nS, nSz = 2 * int(radius) + 1, 2 * int(radius_z) + 1
        vectors = torch.empty(grid + (5,), dtype=torch.float32, device=dev)
        flags = torch.empty(grid, dtype=torch.int32, device=dev)
        planes = torch.empty(grid + (nSz, nS, nS), dtype=torch.float32, device=dev)
        job.d_offset, job.d_vectors, job.d_flags, job.d_planes = int(d_offset_ptr) or None, vectors.data_ptr(), flags.data_ptr(), planes.data_ptr()
        job.stream = int(stream) or None
        self._call("photon_piv_correlate_volume", ctypes.byref(job))
        return vectors, flags, planes

    @staticmethod
    def _volume_cameras(job, sensor_shapes, grids, vol, d_poly_ptr: int):
        """The members sections 20a, 21a and 21b share: the sensors, the grids [N, 4], the table's pointer and the volume."""
        n = len(sensor_shapes)
        table = np.ascontiguousarray(grids, np.float64)
        if not 0 < n <= 8 or table.shape != (n, 4):
            raise ValueError(f"section 21 takes 2 to 8 cameras: one sensor shape each and grids [{n}, 4] (piv_tomo.los_coefficients)")
        job.n_cameras, job.d_poly = n, int(d_poly_ptr) or None
        job.volume = photon_piv_volume_t(float(vol["x0"]), float(vol["y0"]), float(vol["z0"]), float(vol["pitch"]), int(vol["nx"]), int(vol["ny"]),
                                         int(vol["nz"]))
        for c in range(n):
            job.height[c], job.width[c] = int(sensor_shapes[c][0]), int(sensor_shapes[c][1])
        ctypes.memmove(job.grid, table.ctypes.data, table.nbytes)
        return n

    def piv_volume_project(self, d_vol_ptr: int, vol_stride: int, n_frames: int, sensor_shapes, grids, d_poly_ptr: int, vol, d_acc_ptrs,
                           acc_strides, scale_log2: int, d_image_ptrs=None, stream: int = 0):
        """photon_piv_volume_project on raw device pointers: n_frames volumes f32 [nz, ny, nx], vol_stride floats apart; per
        camera the sensor's (height, width), its grid [4], the pointer of its int64 accumulators [n_frames, height width] and
        their stride; d_image_ptrs: per camera the pointer of the f32 images (the accumulators' stride), 0 = none.  Zeroes the
        accumulators and adds every voxel above 0 in fixed point with 2^scale_log2; asynchronous on `stream`."""
        job = photon_piv_volume_project_t(n_frames=int(n_frames), scale_log2=int(scale_log2), d_vol=int(d_vol_ptr) or None, vol_stride=int(vol_stride),
                                          stream=int(stream) or None)
        n = self._volume_cameras(job, sensor_shapes, grids, vol, d_poly_ptr)
        images = [0] * n if d_image_ptrs is None else list(d_image_ptrs)
        if not len(d_acc_ptrs) == len(acc_strides) == len(images) == n:
            raise ValueError("piv_volume_project takes one accumulator pointer, stride and image pointer per camera")
        for c in range(n):
            job.d_acc[c], job.acc_stride[c], job.d_image[c] = int(d_acc_ptrs[c]) or None, int(acc_strides[c]), int(images[c]) or None
        self._call("photon_piv_volume_project", ctypes.byref(job))

    def piv_volume_mart(self, d_frame_ptrs, frame_strides, n_frames: int, sensor_shapes, grids, d_poly_ptr: int, vol, vol_stride: int,
                        d_vol_ptr: int, d_acc_ptr: int, iterations: int, mu_roots: int, threshold: float, scale_log2: int, d_mask_ptr: int = 0,
                        stream: int = 0):
        """photon_piv_volume_mart on raw device pointers: per camera the pointer of its n_frames raw frames f32, their stride
        and the sensor's (height, width); the n_frames volumes f32 at d_vol_ptr, vol_stride apart, are the first guess and
        are updated in place; d_acc_ptr: the workspace int64 [2, n_frames, max height width]; d_mask_ptr: u8 [nz, ny, nx], 1 =
        the voxel stays 0 (0 = NULL).  `iterations` MART iterations with the relaxation 2^-mu_roots; asynchronous on
        `stream`."""
        job = photon_piv_volume_mart_t(n_frames=int(n_frames), iterations=int(iterations), mu_roots=int(mu_roots), scale_log2=int(scale_log2),
                                       threshold=float(threshold), vol_stride=int(vol_stride), d_vol=int(d_vol_ptr) or None,
                                       d_mask=int(d_mask_ptr) or None, d_acc=int(d_acc_ptr) or None, stream=int(stream) or None)
        n = self._volume_cameras(job, sensor_shapes, grids, vol, d_poly_ptr)
        if not len(d_frame_ptrs) == len(frame_strides) == n:
            raise ValueError("piv_volume_mart takes one frame pointer and stride per camera")
        for c in range(n):
            job.d_frame[c], job.frame_stride[c] = int(d_frame_ptrs[c]) or None, int(frame_strides[c])
        self._call("photon_piv_volume_mart", ctypes.byref(job))

    def _los_queued(self, camera_frames, cameras, vol, mode: str, stream: int, dev, mart=None):
        """reconstruct_volume's work, queued on `stream`: (volumes f32 [n, nz, ny, nx], mask u8 [nz, ny, nx], whether
        camera_frames held single frames).  mart: None, or _mart_settings' tuple."""
        import torch
        from . import piv_tomo as pt
        if mode not in pt.MODES:
            raise ValueError(f'mode must be one of {sorted(pt.MODES)}, not {mode!r}')
        if not 2 <= len(cameras) <= 8 or len(camera_frames) != len(cameras):
            raise ValueError("a line-of-sight volume takes 2 to 8 cameras and one frame or stack of frames per camera")
        checked = [_checked(x, f"camera_frames[{c}]") for c, x in enumerate(camera_frames)]
        if any(x is None or x.ndim not in (2, 3) or x.ndim != checked[0].ndim for x in checked):
            raise ValueError("camera_frames must hold one frame [height, width] or one stack [n, height, width] per camera, all alike")
        stacks = [_on_device(x, torch.float32, dev, f"camera_frames[{c}]") for c, x in enumerate(checked)]
        stacks = [t.reshape((-1,) + tuple(t.shape[-2:])) for t in stacks]
        n = int(stacks[0].shape[0])
        if any(int(t.shape[0]) != n for t in stacks):
            raise ValueError("every camera must bring the same number of frames")
        poly, grids = pt.los_coefficients(cameras, vol)
        d_poly = _on_device(poly, torch.float64, dev, "poly")
        coefs = [self._coefficients_of(t, stream) for t in stacks]
        nz, ny, nx = int(vol["nz"]), int(vol["ny"]), int(vol["nx"])
        out = torch.empty((n, nz, ny, nx), dtype=torch.float32, device=dev)
        unseen = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
        self.piv_volume_los([c.data_ptr() for c in coefs], [int(c.shape[1] * c.shape[2]) for c in coefs], n, [tuple(c.shape[1:]) for c in coefs],
                            grids, d_poly.data_ptr(), vol, nz * ny * nx, out.data_ptr(), unseen.data_ptr(), pt.MODES[mode], stream)
        if mart is not None:            # the iterations on the frames themselves, behind the first guess on the same stream
            iterations, roots, threshold, scale_log2 = mart
            acc = torch.empty((2, n, max(int(t.shape[1] * t.shape[2]) for t in stacks)), dtype=torch.int64, device=dev)
            self.piv_volume_mart([t.data_ptr() for t in stacks], [int(t.shape[1] * t.shape[2]) for t in stacks], n, [tuple(t.shape[1:]) for t in stacks],
                                 grids, d_poly.data_ptr(), vol, nz * ny * nx, out.data_ptr(), acc.data_ptr(), iterations, roots, threshold, scale_log2,
                                 unseen.data_ptr(), stream)
        return out, unseen, checked[0].ndim == 2

    @staticmethod
    def _mart_settings(method: str, mode: str, camera_frames, iterations, relaxation, threshold, scale_log2):
        """The drivers' method= / reconstruction= on the host: None for "los"; for "mart" (iterations, mu_roots, threshold,
        scale_log2), the last two chosen from the frames' maximum where the caller gives None (piv_mart.default_threshold,
        scale_log2_for: read on the host; frames that are device tensors are read back first, one more wait)."""
        from . import piv_mart as pm
        if method not in ("los", "mart"):
            raise ValueError(f'the reconstruction must be "los" or "mart", not {method!r}')
        if method == "los":
            return None
        if mode != "min":
            raise ValueError('MART starts from the line-of-sight volume in mode "min"')
        roots = pm.mu_roots_of(relaxation)
        if threshold is None or scale_log2 is None:
            host = [x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x) for x in camera_frames]
            threshold = pm.default_threshold(host) if threshold is None else threshold
            scale_log2 = pm.scale_log2_for(host) if scale_log2 is None else scale_log2
        pm.check_arguments(iterations, roots, threshold, scale_log2)
        return int(iterations), roots, float(threshold), int(scale_log2)

    def reconstruct_volume(self, camera_frames, cameras, vol, mode: str = "min", method: str = "los", iterations: int = 5,
                           relaxation: float = 0.5, threshold: Optional[float] = None, scale_log2: Optional[int] = None):
        """A particle volume from N cameras by line of sight (section 20a; models: photon_amd.piv_tomo.los_model_f32, bit for
        bit, and los_model).  camera_frames: a list with one frame [height, width] or one stack [n, height, width] per
        camera, taken as the ingest rule of this class takes any image (the sensors may differ); cameras: 2 to 8 piv_stereo
        cameras; vol: a piv_tomo volume; mode "min" (MinLOS) or "product" (multiplicative LOS, without the N-th root).  On
        the current stream: the B-spline coefficients per frame, the cameras folded at every slice on the host and uploaded
        (a copy on the current stream), one line-of-sight launch for all frames; nothing waits for the result.  Returns device tensors (volumes f32 [n, nz, ny, nx], or [nz,
        ny, nx] for single frames; mask u8 [nz, ny, nx], 1 where a camera does not see the voxel).
        method "mart": the line-of-sight volume in mode "min" is the first guess of `iterations` MART iterations on the
        frames themselves (section 21b; models: photon_amd.piv_mart.mart_model_f32 of los_model_f32, bit for bit, and
        reconstruct_model), on the same stream, nothing waits.  relaxation: 1, 0.5, 0.25 or 0.125; threshold: voxels below it
        become 0 (None: 1e-4 of the frames' maximum); scale_log2: section 21a's fixed-point scale (None: the largest s with 4
        max(frames) 2^s <= 2^31)."""
        dev, stream = _device_and_stream()
        mart = self._mart_settings(method, mode, camera_frames, iterations, relaxation, threshold, scale_log2)
        out, unseen, single = self._los_queued(camera_frames, cameras, vol, mode, stream, dev, mart)
        return (out[0] if single else out), unseen

    def reproject(self, volumes, cameras, vol, sensor_shapes, scale_log2: Optional[int] = None):
        """The images the cameras would see of a particle volume (section 21a; model: photon_amd.piv_mart.project_model, integer
        for integer).  volumes: one volume [nz, ny, nx] or a stack [n, nz, ny, nx], taken as the ingest rule of this class
        takes any array; cameras: 2 to 8 piv_stereo cameras; vol: a piv_tomo volume; sensor_shapes: (height, width) per camera.
        scale_log2: the fixed-point scale (None: the largest s with max(volumes) 2^s <= 2^31, read on the host: a volume on
        the device is waited for).  On the current stream; nothing waits for the result.  Returns two lists of device
        tensors, one entry per camera: (images f32 [n, height, width], accumulators int64 [n, height, width]), [height,
        width] for one volume."""
        import torch
        from . import piv_mart as pm
        from . import piv_tomo as pt
        dev, stream = _device_and_stream()
        checked = _checked(volumes, "volumes")
        if checked is None or checked.ndim not in (3, 4) or tuple(checked.shape[-3:]) != (int(vol["nz"]), int(vol["ny"]), int(vol["nx"])):
            raise ValueError("volumes must be [nz, ny, nx] or [n, nz, ny, nx] of the volume's size")
        if not 2 <= len(cameras) <= 8 or len(sensor_shapes) != len(cameras):
            raise ValueError("a re-projection takes 2 to 8 cameras and one sensor shape per camera")
        d_vol = _on_device(checked, torch.float32, dev, "volumes")
        d_vol = d_vol.reshape((-1,) + tuple(d_vol.shape[-3:]))
        if scale_log2 is None:
            scale_log2 = min(pm.scale_log2_for([d_vol.cpu().numpy()]) + 2, pm.SCALE_LOG2_RANGE[1])
        pm.check_scale(scale_log2)
        poly, grids = pt.los_coefficients(cameras, vol)
        d_poly = _on_device(poly, torch.float64, dev, "poly")
        n, shapes = int(d_vol.shape[0]), [(int(h), int(w)) for h, w in sensor_shapes]
        acc = [torch.empty((n, h, w), dtype=torch.int64, device=dev) for h, w in shapes]
        images = [torch.empty((n, h, w), dtype=torch.float32, device=dev) for h, w in shapes]
        self.piv_volume_project(d_vol.data_ptr(), int(d_vol.shape[1] * d_vol.shape[2] * d_vol.shape[3]), n, shapes, grids, d_poly.data_ptr(), vol,
                                [a.data_ptr() for a in acc], [h * w for h, w in shapes], int(scale_log2), [i.data_ptr() for i in images], stream)
        if checked.ndim == 3:
            return [i[0] for i in images], [a[0] for a in acc]
        return images, acc

    def correlate_tomo(self, camera_frames, cameras, vol, win: int = 32, step: int = 16, radius: int = 4, win_z: Optional[int] = None,
                       step_z: Optional[int] = None, radius_z: Optional[int] = None, mode: str = "min", offsets=None,
                       reconstruction: str = "los", iterations: int = 5, relaxation: float = 0.5, threshold: Optional[float] = None,
                       scale_log2: Optional[int] = None):
        """Three displacement components on a 3-D grid from N cameras (section 20; model:
        photon_amd.piv_tomo.correlate_tomo_model).  camera_frames: a list with the two exposures of each camera, a stack [2,
        height, width], taken as the ingest rule of this class takes any stack; cameras, vol, mode as reconstruct_volume
        takes them.  win_z defaults to win, capped at 64 and nz; step_z to max(1, win_z / 2); radius_z to min(radius, 16,
        win_z / 2).  offsets: integer (ox, oy, oz) per node [n_slabs, n_rows, n_cols, 3] in voxels, or None.  On the current
        stream: both exposures through one line-of-sight launch, then the 3-D correlation; the host waits once.
        reconstruction "mart" with iterations, relaxation, threshold and scale_log2 as reconstruct_volume(method="mart")
        takes them: the MART iterations between the two, on the same stream (model: photon_amd.piv_mart.mart_tomo_model).
        Returns numpy (displacements f64 [n_slabs, n_rows, n_cols, 3] = pitch (dx, dy, dz) in world units; vectors f32
        [n_slabs, n_rows, n_cols, 5] = dx, dy, dz in voxels, peak, ratio; flags int32 [n_slabs, n_rows, n_cols]; partial bool
        [n_slabs, n_rows, n_cols], true where the window holds a voxel some camera does not see)."""
        import torch
        from . import piv_tomo as pt
        win_z, step_z, radius_z = pt.z_defaults(vol, win, radius, win_z, step_z, radius_z)
        pt.check_arguments((int(vol["nz"]), int(vol["ny"]), int(vol["nx"])), win, step, radius, win_z, step_z, radius_z)
        mart = self._mart_settings(reconstruction, mode, camera_frames, iterations, relaxation, threshold, scale_log2)
        dev, stream = _device_and_stream()
        d_off = None
        if offsets is not None:
            grid = pt.grid_shape((int(vol["nz"]), int(vol["ny"]), int(vol["nx"])), win, step, win_z, step_z)
            table = _checked(offsets, "offsets")
            if tuple(table.shape) != grid + (3,):
                raise ValueError(f"offsets must be {grid + (3,)}: (ox, oy, oz) per node, not {tuple(table.shape)}")
            d_off = _on_device(table, torch.float64, dev, "offsets").to(torch.int32).contiguous()      # whole numbers: exact in f64
        volumes, unseen, _ = self._los_queued(camera_frames, cameras, vol, mode, stream, dev, mart)
        if volumes.shape[0] != 2:
            raise ValueError("correlate_tomo takes the two exposures of each camera, [2, height, width]")
        nz, ny, nx = (int(v) for v in volumes.shape[1:])
        vectors, flags, _ = self.piv_correlate_volume(volumes[0].data_ptr(), volumes[1].data_ptr(), nx, ny, nz, win, step, radius, win_z, step_z,
                                                      radius_z, 0 if d_off is None else d_off.data_ptr(), stream)
        # a window holds an unseen voxel where the mask's maximum over the window is 1
        pooled = torch.nn.functional.max_pool3d(unseen[None, None].to(torch.float32), (win_z, win, win), (step_z, step, step))[0, 0]
        vectors, flags, partial = vectors.cpu().numpy(), flags.cpu().numpy(), (pooled > 0).cpu().numpy()       # the host waits here
        return float(vol["pitch"]) * vectors[..., :3].astype(np.float64), vectors, flags, partial

    # ---- dense optical flow on the device (section 12) --------------------------------------------------------------------
    def field_to_pixels(self, d_field_ptr: int, field_stride: int, n_rows: int, n_cols: int, win: int, step: int, width: int, height: int,
                        d_dense_ptr: int, stream: int = 0):
        """photon_piv_field_to_pixels on raw device pointers: the grid's field at every pixel, f32 [height, width, 2]."""
        self._call("photon_piv_field_to_pixels", _vp(d_field_ptr), int(field_stride), int(n_rows), int(n_cols), int(win), int(step), int(width),
                   int(height), _vp(d_dense_ptr), _vp(stream))

    def piv_deform_dense(self, d_coef_ptr: int, width: int, height: int, d_dense_ptr: int, scale: float, d_out_ptr: int, stream: int = 0):
        """photon_piv_deform_dense on raw device pointers: the image of the coefficients warped by scale x a per-pixel field."""
        self._call("photon_piv_deform_dense", _vp(d_coef_ptr), int(width), int(height), _vp(d_dense_ptr), float(scale), _vp(d_out_ptr),
                   _vp(stream))

    def optflow_terms(self, d_w1_ptr: int, d_w2_ptr: int, width: int, height: int, d_u0_ptr: int, gain: float, alpha2: float,
                      d_terms_ptr: int, stream: int = 0):
        """photon_optflow_terms on raw device pointers (d_u0_ptr: 0 = a zero field): (Ix, Iy, c, w) per pixel."""
        self._call("photon_optflow_terms", _vp(d_w1_ptr), _vp(d_w2_ptr), int(width), int(height), _vp(d_u0_ptr), float(gain), float(alpha2),
                   _vp(d_terms_ptr), _vp(stream))

    def optflow_iterations_per_launch(self) -> int:
        """T of photon_optflow_iterate: the sweeps one launch performs."""
        return int(self.lib.photon_optflow_iterations_per_launch())

    def optflow_iterate(self, d_terms_ptr: int, d_u_ptr: int, width: int, height: int, iterations: int, d_out_ptr: int,
                        d_tmp_ptr: int = 0, stream: int = 0):
        """photon_optflow_iterate on raw device pointers (d_tmp_ptr: 0 = NULL, accepted up to T iterations)."""
        self._call("photon_optflow_iterate", _vp(d_terms_ptr), _vp(d_u_ptr), int(width), int(height), int(iterations), _vp(d_out_ptr),
                   _vp(d_tmp_ptr), _vp(stream))

    def optical_flow(self, im1, im2, predictor=None, win: int = 32, step: int = 16, alpha2: float = 5.0, warps: int = 3,
                     iterations: int = 48, return_grid: bool = False):
        """Dense displacement field of an image pair by optical flow (section 12; model:
        photon_amd.optical_flow.optical_flow_model).  predictor: a vector grid [n_rows, n_cols, >= 2] of (win, step), numpy
        or a device tensor, spread to the pixels on the device; or a dense field [height, width, 2]; or None: one iteration
        of correlate_deform, kept on the device.  Per warp both frames are warped half-way by the current field, then the
        data terms and `iterations` Jacobi sweeps.  Returns the field as numpy f32 [height, width, 2]; with return_grid also
        the field at section 5's window centres [n_rows, n_cols, 2].  Everything runs on the current stream; the host waits
        for the gain 1 / std(im1) (a scalar the terms take by value; the first kernels are queued before it) and for the
        result."""
        import torch
        from . import optical_flow as of
        predictor = _checked(predictor, "predictor", 3)
        dev, stream, a, b, h, w = _image_pair(im1, im2)
        of.check_driver_arguments(alpha2, warps, iterations)
        inv_std = 1.0 / torch.std(a, correction=0)
        if predictor is None:
            from . import piv_multigrid as pm
            levels = pm.check_schedule((h, w), ((win, step),), (1,), radius=None, residual_radius=4, method="direct")
            predictor = self._deform_chain(a, b, *levels, _Correlator((win,)).on_device(self, (h, w), dev))[0]
        pred = _on_device(predictor, torch.float32, dev, "predictor", 3)
        field = torch.empty((2, h, w, 2), dtype=torch.float32, device=dev)      # the current field and the next one
        if of.predictor_shape(pred.shape, (h, w), win, step) == "grid":
            pred = (pred if pred.shape[2] in (2, 4) else pred[..., :2]).contiguous()
            self.field_to_pixels(pred.data_ptr(), int(pred.shape[2]), int(pred.shape[0]), int(pred.shape[1]), win, step, w, h,
                                 field[0].data_ptr(), stream)
        else:
            field[0].copy_(pred)
        terms = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
        tmp = torch.empty((h, w, 2), dtype=torch.float32, device=dev) if int(iterations) > self.optflow_iterations_per_launch() else None
        coef, warped = self._frame_coefficients(a, b, stream)
        gain = float(inv_std)
        cur = 0
        for _ in range(int(warps)):
            u = field[cur]
            self.piv_deform_dense(coef[0].data_ptr(), w, h, u.data_ptr(), -0.5, warped[0].data_ptr(), stream)
            self.piv_deform_dense(coef[1].data_ptr(), w, h, u.data_ptr(), 0.5, warped[1].data_ptr(), stream)
            self.optflow_terms(warped[0].data_ptr(), warped[1].data_ptr(), w, h, u.data_ptr(), gain, alpha2, terms.data_ptr(), stream)
            self.optflow_iterate(terms.data_ptr(), u.data_ptr(), w, h, iterations, field[cur ^ 1].data_ptr(),
                                 tmp.data_ptr() if tmp is not None else 0, stream)
            cur ^= 1
        dense = field[cur].cpu().numpy()
        return (dense, of.sample_at_window_centres(dense, win, step)) if return_grid else dense

    # ---- dot tracking on the device (section 8) ---------------------------------------------------------------------------
    def dots_scratch_bytes(self, width: int, height: int, radius: Optional[float] = None, max1: int = 0, max2: int = 0) -> int:
        """Bytes of device scratch dots_detect needs for a width x height image, or with `radius` what dots_match needs for
        that radius and the capacities max1, max2 (0: arguments the call would refuse)."""
        if radius is None:
            return int(self.lib.photon_dots_detect_scratch_bytes(int(width), int(height)))
        return int(self.lib.photon_dots_match_scratch_bytes(int(width), int(height), float(radius), int(max1), int(max2)))

    def dots_image_max(self, d_im_ptr: int, width: int, height: int, d_max_ptr: int, stream: int = 0):
        """photon_dots_image_max on raw device pointers: the largest finite pixel into the device f32 at d_max_ptr."""
        self._call("photon_dots_image_max", _vp(d_im_ptr), int(width), int(height), _vp(d_max_ptr), _vp(stream))

    def dots_detect(self, d_im_ptr: int, width: int, height: int, threshold: float, d_scale_ptr: int, max_dots: int, d_peaks_ptr: int,
                    d_count_ptr: int, d_scratch_ptr: int, scratch_bytes: int, stream: int = 0):
        """photon_dots_detect on raw device pointers (d_scale_ptr: 0 = NULL), asynchronous on `stream`."""
        self._call("photon_dots_detect", _vp(d_im_ptr), int(width), int(height), float(threshold), _vp(d_scale_ptr), int(max_dots),
                   _vp(d_peaks_ptr), _vp(d_count_ptr), _vp(d_scratch_ptr), int(scratch_bytes), _vp(stream))

    def dots_fit(self, d_im_ptr: int, width: int, height: int, d_peaks_ptr: int, d_count_ptr: int, max_dots: int, box_radius: int,
                 sigma_w: float, iterations: int, background: float, d_dots_ptr: int, d_status_ptr: int, stream: int = 0):
        """photon_dots_fit on raw device pointers, asynchronous on `stream`."""
        self._call("photon_dots_fit", _vp(d_im_ptr), int(width), int(height), _vp(d_peaks_ptr), _vp(d_count_ptr), int(max_dots), int(box_radius),
                   float(sigma_w), int(iterations), float(background), _vp(d_dots_ptr), _vp(d_status_ptr), _vp(stream))

    def dots_match(self, d_dots1_ptr: int, d_status1_ptr: int, d_count1_ptr: int, max1: int, d_dots2_ptr: int, d_status2_ptr: int,
                   d_count2_ptr: int, max2: int, radius: float, width: int, height: int, d_pair_ptr: int, d_shift_ptr: int,
                   d_npaired_ptr: int, d_scratch_ptr: int, scratch_bytes: int, d_field_ptr: int = 0, field_stride: int = 2,
                   n_rows: int = 0, n_cols: int = 0, win: int = 0, step: int = 0, reject_mask: int = 0, stream: int = 0):
        """photon_dots_match on raw device pointers (d_field_ptr: 0 = no predictor), asynchronous on `stream`."""
        self._call("photon_dots_match", _vp(d_dots1_ptr), _vp(d_status1_ptr), _vp(d_count1_ptr), int(max1), _vp(d_dots2_ptr), _vp(d_status2_ptr),
                   _vp(d_count2_ptr), int(max2), int(reject_mask), _vp(d_field_ptr), int(field_stride), int(n_rows), int(n_cols), int(win),
                   int(step), float(radius), int(width), int(height), _vp(d_pair_ptr), _vp(d_shift_ptr), _vp(d_npaired_ptr), _vp(d_scratch_ptr),
                   int(scratch_bytes), _vp(stream))

    def dots_window_means(self, d_dots1_ptr: int, d_pair_ptr: int, d_shift_ptr: int, d_count1_ptr: int, max1: int, width: int,
                          height: int, win: int, step: int, min_count: int, anchor: int, d_vectors_ptr: int, d_flags_ptr: int,
                          stream: int = 0):
        """photon_dots_window_means on raw device pointers, asynchronous on `stream`."""
        self._call("photon_dots_window_means", _vp(d_dots1_ptr), _vp(d_pair_ptr), _vp(d_shift_ptr), _vp(d_count1_ptr), int(max1), int(width),
                   int(height), int(win), int(step), int(min_count), int(anchor), _vp(d_vectors_ptr), _vp(d_flags_ptr), _vp(stream))

    def correlation_predictor(self, im1, im2, win: int = 32, step: int = 16, radius: Optional[int] = None, eps: float = 0.1,
                              threshold: float = 2.0, method: str = "direct", window_sigma: Optional[float] = None, diameter: float = 2.5,
                              mask=None, min_valid_fraction: float = 0.5, fill_masked: bool = False, weighting=None):
        """A predictor for track_dots from one pass of window correlation: photon_piv_correlate, then photon_piv_validate
        (median test, replacement, 3 x 3 smoothing) -- pass 0 of correlate_deform.  Returns the smoothed field as a torch
        device tensor [n_rows, n_cols, 2], queued on the current stream: hand it to track_dots as predictor=(field, win, step)
        and a displacement larger than the spacing of the dots no longer pairs a dot with its neighbour.  method, window_sigma,
        diameter: the correlator, as ``correlate`` takes them.  mask, min_valid_fraction: as ``correlate`` takes them.  The
        smoothed field carries the neighbours' median across masked-out nodes; as in the other drivers fill_masked=False
        returns NaN there (set on the device, nothing waits), and a caller who hands the field on as a predictor wants
        fill_masked=True: a node that is not finite reads as (0, 0) in every warp.  weighting: as ``correlate`` takes it."""
        im1, im2, _ = _checked_pair(im1, im2, mask)
        correlator = _Correlator((win,), method, window_sigma=window_sigma, diameter=diameter, mask=mask,
                                 min_valid_fraction=min_valid_fraction, weighting=weighting)
        dev, stream, a, b, h, w = _pair_on_device(im1, im2)
        correlate, radius, check = correlator.on_device(self, (h, w), dev).at(win, radius)
        check((h, w), win, step, radius)
        settings = _DeformSettings(eps=eps, threshold=threshold)
        _, _, smoothed, status = self._correlate_validated(correlate, a, b, (win, step), radius, settings, stream)
        return smoothed if mask is None or fill_masked else _nan_where_masked_out(smoothed, status)

    def track_dots(self, im1, im2, threshold: float, box_radius: int = 3, sigma_w: float = 1.0, iterations: int = 4,
                   background: float = 0.0, radius: float = 3.0, predictor=None, max_dots: Optional[int] = None, grid=None,
                   relative: bool = False, reject_mask: int = 0) -> dict:
        """Per-dot shifts of an image pair (section 8; model: photon_amd.dot_tracking.track_dots_model, the same keys):
        detect and locate the dots of both frames, pair them within `radius` px of frame 1's position (plus the predictor:
        None, or (field [n_rows, n_cols, 2 or 4], win, step) as correlate / correlate_deform return it), and with
        grid = (win, step, min_count, anchor) average the pairs onto section 5's window grid.  relative: `threshold` is a
        fraction of each image's maximum, taken on the device.  max_dots None = one dot per 32 pixels, at least 1024.
        Returns numpy: dots1 / dots2 [n, 4] = x, y, peak, diameter; status1 / status2; count1 / count2 (what detect
        found: above max_dots the first max_dots were kept); pair [n1]; shift [n1, 4] = x_mid, y_mid, dx, dy; npaired;
        vectors [n_rows, n_cols, 4] = mean dx, mean dy, count, rms and flags with a grid.  Everything runs on the current
        stream from torch-allocated buffers; the host waits once, for the result."""
        import torch
        from . import dot_tracking as dt
        from . import piv_correlation as pc
        if predictor is not None:
            predictor = (_checked(predictor[0], "the predictor field", 3), *predictor[1:])
        dev, stream, a, b, h, w = _image_pair(im1, im2)
        cap = dt.default_max_dots((h, w)) if max_dots is None else int(max_dots)
        det_bytes = self.dots_scratch_bytes(w, h)
        mat_bytes = self.dots_scratch_bytes(w, h, radius, cap, cap) if cap >= 1 and radius > 0 else 0
        scratch = torch.empty(max(det_bytes, mat_bytes, 16), dtype=torch.uint8, device=dev)   # the calls are ordered on one stream
        ints = torch.empty((2, cap + 1), dtype=torch.int32, device=dev)        # per frame: peaks [cap], count
        dots = torch.empty((2, cap, 4), dtype=torch.float32, device=dev)
        status = torch.empty((2, cap), dtype=torch.int32, device=dev)
        top = torch.empty(2, dtype=torch.float32, device=dev)
        for f, im in enumerate((a, b)):
            d_scale = 0
            if relative:
                d_scale = top[f].data_ptr()
                self.dots_image_max(im.data_ptr(), w, h, d_scale, stream)
            self.dots_detect(im.data_ptr(), w, h, threshold, d_scale, cap, ints[f].data_ptr(), ints[f, cap:].data_ptr(),
                             scratch.data_ptr(), scratch.numel(), stream)
            self.dots_fit(im.data_ptr(), w, h, ints[f].data_ptr(), ints[f, cap:].data_ptr(), cap, box_radius, sigma_w, iterations,
                          background, dots[f].data_ptr(), status[f].data_ptr(), stream)
        pair = torch.empty(cap + 1, dtype=torch.int32, device=dev)             # pair [cap], npaired
        shift = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        field_args = {}
        if predictor is not None:
            field, pwin, pstep = predictor
            fld = _on_device(field, torch.float32, dev, "the predictor field", 3)
            if fld.shape[2] not in (2, 4):
                raise ValueError("the predictor field must be [n_rows, n_cols, 2 or 4]")
            field_args = dict(d_field_ptr=fld.data_ptr(), field_stride=int(fld.shape[2]), n_rows=int(fld.shape[0]), n_cols=int(fld.shape[1]),
                              win=int(pwin), step=int(pstep))
        self.dots_match(dots[0].data_ptr(), status[0].data_ptr(), ints[0, cap:].data_ptr(), cap, dots[1].data_ptr(), status[1].data_ptr(),
                        ints[1, cap:].data_ptr(), cap, radius, w, h, pair.data_ptr(), shift.data_ptr(), pair[cap:].data_ptr(),
                        scratch.data_ptr(), scratch.numel(), reject_mask=reject_mask, stream=stream, **field_args)
        vectors = flags = None
        if grid is not None:
            win, step, min_count, anchor = grid
            if int(win) < 1 or int(step) < 1 or h < int(win) or w < int(win):
                raise ValueError(f"no window grid of win {win}, step {step} on a {h} x {w} image")
            r, c = pc.grid_shape((h, w), win, step)
            vectors = torch.empty((r, c, 4), dtype=torch.float32, device=dev)
            flags = torch.empty((r, c), dtype=torch.int32, device=dev)
            self.dots_window_means(dots[0].data_ptr(), pair.data_ptr(), shift.data_ptr(), ints[0, cap:].data_ptr(), cap, w, h, win, step,
                                   min_count, anchor, vectors.data_ptr(), flags.data_ptr(), stream)
        counts = ints[:, cap].cpu().numpy()                                     # the one host wait
        n1, n2 = (min(int(c), cap) for c in counts)
        out = {"dots1": dots[0, :n1].cpu().numpy(), "dots2": dots[1, :n2].cpu().numpy(), "status1": status[0, :n1].cpu().numpy(),
               "status2": status[1, :n2].cpu().numpy(), "count1": int(counts[0]), "count2": int(counts[1]),
               "pair": pair[:n1].cpu().numpy(), "shift": shift[:n1].cpu().numpy(), "npaired": int(pair[cap].item())}
        if grid is not None:
            out["vectors"], out["flags"] = vectors.cpu().numpy(), flags.cpu().numpy()
        return out

    # ---- gradient-field integration on the device (photon_integrate_gradient) ------------------------------------
    def integrate_gradient_ptr(self, d_gx_ptr: int, d_gy_ptr: int, nx: int, ny: int, d_phi_ptr: int, d_w_ptr: int = 0,
                               d_fixed_ptr: int = 0, d_value_ptr: int = 0, hx: float = 1.0, hy: float = 1.0, tol: float = 1e-8,
                               max_iter: Optional[int] = None, stream: int = 0) -> dict:
        """Integrate a device gradient field (raw pointers: f64 gx, gy, w, value and u8 fixed, row-major ny x nx; 0 = NULL)
        into the device f64 array at d_phi_ptr.  Returns the stats as a dict; the call has synchronised `stream`.
        max_iter None = 20 max(nx, ny).  The definition: include/parallel_ray_tracing.h, section 6
        (photon_amd.bos_density: host model)."""
        from .bos_density import default_max_iter
        max_iter = default_max_iter(nx, ny) if max_iter is None else int(max_iter)
        st = photon_integrate_stats_t()
        self._call("photon_integrate_gradient", *(_vp(v) for v in (d_gx_ptr, d_gy_ptr, d_w_ptr, d_fixed_ptr, d_value_ptr)), int(nx), int(ny),
                   float(hx), float(hy), float(tol), max_iter, _vp(d_phi_ptr), ctypes.byref(st), _vp(stream))
        return st.as_dict()

    def integrate_gradient(self, gx, gy, w=None, fixed=None, value=None, hx: float = 1.0, hy: float = 1.0, tol: float = 1e-8,
                           max_iter: Optional[int] = None):
        """Weighted least-squares integration of a gradient field on the device (numpy arrays or torch device tensors,
        [ny, nx]; gx along +column, gy along +row).  w: weights (None = 1); fixed: Dirichlet mask (None = the outer frame);
        value: values at the fixed nodes (None = 0).  Returns (phi numpy f64 [ny, nx], stats dict); phi is NaN on the
        unknown nodes that reach no fixed node.  max_iter None = 20 max(nx, ny)."""
        import torch
        from . import bos_density
        gx, gy, w, fixed, value = (_checked(a, name, 2) for a, name in ((gx, "gx"), (gy, "gy"), (w, "w"), (fixed, "fixed"), (value, "value")))
        if gx is None or gy is None or tuple(gx.shape) != tuple(gy.shape):
            raise ValueError("gx and gy must be two 2-d arrays of one shape")
        for name, t in (("w", w), ("fixed", fixed), ("value", value)):
            if t is not None and tuple(t.shape) != tuple(gx.shape):
                raise ValueError(f"{name} must have the shape of gx, {tuple(gx.shape)}")
        dev, stream = _device_and_stream()
        tgx, tgy = _on_device(gx, torch.float64, dev, "gx", 2), _on_device(gy, torch.float64, dev, "gy", 2)
        ny, nx = tgx.shape
        tw, tv = _on_device(w, torch.float64, dev, "w", 2), _on_device(value, torch.float64, dev, "value", 2)
        tf = _on_device(fixed, torch.uint8, dev, "fixed", 2, nonzero=True)
        bos_density.check_arguments(nx, ny, hx, hy, tol, bos_density.default_max_iter(nx, ny) if max_iter is None else max_iter)
        phi = torch.empty((ny, nx), dtype=torch.float64, device=dev)
        stats = self.integrate_gradient_ptr(tgx.data_ptr(), tgy.data_ptr(), nx, ny, phi.data_ptr(),
                                            tw.data_ptr() if tw is not None else 0, tf.data_ptr() if tf is not None else 0,
                                            tv.data_ptr() if tv is not None else 0, hx, hy, tol, max_iter, stream=stream)
        return phi.cpu().numpy(), stats

    # ---- tomography on the device (include/parallel_ray_tracing.h, section 9) ----------------------------------------
    @staticmethod
    def _tomo_grid(dims, spacing, origin):
        """nx, ny, nz, spacing, origin as the tomography entry points take them (a scalar spacing stands for all three)."""
        og = _f64x3(origin)
        if og.shape != (3,):
            raise ValueError("origin must hold three values")
        nx, ny, nz = (int(n) for n in dims)
        return nx, ny, nz, _ptr(_f64x3(spacing, scalar_ok=True)), _ptr(og)

    def tomo_project(self, d_f_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int, n_rays: int, d_p_ptr: int,
                     stream: int = 0):
        """P = A f on raw device pointers (f64: f [nz, ny, nx], origins and dirs [n_rays, 3], p [n_rays]; dims = (nx, ny,
        nz)).  Asynchronous on `stream`."""
        grid = self._tomo_grid(dims, spacing, origin)
        self._call("photon_tomo_project", _vp(d_f_ptr), *grid, _vp(d_origins_ptr), _vp(d_dirs_ptr), int(n_rays), _vp(d_p_ptr), _vp(stream))

    def tomo_backproject(self, d_y_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int, n_rays: int, d_v_ptr: int,
                         stream: int = 0):
        """v += A^T y on raw device pointers (f64: y [n_rays], v [nz, ny, nx]): adds into v.  Asynchronous on `stream`."""
        grid = self._tomo_grid(dims, spacing, origin)
        self._call("photon_tomo_backproject", _vp(d_y_ptr), *grid, _vp(d_origins_ptr), _vp(d_dirs_ptr), int(n_rays), _vp(d_v_ptr), _vp(stream))

    def _tomo_solve_ptr(self, entry: str, d_data_ptrs, dims, spacing, origin, d_ray_ptrs, n_rays, d_f_ptr, d_w_ptr, d_support_ptr, lam, tol,
                        max_iter, stream) -> dict:
        """photon_tomo_reconstruct or photon_tomo_reconstruct_deflections (`entry`) on raw pointers: d_data_ptrs the data
        over the rays (p, or g1 and g2), d_ray_ptrs origins and dirs (and t1, t2)."""
        from .tomography import DEFAULT_MAX_ITER
        grid = self._tomo_grid(dims, spacing, origin)
        st = photon_tomo_stats_t()
        self._call(entry, *(_vp(d) for d in d_data_ptrs), _vp(d_w_ptr), _vp(d_support_ptr), *grid, *(_vp(d) for d in d_ray_ptrs), int(n_rays),
                   float(lam), float(tol), DEFAULT_MAX_ITER if max_iter is None else int(max_iter), _vp(d_f_ptr), ctypes.byref(st), _vp(stream))
        return st.as_dict()

    def _tomo_solve(self, entry: str, data, names: str, dims, spacing, origin, rays, ray_names: str, w, support, lam, tol, max_iter):
        """tomo_reconstruct and tomo_reconstruct_deflections: `data` the arrays over the rays (p, or g1 and g2), `rays` those
        of three values per ray (origins and dirs, and t1, t2); the names are the message's."""
        import torch
        from . import tomography
        nx, ny, nz = (int(n) for n in dims)
        data_names, rays_names = names.split(", "), ray_names.replace(" and ", ", ").split(", ")      # the messages' names, one per array
        assert len(data_names) == len(data) and len(rays_names) == len(rays), (names, ray_names)
        rays = [_checked(a, name) for a, name in zip(rays, rays_names)]
        data = [_checked(a, name) for a, name in zip(data, data_names)]
        w, support = _checked(w, "w"), _checked(support, "support", 3)
        if any(a is None for a in (*rays, *data)):
            raise TypeError(f"{names}, {ray_names} must be arrays, not None")
        n_rays = int(np.prod(data[0].shape))
        if any(int(np.prod(a.shape)) != 3 * n_rays for a in rays) or any(int(np.prod(a.shape)) != n_rays for a in data) \
                or (w is not None and int(np.prod(w.shape)) != n_rays):
            raise ValueError(f"{names} and w hold one value per ray, {ray_names} three")
        if support is not None and tuple(support.shape) != (nz, ny, nx):
            raise ValueError(f"support must be [nz, ny, nx] = {(nz, ny, nx)}")
        dev, stream = _device_and_stream()
        rays = [_on_device(a, torch.float64, dev, name).reshape(-1, 3) for a, name in zip(rays, rays_names)]
        data = [_on_device(a, torch.float64, dev, name).reshape(-1) for a, name in zip(data, data_names)]
        tw = _on_device(w, torch.float64, dev, "w")
        ts = _on_device(support, torch.uint8, dev, "support", 3, nonzero=True)
        max_iter = tomography.DEFAULT_MAX_ITER if max_iter is None else int(max_iter)
        tomography.check_arguments(dims, _f64x3(spacing, scalar_ok=True), origin, n_rays, lam, tol, max_iter)
        f = torch.empty((nz, ny, nx), dtype=torch.float64, device=dev)
        stats = self._tomo_solve_ptr(entry, [a.data_ptr() for a in data], dims, spacing, origin, [a.data_ptr() for a in rays], n_rays,
                                     f.data_ptr(), tw.data_ptr() if tw is not None else 0, ts.data_ptr() if ts is not None else 0, lam, tol,
                                     max_iter, stream)
        return f.cpu().numpy(), stats

    def tomo_reconstruct_ptr(self, d_p_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int, n_rays: int, d_f_ptr: int,
                             d_w_ptr: int = 0, d_support_ptr: int = 0, lam: float = 1.0, tol: float = 1e-6,
                             max_iter: Optional[int] = None, stream: int = 0) -> dict:
        """Solve for the device f64 field at d_f_ptr [nz, ny, nx] from the projections at d_p_ptr (raw pointers: f64 p, w,
        origins, dirs; u8 support; 0 = NULL).  Returns the stats as a dict; the call has synchronised `stream`.  max_iter
        None = tomography.DEFAULT_MAX_ITER."""
        return self._tomo_solve_ptr("photon_tomo_reconstruct", (d_p_ptr,), dims, spacing, origin, (d_origins_ptr, d_dirs_ptr), n_rays,
                                    d_f_ptr, d_w_ptr, d_support_ptr, lam, tol, max_iter, stream)

    def tomo_reconstruct(self, p, dims, spacing, origin, origins, dirs, w=None, support=None, lam: float = 1.0, tol: float = 1e-6,
                         max_iter: Optional[int] = None):
        """The 3-D field from projections along rays, on the device (numpy arrays or torch device tensors): p, w [n_rays]
        (w None = 1; a ray whose p or w is not finite or whose w <= 0 takes no part), origins and dirs [n_rays, 3] world
        microns, support [nz, ny, nx] (None = every voxel), lam the dimensionless smoothness weight.  Returns (f numpy f64
        [nz, ny, nx], stats dict).  The definition: include/parallel_ray_tracing.h, section 9 (photon_amd.tomography: host
        model, and view_rays / grid_of for the geometry)."""
        return self._tomo_solve("photon_tomo_reconstruct", (p,), "p", dims, spacing, origin, (origins, dirs), "origins and dirs", w, support,
                                lam, tol, max_iter)

    # ---- tomography from deflections (include/parallel_ray_tracing.h, section 10) -------------------------------------
    def tomo_deflect(self, d_f_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int, d_t1_ptr: int, d_t2_ptr: int,
                     n_rays: int, d_g1_ptr: int, d_g2_ptr: int, stream: int = 0):
        """g1 = D_t1 f, g2 = D_t2 f on raw device pointers (f64: f [nz, ny, nx]; origins, dirs, t1, t2 [n_rays, 3]; g1, g2
        [n_rays]).  Asynchronous on `stream`."""
        grid = self._tomo_grid(dims, spacing, origin)
        self._call("photon_tomo_deflect", _vp(d_f_ptr), *grid, _vp(d_origins_ptr), _vp(d_dirs_ptr), _vp(d_t1_ptr),
                   _vp(d_t2_ptr), int(n_rays), _vp(d_g1_ptr), _vp(d_g2_ptr), _vp(stream))

    def tomo_deflect_adjoint(self, d_y1_ptr: int, d_y2_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int,
                             d_t1_ptr: int, d_t2_ptr: int, n_rays: int, d_v_ptr: int, stream: int = 0):
        """v += D_t1^T y1 + D_t2^T y2 on raw device pointers (f64: y1, y2 [n_rays], v [nz, ny, nx]): adds into v.
        Asynchronous on `stream`."""
        grid = self._tomo_grid(dims, spacing, origin)
        self._call("photon_tomo_deflect_adjoint", _vp(d_y1_ptr), _vp(d_y2_ptr), *grid, _vp(d_origins_ptr), _vp(d_dirs_ptr),
                   _vp(d_t1_ptr), _vp(d_t2_ptr), int(n_rays), _vp(d_v_ptr), _vp(stream))

    def tomo_reconstruct_deflections_ptr(self, d_g1_ptr: int, d_g2_ptr: int, dims, spacing, origin, d_origins_ptr: int, d_dirs_ptr: int,
                                         d_t1_ptr: int, d_t2_ptr: int, n_rays: int, d_f_ptr: int, d_w_ptr: int = 0,
                                         d_support_ptr: int = 0, lam: float = 1.0, tol: float = 1e-6, max_iter: Optional[int] = None,
                                         stream: int = 0) -> dict:
        """Solve for the device f64 field at d_f_ptr [nz, ny, nx] from the deflections at d_g1_ptr, d_g2_ptr (raw pointers:
        f64 g1, g2, w, origins, dirs, t1, t2; u8 support; 0 = NULL).  Returns the stats as a dict; the call has synchronised
        `stream`.  max_iter None = tomography.DEFAULT_MAX_ITER."""
        return self._tomo_solve_ptr("photon_tomo_reconstruct_deflections", (d_g1_ptr, d_g2_ptr), dims, spacing, origin,
                                    (d_origins_ptr, d_dirs_ptr, d_t1_ptr, d_t2_ptr), n_rays, d_f_ptr, d_w_ptr, d_support_ptr, lam, tol,
                                    max_iter, stream)

    def tomo_reconstruct_deflections(self, g1, g2, dims, spacing, origin, origins, dirs, t1, t2, w=None, support=None, lam: float = 1.0,
                                     tol: float = 1e-6, max_iter: Optional[int] = None):
        """The 3-D field from the deflections measured along rays, on the device (numpy arrays or torch device tensors):
        g1, g2, w [n_rays] (g_j the integral of grad f . t_j along the ray; w None = 1; a ray whose g1, g2 or w is not
        finite or whose w <= 0 takes no part), origins, dirs, t1, t2 [n_rays, 3] world microns, support [nz, ny, nx] (None
        = every voxel: the mean of f is then 0), lam the dimensionless smoothness weight.  Returns (f numpy f64 [nz, ny,
        nx], stats dict).  The definition: include/parallel_ray_tracing.h, section 10 (photon_amd.tomography: host model,
        and view_rays / view_frames / grid_of for the geometry)."""
        return self._tomo_solve("photon_tomo_reconstruct_deflections", (g1, g2), "g1, g2", dims, spacing, origin, (origins, dirs, t1, t2),
                                "origins, dirs, t1 and t2", w, support, lam, tol, max_iter)

    # ---- volumes ------------------------------------------------------------------------------
    def volume_load_nrrd(self, path: str, interpolation: int = 1) -> "Volume":
        h = ctypes.c_void_p()
        self._call("photon_volume_load_nrrd", path.encode(), int(interpolation), ctypes.byref(h))
        return Volume(self, h)

    def volume_from_density(self, rho: np.ndarray, spacing, origin, interpolation: int = 1) -> "Volume":
        """rho indexed [z, y, x] (x fastest), float32."""
        rho = np.ascontiguousarray(rho, dtype=np.float32)
        nz, ny, nx = rho.shape
        h = ctypes.c_void_p()
        self._call("photon_volume_from_density", _ptr(rho), nx, ny, nz, _ptr(_f64x3(spacing)), _ptr(_f64x3(origin)), int(interpolation),
                   ctypes.byref(h))
        return Volume(self, h)

    def volume_gaussian(self, n, spacing, origin, rho0: float, amp: float, centre, sigma: float,
                        interpolation: int = 1) -> "Volume":
        """rho0 + amp exp(-|r - centre|^2 / 2 sigma^2) evaluated on the device (no host array, no file)."""
        h = ctypes.c_void_p()
        self._call("photon_volume_gaussian", *_gaussian_args(n, spacing, origin, rho0, amp, centre, sigma), int(interpolation), ctypes.byref(h))
        return Volume(self, h)

    def density_gaussian_write_nrrd(self, path: str, n, spacing, origin, rho0: float, amp: float, centre, sigma: float) -> str:
        """The field of volume_gaussian as an NRRD file (evaluated on the device)."""
        self._call("photon_density_gaussian_write_nrrd", path.encode(), *_gaussian_args(n, spacing, origin, rho0, amp, centre, sigma))
        return path

    # ---- sources generated on the device ------------------------------------------------------
    def sources_bos(self, dot_xy, template_xy, z: float, radiance: float) -> "Sources":
        d = np.ascontiguousarray(dot_xy, dtype=np.float64).reshape(-1, 2)
        t = np.ascontiguousarray(template_xy, dtype=np.float64).reshape(-1, 2)
        dx, dy, tx, ty = (np.ascontiguousarray(a) for a in (d[:, 0], d[:, 1], t[:, 0], t[:, 1]))
        h = ctypes.c_void_p()
        self._call("photon_sources_bos", _ptr(dx), _ptr(dy), d.shape[0], _ptr(tx), _ptr(ty), t.shape[0], float(z), float(radiance), ctypes.byref(h))
        return Sources(self, h)

    def sources_piv(self, seed: int, n: int, box_min, box_max, z_object: float, beam_fwhm: float,
                    irradiance_constant: float, diameter_cdf=None) -> "Sources":
        h = ctypes.c_void_p()
        self._call("photon_sources_piv", *_piv_args(seed, n, box_min, box_max, z_object, beam_fwhm, irradiance_constant, diameter_cdf),
                   ctypes.byref(h))
        return Sources(self, h)

    def flow_from_grid(self, u, v, w, spacing, origin) -> "Flow":
        """A steady velocity field (microns per unit of t) on the nodes origin + (i, j, k) * spacing of the PIV field's world
        frame; u, v, w: [nz][ny][nx] (x fastest), stored as f32 (photon_flow_from_grid)."""
        comps = [np.ascontiguousarray(a, dtype=np.float32) for a in (u, v, w)]
        if comps[0].ndim != 3 or any(c.shape != comps[0].shape for c in comps):
            raise ValueError("u, v, w must be three arrays of one shape [nz][ny][nx]")
        nz, ny, nx = comps[0].shape
        h = ctypes.c_void_p()
        self._call("photon_flow_from_grid", _ptr(comps[0]), _ptr(comps[1]), _ptr(comps[2]), nx, ny, nz, _ptr(_f64x3(spacing)), _ptr(_f64x3(origin)),
                   ctypes.byref(h))
        return Flow(self, h)

    def sources_piv_advected(self, seed: int, n: int, box_min, box_max, z_object: float, beam_fwhm: float,
                             irradiance_constant: float, diameter_cdf=None, flow: Optional["Flow"] = None, t: float = 0.0,
                             steps: int = 16, return_world: bool = False):
        """The sources_piv field at time t: every particle moved through `flow` by `steps` RK4 steps
        (photon_sources_piv_advected).  Returns Sources, or (Sources, world_xyz f64 [n][3]) with return_world."""
        world = np.empty((max(int(n), 0), 3), np.float64) if return_world else None
        h = ctypes.c_void_p()
        self._call("photon_sources_piv_advected", *_piv_args(seed, n, box_min, box_max, z_object, beam_fwhm, irradiance_constant, diameter_cdf),
                   flow.handle if flow is not None else None, float(t), int(steps), _ptr(world) if world is not None else None, ctypes.byref(h))
        return (Sources(self, h), world) if return_world else Sources(self, h)

    # ---- scenes -------------------------------------------------------------------------------
    def scene_create_from_sources(self, call: RayTracingCall, sources: "Sources") -> "Scene":
        """Like scene_create, with the light-field sources already in HBM (call's own source arrays unused)."""
        scene = self._scene_create("photon_scene_create_from_sources", call, (sources.handle,))
        scene.num_sources = sources.count()
        return scene

    def scene_create(self, call: RayTracingCall) -> "Scene":
        return self._scene_create("photon_scene_create", call)

    def _scene_create(self, entry: str, call: RayTracingCall, sources=()) -> "Scene":
        """photon_scene_create, or with sources = (handle,) photon_scene_create_from_sources: the same arguments otherwise."""
        sd, ls, elems, centers, planes, sysidx, cam = call.pack()
        h = ctypes.c_void_p()
        self._call(
            entry, ctypes.c_float(call.lens_pitch), ctypes.c_float(call.image_distance), ctypes.byref(sd),
            call.scattering_type.encode(), ctypes.byref(ls), *sources, int(call.lightray_number_per_particle),
            ctypes.c_float(call.beam_wavelength), ctypes.c_float(call.aperture_f_number), len(call.elements),
            _ptr(centers), elems, _ptr(planes), _ptr(sysidx), ctypes.byref(cam),
            ctypes.c_float(call.ray_cone_pitch_ratio), ctypes.byref(h))
        return Scene(self, h, call)


class Volume:
    def __init__(self, lib: PhotonLibrary, handle):
        self._lib, self.handle = lib, handle

    def info(self) -> photon_volume_info_t:
        i = photon_volume_info_t()
        self._lib._call("photon_volume_info", self.handle, ctypes.byref(i))
        return i

    def set_weight_bits(self, bits: int):
        """Trilinear weights: 0 = exact f32, 8 = the texture unit's 8 fractional bits."""
        self._lib._call("photon_volume_set_weight_bits", self.handle, int(bits))

    def download(self, coefficients: bool = False) -> np.ndarray:
        i = self.info()
        out = np.empty((i.nz, i.ny, i.nx, 4), np.float32)
        self._lib._call("photon_volume_download", self.handle, int(coefficients), _ptr(out))
        return out

    def sample(self, coords: np.ndarray) -> np.ndarray:
        c = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 3)
        out = np.empty((c.shape[0], 4), np.float32)
        self._lib._call("photon_volume_sample", self.handle, c.shape[0], _ptr(c), _ptr(out))
        return out

    def trace_rays(self, pos: np.ndarray, direction: np.ndarray, algorithm: int = 2):
        p = np.array(pos, dtype=np.float32, order="C").reshape(-1, 3)
        d = np.array(direction, dtype=np.float32, order="C").reshape(-1, 3)
        steps = np.zeros(p.shape[0], np.int32)
        self._lib._call("photon_trace_volume_rays", self.handle, int(algorithm), p.shape[0], _ptr(p), _ptr(d), _ptr(steps))
        return p, d, steps

    def trace_rays_queued(self, pos: np.ndarray, direction: np.ndarray, algorithm: int = 2, segments: int = -1):
        """The march of trace_rays through the render path's launch (persistent waves, work queues, `segments` pieces)."""
        p = np.array(pos, dtype=np.float32, order="C").reshape(-1, 3)
        d = np.array(direction, dtype=np.float32, order="C").reshape(-1, 3)
        self._lib._call("photon_trace_volume_rays_queued", self.handle, int(algorithm), p.shape[0], _ptr(p), _ptr(d), int(segments))
        return p, d

    def free(self):
        if self.handle:
            self._lib.lib.photon_volume_free(self.handle)
            self.handle = None


class Sources:
    """Light-field sources generated in HBM (photon_sources_t)."""

    def __init__(self, lib: PhotonLibrary, handle):
        self._lib, self.handle = lib, handle

    def count(self) -> int:
        return int(self._lib.lib.photon_sources_count(self.handle))

    def download(self) -> dict:
        n = self.count()
        out = dict(x=np.empty(n, np.float32), y=np.empty(n, np.float32), z=np.empty(n, np.float32),
                   radiance=np.empty(n, np.float64), diameter_index=np.empty(n, np.int32))
        self._lib._call("photon_sources_download", self.handle, _ptr(out["x"]), _ptr(out["y"]), _ptr(out["z"]), _ptr(out["radiance"]),
                        _ptr(out["diameter_index"]))
        return out

    def free(self):
        if self.handle:
            self._lib.lib.photon_sources_free(self.handle)
            self.handle = None


class Flow:
    """A velocity field on a grid in HBM (photon_flow_t)."""

    def __init__(self, lib: PhotonLibrary, handle):
        self._lib, self.handle = lib, handle

    def free(self):
        if self.handle:
            self._lib.lib.photon_flow_free(self.handle)
            self.handle = None


class Scene:
    def __init__(self, lib: PhotonLibrary, handle, call: RayTracingCall):
        self._lib, self.handle, self.call = lib, handle, call
        self.num_sources = call.num_sources

    def trace(self, d_image_ptr: int, volume: Optional[Volume] = None, algorithm: int = 0, src_begin: int = 0,
              src_end: Optional[int] = None, stream: int = 0, want_stats: bool = False):
        """Accumulate into a DEVICE image (raw pointer, e.g. torch tensor .data_ptr())."""
        if src_end is None:
            src_end = self.num_sources
        stats = photon_trace_stats_t() if want_stats else None
        self._lib._call("photon_trace", self.handle, volume.handle if volume is not None else None, int(algorithm), int(src_begin), int(src_end),
                        _vp(d_image_ptr), _vp(stream), ctypes.byref(stats) if stats is not None else None)
        return stats

    def trace_moments(self, d_image_ptr: int, d_records_ptr: int, volume: Optional[Volume] = None, algorithm: int = 0,
                      src_begin: int = 0, src_end: Optional[int] = None, stream: int = 0):
        """trace() plus the per-source sensor moments (photon_trace_moments): the records of sources [src_begin, src_end) go
        to the DEVICE array f64[num_sources][8] at d_records_ptr; every other record is left as it is."""
        if src_end is None:
            src_end = self.num_sources
        self._lib._call("photon_trace_moments", self.handle, volume.handle if volume is not None else None, int(algorithm), int(src_begin),
                        int(src_end), _vp(d_image_ptr), _vp(d_records_ptr), _vp(stream))

    @property
    def has_stats_window(self) -> bool:
        return self._lib.has_stats_window

    def stats_begin(self, stream: int = 0):
        """Open a statistics window: traces without want_stats record their events and let the counters run."""
        self._lib._call("photon_scene_stats_begin", self.handle, _vp(stream))

    def stats_end(self, stream: int = 0):
        """Wait for the stream and return the window's sums (photon_trace_stats_t; .traces = calls covered)."""
        stats = photon_trace_stats_t()
        self._lib._call("photon_scene_stats_end", self.handle, _vp(stream), ctypes.byref(stats))
        return stats

    def check(self, stream: int = 0):
        """Wait for `stream`; raise if a trace of this scene had a hand-off error between march segments (photon_scene_check)."""
        self._lib._call("photon_scene_check", self.handle, _vp(stream))

    def set_march_segments(self, segments: int):
        """-1 the library's choice, 1 whole marches, n: cut every march of a large launch into n segments (speed only)."""
        self._lib._call("photon_scene_set_march_segments", self.handle, int(segments))

    def set_march_profile(self, on: bool):
        """Record wave entry / first-group / exit times of the march launches (measurement; off by default)."""
        self._lib._call("photon_scene_set_march_profile", self.handle, int(bool(on)))

    def march_profile(self) -> dict:
        """Means over the march launches since the statistics were last reset (see photon_march_profile_t)."""
        out = photon_march_profile_t()
        out.struct_size = ctypes.sizeof(photon_march_profile_t)
        self._lib._call("photon_scene_march_profile", self.handle, ctypes.byref(out))
        return out.as_dict()

    def set_noise(self, add_pos_noise=False, pos_noise_std=0.0, add_ngrad_noise=False, ngrad_noise_std=0.0, seed=0):
        self._lib._call("photon_scene_set_noise", self.handle, int(bool(add_pos_noise)), float(pos_noise_std), int(bool(add_ngrad_noise)),
                        float(ngrad_noise_std), int(seed))

    def set_ray_order(self, mode: int):
        """0 source-major (reference order), 1 lens-major over spatially sorted sources, 2 auto (default)."""
        self._lib._call("photon_scene_set_ray_order", self.handle, int(mode))

    def set_skip_doomed(self, on: bool):
        """Drop rays that provably die on the first element's aperture before the march (default on)."""
        self._lib._call("photon_scene_set_skip_doomed", self.handle, int(bool(on)))

    def live_rays(self) -> int:
        """Lens samples per source a volume-free launch keeps (photon_scene_live_rays); rays_per_source = nothing ruled out."""
        return int(self._lib.lib.photon_scene_live_rays(self.handle))

    def live_sources(self):
        """The sources a volume-free launch keeps, ascending (photon_scene_live_sources); None = every source."""
        f = self._lib.lib.photon_scene_live_sources
        n = f(self.handle, None, 0)
        if n == -1:
            return None
        if n < 0:
            raise PhotonError(f"photon_scene_live_sources returned {n}")
        out = np.empty(int(n), np.int32)
        got = f(self.handle, _ptr(out), int(n))
        if got != n:
            raise PhotonError(f"photon_scene_live_sources returned {got}, expected {n}")
        return out

    def live_samples(self):
        """The lens samples a volume-free launch keeps, ascending (photon_scene_live_samples)."""
        n = self.live_rays()
        out = np.zeros(max(n, 1), np.int32)
        got = int(self._lib.lib.photon_scene_live_samples(self.handle, _ptr(out), int(out.size)))
        if got != n:
            raise PhotonError(f"photon_scene_live_samples returned {got}, expected {n}")
        return out[:n]

    def set_source_base(self, first_source: int):
        """This scene holds the slice of a job's sources that starts at `first_source` (noise ids stay job-wide)."""
        self._lib._call("photon_scene_set_source_base", self.handle, int(first_source))

    def set_element_train(self, mode: int):
        """0 = the reference's element walk (element 0 only), 1 = the working multi-element train."""
        self._lib._call("photon_scene_set_element_train", self.handle, int(mode))

    def free(self):
        if self.handle:
            self._lib.lib.photon_scene_free(self.handle)
            self.handle = None
