"""raytracercore_amd -- MI355X (gfx950) path-tracing core behind RaytracerCore's render seam.

The product is ``librtcore_hip.so`` (HIP kernels + the C ABI of ``include/rtcore.h``).  This
module is the Python host mirror used by the tests and the benchmark: ctypes structs that
match the ABI, a ``SceneLoader`` over ``rt_parse_scene`` (SceneLoader.FromFile,
RaytracerCore/SceneLoader.cs:112-440) and a ``GpuRaytracer`` that owns one device scene and
renders tile passes with the semantics of ``Raytracer.Render`` (Raytracer.cs:294-330).

There is no CPU fallback: if the shared library is missing or no HIP device is present the
calls raise ``RtError``.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librtcore_hip.so")
REPO_ROOT = os.path.dirname(_HERE)

RT_OK = 0
ABI_VERSION = 6  # RTCORE_ABI_VERSION of include/rtcore.h
RT_PRIM_TRIANGLE, RT_PRIM_SPHERE, RT_PRIM_PLANE = 0, 1, 2
RT_FLAG_MIRROR, RT_FLAG_TWOSIDED, RT_FLAG_INVERT, RT_FLAG_HASNORMALS, RT_FLAG_TRANSFORMED = 1, 2, 4, 8, 16
RT_CAMERA_FRUSTUM, RT_CAMERA_ORTHO = 0, 1
RT_TRAVERSAL_AUTO, RT_TRAVERSAL_BRUTE, RT_TRAVERSAL_BVH, RT_TRAVERSAL_BVH2, RT_TRAVERSAL_GROUPED = 0, 1, 2, 3, 4
RT_BVH_BUILDER_AUTO, RT_BVH_BUILDER_HOST, RT_BVH_BUILDER_GPU = 0, 1, 2
# rt_bounce_type = Raytracer.BounceType (Raytracer.cs:14-26)
(RT_BOUNCE_SKIPPED, RT_BOUNCE_DIFFUSE, RT_BOUNCE_SPECULAR, RT_BOUNCE_SPECULAR_FAIL, RT_BOUNCE_TRANSMITTED,
 RT_BOUNCE_EMISSION, RT_BOUNCE_PURE_BLACK, RT_BOUNCE_RECURSION_COMPLETE, RT_BOUNCE_MISSED, RT_BOUNCE_DEBUG) = range(10)
BOUNCE_TYPE_NAMES = ("Skipped", "Diffuse", "Specular", "SpecularFail", "Transmitted", "Emission", "PureBlack",
                     "RecursionComplete", "Missed", "Debug")
RT_TRACE_MAX_RECORDS = 1 << 20  # records of one rt_trace_paths call
# rt_gather_mode (rt_render_surfels): the reference's diffuse bounce, Lambert's cosine, the uniform sphere
RT_GATHER_DIFFUSE, RT_GATHER_COSINE, RT_GATHER_SPHERE = 0, 1, 2
RT_LIST_RAYS, RT_LIST_BEAMS, RT_LIST_SURFELS = 0, 1, 2  # rt_list_kind (rt_render_list)


class rt_query_mode(enum.IntEnum):
    """Mode of rt_query_rays (include/rtcore.h)."""
    RT_QUERY_FAST = 0   # the path kernels' fp32 closest hit, in the scene's traversal mode
    RT_QUERY_EXACT = 1  # the fp64 reference query of rt_primary_ids


RT_QUERY_FAST, RT_QUERY_EXACT = int(rt_query_mode.RT_QUERY_FAST), int(rt_query_mode.RT_QUERY_EXACT)
RT_SELECT_PRIM, RT_SELECT_NODE = 0, 1  # rt_select_kind: a primitive ID / a reference-BVH node in pre-order
RT_SELECT_MAX_TESTS = 1 << 32  # item tests (pixels or rays x items) of one selection call
BUILD_STAT_NAMES = ("prepare_ms", "bvh_ms", "upload_ms", "gpu_build_ms", "ploc_rounds", "wide_nodes", "stack_need",
                    "flat_rects", "flat_boxes", "flat_frames", "flat_frame_boxes", "flat_frame_rects", "flat_tris",
                    "flat_spheres", "hot_nodes", "jit_status", "jit_compile_ms", "jit_cached", "group_max",
                    "wide_leaves", "compact_leaves", "outer_prims")


def set_jit(on: bool) -> None:
    """rt_set_jit: scene-specialised brute-force kernels (hiprtc) on or off, process-wide."""
    _check(load_library().rt_set_jit(1 if on else 0))


def jit_compile_check(arch: str = "gfx950", grouped: bool = False) -> int:
    """rt_debug_jit_compile (host only): code-object bytes of a scene-specialised build of the
    embedded kernel sources for `arch`; raises RtError with the compiler log on failure."""
    buf = C.create_string_buffer(8192)
    n = load_library().rt_debug_jit_compile(arch.encode(), 1 if grouped else 0, buf, len(buf))
    if n < 0:
        raise RtError(f"scene-specialised build failed: {buf.value.decode(errors='replace')}")
    return n


class RtError(RuntimeError):
    """A negative rt_status from the library (message from rt_last_error)."""


class rt_vec4d(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("w", C.c_double)]


class rt_color(C.Structure):
    _fields_ = [("r", C.c_double), ("g", C.c_double), ("b", C.c_double)]


class rt_prim(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("flags", C.c_int32),
        ("p", rt_vec4d * 3), ("n", rt_vec4d * 3),
        ("radius", C.c_double),
        ("to_obj", C.c_double * 16), ("to_world", C.c_double * 16), ("to_normal", C.c_double * 16),
        ("emission", rt_color), ("diffuse", rt_color), ("specular", rt_color), ("refraction", rt_color),
        ("shininess", C.c_double), ("refractive_index", C.c_double),
    ]


class rt_camera(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("reserved", C.c_int32),
        ("position", rt_vec4d), ("look_at", rt_vec4d), ("up", rt_vec4d),
        ("fov_y", C.c_double), ("size_mult", C.c_double),
        ("image_plane", C.c_double), ("dof_amount", C.c_double), ("focal_length", C.c_double),
    ]


class rt_scene_params(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("recursion", C.c_int32), ("debug_geom", C.c_int32),
        ("air_ior", C.c_double), ("ambient", rt_color),
    ]


class rt_scene_info(C.Structure):
    _fields_ = [
        ("n_prims", C.c_int32), ("ref_bvh_nodes", C.c_int32), ("ref_bvh_depth", C.c_int32),
        ("sah_bvh_nodes", C.c_int32), ("sah_bvh_depth", C.c_int32), ("traversal", C.c_int32),
        ("device", C.c_int32), ("bvh_builder", C.c_int32), ("device_bytes", C.c_uint64),
    ]


class rt_debug_ray(C.Structure):
    """One bounce of rt_trace_paths (Raytracer.DebugRay + its Hit): 96 B, offsets in include/rtcore.h."""
    _fields_ = [
        ("prim_id", C.c_int32), ("type", C.c_int32), ("inside", C.c_int32), ("distance", C.c_float),
        ("fresnel", C.c_float), ("cos_in", C.c_float), ("bounce", C.c_int32), ("reserved0", C.c_int32),
        ("position", C.c_float * 3), ("normal", C.c_float * 3), ("origin", C.c_float * 3),
        ("direction", C.c_float * 3), ("tint", C.c_float * 3), ("reserved1", C.c_int32),
    ]


# the same record as a numpy structured dtype (the element type of GpuRaytracer.trace_paths' records)
DEBUG_RAY_DTYPE = np.dtype([
    ("prim_id", np.int32), ("type", np.int32), ("inside", np.int32), ("distance", np.float32),
    ("fresnel", np.float32), ("cos_in", np.float32), ("bounce", np.int32), ("reserved0", np.int32),
    ("position", np.float32, (3,)), ("normal", np.float32, (3,)), ("origin", np.float32, (3,)),
    ("direction", np.float32, (3,)), ("tint", np.float32, (3,)), ("reserved1", np.int32),
])


class rt_ray(C.Structure):
    """Ray (Vectors/Ray.cs): origin (w = 1) and unit direction (w = 0), 64 B."""
    _fields_ = [("origin", rt_vec4d), ("direction", rt_vec4d)]


class rt_beam(C.Structure):
    """A ray and its first-order footprint (rt_render_beams): 192 B, twelve 16-byte rows."""
    _fields_ = [("origin", rt_vec4d), ("direction", rt_vec4d), ("origin_du", rt_vec4d), ("origin_dv", rt_vec4d),
                ("direction_du", rt_vec4d), ("direction_dv", rt_vec4d)]


class rt_surfel(C.Structure):
    """A surface point and its normal (rt_render_surfels): 64 B, four 16-byte rows."""
    _fields_ = [("position", rt_vec4d), ("normal", rt_vec4d)]


class rt_probe_sh(C.Structure):
    """288 B: nine rows l = 0 .. 8 of four doubles (the r, g, b sums and the misses' projection)."""
    _fields_ = [("c", (C.c_double * 4) * 9)]


class rt_probe_moments(C.Structure):
    """64 B: the second moments of a probe's band-0/1 luminance coefficients, rows l = 0 .. 3 of (the hits' sum
    of (y Y_l)^2, the primary misses' sum of Y_l^2) (rt_render_probe_list_device)."""
    _fields_ = [("m", (C.c_double * 2) * 4)]


class rt_probe_select_params(C.Structure):
    """The selection rule of adaptive light probes (rt_probe_select_device), 48 B."""
    _fields_ = [("rel_tol", C.c_double), ("irr_floor", C.c_double), ("ambient", rt_color), ("min_samples", C.c_uint32),
                ("max_samples", C.c_uint32)]


RT_PROBE_GRID_VISIBILITY = 1  # rt_probe_grid.flags: leave out the probes the point cannot see


class rt_probe_grid(C.Structure):
    """A regular grid of light probes (rt_shade_probes): 80 B, five 16-byte rows; probe (ix, iy, iz) has index
    (iz * ny + iy) * nx + ix and the position origin + (ix, iy, iz) * step."""
    _fields_ = [("origin", C.c_double * 3), ("step", C.c_double * 3), ("dims", C.c_int32 * 3), ("flags", C.c_uint32),
                ("bias", C.c_double), ("reserved", C.c_uint32 * 2)]


def probe_grid(origin, step, dims, visibility: bool = True, bias: float = 0.0) -> rt_probe_grid:
    """rt_probe_grid from three floats each for origin and step and three ints for dims; the library checks
    the values."""
    return rt_probe_grid((C.c_double * 3)(*[float(v) for v in origin]), (C.c_double * 3)(*[float(v) for v in step]),
                         (C.c_int32 * 3)(*[int(v) for v in dims]), RT_PROBE_GRID_VISIBILITY if visibility else 0,
                         float(bias))


RT_PROBE_DEPTH_WRAP = 1  # rt_probe_depth_params.flags: the shading multiplies by the backface wrap weight


class rt_probe_depth_params(C.Structure):
    """The parameters of probe depth maps (rt_render_probe_depth_device, rt_shade_probes_depth_device), 32 B."""
    _fields_ = [("d_max", C.c_double), ("var_floor", C.c_double), ("sharpness", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


def probe_depth_params(d_max: float, sharpness: int = 5, var_floor: float = 1e-4, wrap: bool = False) -> rt_probe_depth_params:
    """rt_probe_depth_params; the library checks the values."""
    return rt_probe_depth_params(float(d_max), float(var_floor), int(sharpness), RT_PROBE_DEPTH_WRAP if wrap else 0)


RT_PROBE_INSIDE = 1  # probe state: inside geometry; absent in the placed shading
RT_PROBE_IDLE = 2  # probe state: no front face within the cell's diagonal
RT_PROBE_RELOCATE_CLASSIFY_ONLY = 1  # rt_probe_relocate_params.flags: offsets are read, never written


class rt_probe_relocate_params(C.Structure):
    """The parameters of probe relocation (rt_relocate_probes_device), 32 B."""
    _fields_ = [("back_share", C.c_double), ("min_front", C.c_double), ("max_offset", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


def probe_relocate_params(min_front: float, back_share: float = 0.25, max_offset: float = 0.45,
                          classify_only: bool = False) -> rt_probe_relocate_params:
    """rt_probe_relocate_params (DDGI's defaults for the two shares); the library checks the values."""
    return rt_probe_relocate_params(float(back_share), float(min_front), float(max_offset),
                                    RT_PROBE_RELOCATE_CLASSIFY_ONLY if classify_only else 0, 0)


# rt_probe_relocation, 64 B per probe
RELOCATION_DTYPE = np.dtype([("state", "<u4"), ("moved", "<u4"), ("front", "<u4"), ("back", "<u4"), ("misses", "<u4"),
                             ("skipped", "<u4"), ("k_near", "<i4"), ("k_back", "<i4"), ("k_far", "<i4"), ("reserved", "<i4"),
                             ("d_near", "<f8"), ("d_back", "<f8"), ("d_far", "<f8")])
assert RELOCATION_DTYPE.itemsize == 64


class rt_obscurance_params(C.Structure):
    """The parameters of obscurance at surfels (rt_obscurance_surfels_device), 24 B."""
    _fields_ = [("radius", C.c_double), ("power", C.c_int32), ("reserved", C.c_uint32 * 3)]


class rt_obscurance(C.Structure):
    """One entry's obscurance accumulators (OBSCURANCE_DTYPE), 48 B."""
    _fields_ = [("o", C.c_double), ("o2", C.c_double), ("bent", C.c_double * 3), ("samples", C.c_uint32),
                ("hits", C.c_uint32)]


class rt_obscurance_select_params(C.Structure):
    """The stopping rule of adaptive obscurance (rt_obscurance_select_device), 16 B."""
    _fields_ = [("tol", C.c_double), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32)]


def obscurance_params(radius: float, power: int = 1) -> rt_obscurance_params:
    """rt_obscurance_params; the library checks the values."""
    return rt_obscurance_params(float(radius), int(power))


def obscurance_select_params(tol: float, min_samples: int, max_samples: int) -> rt_obscurance_select_params:
    """rt_obscurance_select_params; the library checks the values."""
    return rt_obscurance_select_params(float(tol), int(min_samples), int(max_samples))


class rt_hit(C.Structure):
    """One answer of rt_query_rays (Hit.cs): 48 B, offsets in include/rtcore.h."""
    _fields_ = [
        ("prim_id", C.c_int32), ("inside", C.c_int32), ("distance", C.c_double),
        ("position", C.c_float * 3), ("normal", C.c_float * 3), ("reserved", C.c_int32 * 2),
    ]


class rt_select_item(C.Structure):
    """One item of a selection list: (rt_select_kind, Primitive.ID or reference-BVH node index), 8 B."""
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


class rt_selection(C.Structure):
    """One answer of the selection pass: the winner's index in the caller's list (-1: none), 0, its distance; 16 B."""
    _fields_ = [("item", C.c_int32), ("reserved", C.c_int32), ("distance", C.c_double)]


class rt_adaptive_params(C.Structure):
    """The selection rule of adaptive sampling (rt_adaptive_select_device), 32 B."""
    _fields_ = [("rel_tol", C.c_double), ("lum_floor", C.c_double), ("min_samples", C.c_uint32),
                ("max_samples", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RT_DENOISE_SAME_PRIM = 1  # rt_denoise_params.flags: a tap of another prim_id weighs 0


class rt_denoise_params(C.Structure):
    """The a-trous filter's parameters (rt_denoise_device), 32 B."""
    _fields_ = [("sigma_l", C.c_float), ("sigma_z", C.c_float), ("lum_eps", C.c_float), ("normal_pow_log2", C.c_int32),
                ("iterations", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# what GpuRaytracer.denoise uses where the caller names no value (sigma_l counts standard
# deviations of a pixel mean that adaptive sampling left as large as rel_tol of the luminance, so it is small)
DENOISE_DEFAULTS = dict(sigma_l=1.5, sigma_z=0.05, lum_eps=1e-4, normal_pow_log2=6, iterations=5, flags=0)


def denoise_iterations(width: int, height: int) -> int:
    """The levels GpuRaytracer.denoise runs where the caller names none: the filter's reach, 2 (2^k - 1) pixels
    each way after k levels, held to about a twentieth of the frame's shorter side -- 5 from 1024 pixels up,
    one fewer per halving, at least 1."""
    return max(1, min(5, int(min(width, height)).bit_length() - 6))


def denoise_params(**kw) -> rt_denoise_params:
    """rt_denoise_params from keywords, DENOISE_DEFAULTS for the rest."""
    v = dict(DENOISE_DEFAULTS)
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"unknown denoise parameter(s): {sorted(unknown)}")
    v.update(kw)
    return rt_denoise_params(float(v["sigma_l"]), float(v["sigma_z"]), float(v["lum_eps"]), int(v["normal_pow_log2"]),
                             int(v["iterations"]), int(v["flags"]))


RT_REPROJECT_SAME_PRIM = 1  # rt_reproject_params.flags: the source pixel must show the same prim_id


class rt_reproject_params(C.Structure):
    """The temporal reprojection's parameters (rt_reproject_device), 32 B."""
    _fields_ = [("sigma_z", C.c_float), ("normal_cos_min", C.c_float), ("max_history", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


# what GpuRaytracer.reproject uses where the caller names no value (profiles/reproject/README.md)
REPROJECT_DEFAULTS = dict(sigma_z=0.05, normal_cos_min=0.9, max_history=32, flags=RT_REPROJECT_SAME_PRIM)


def reproject_params(**kw) -> rt_reproject_params:
    """rt_reproject_params from keywords, REPROJECT_DEFAULTS for the rest."""
    v = dict(REPROJECT_DEFAULTS)
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"unknown reproject parameter(s): {sorted(unknown)}")
    v.update(kw)
    return rt_reproject_params(float(v["sigma_z"]), float(v["normal_cos_min"]), int(v["max_history"]), int(v["flags"]))


SELECT_ITEM_DTYPE = np.dtype([("kind", np.int32), ("index", np.int32)])
SELECTION_DTYPE = np.dtype([("item", np.int32), ("reserved", np.int32), ("distance", np.float64)])

# the same records as numpy structured dtypes (GpuRaytracer.query_rays, camera_rays)
RAY_DTYPE = np.dtype([("origin", np.float64, (4,)), ("direction", np.float64, (4,))])
BEAM_DTYPE = np.dtype([(f, np.float64, (4,)) for f in
                       ("origin", "direction", "origin_du", "origin_dv", "direction_du", "direction_dv")])
SURFEL_DTYPE = np.dtype([("position", np.float64, (4,)), ("normal", np.float64, (4,))])
PROBE_MOMENTS_DTYPE = np.dtype([("m", np.float64, (4, 2))])  # rt_probe_moments
OBSCURANCE_DTYPE = np.dtype([("o", np.float64), ("o2", np.float64), ("bent", np.float64, (3,)), ("samples", np.uint32),
                             ("hits", np.uint32)])  # rt_obscurance
HIT_DTYPE = np.dtype([
    ("prim_id", np.int32), ("inside", np.int32), ("distance", np.float64),
    ("position", np.float32, (3,)), ("normal", np.float32, (3,)), ("reserved", np.int32, (2,)),
])

# entry points added under an unchanged ABI version: bound when the library has them (an older build
# named by RTCORE_LIB may not)
_OPTIONAL = ("rt_query_rays", "rt_query_rays_device", "rt_camera_rays", "rt_select_pixels", "rt_select_pixels_device",
             "rt_select_rays", "rt_select_rays_device", "rt_render_rays", "rt_render_rays_device",
             "rt_occluded_rays", "rt_occluded_rays_device", "rt_render_pixels", "rt_render_pixels_device",
             "rt_adaptive_select_device", "rt_primary_hits_device", "rt_denoise_device", "rt_reproject_device",
             "rt_render_beams", "rt_render_beams_device", "rt_camera_beams",
             "rt_render_surfels", "rt_render_surfels_device", "rt_render_list", "rt_render_list_device",
             "rt_occluded_surfels", "rt_occluded_surfels_device", "rt_render_probes", "rt_render_probes_device",
             "rt_probe_radiance_device", "rt_shade_probes", "rt_shade_probes_device", "rt_render_probe_list_device",
             "rt_probe_select_device", "rt_render_probe_depth_device", "rt_probe_depth_close_device",
             "rt_shade_probes_depth_device", "rt_obscurance_surfels_device", "rt_obscurance_select_device",
             "rt_debug_launch_overlap", "rt_debug_kernel_times_raw", "rt_probe_positions_device",
             "rt_relocate_probes_device", "rt_shade_probes_placed", "rt_shade_probes_placed_device",
             "rt_shade_probes_depth_placed_device")

_lib: Optional[C.CDLL] = None


def load_library(path: str = "") -> C.CDLL:
    """Load librtcore_hip.so (built by __graft_entry__.build()).  Raises if it is missing.

    RTCORE_LIB may name an alternative build of the same library (e.g. a tuning variant).
    """
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("RTCORE_LIB", "") or LIB_PATH
    if not os.path.exists(path):
        raise RtError(f"{path} is missing: run __graft_entry__.build() (make -C raytracercore_amd/csrc)")
    # torch-ROCm wheels carry their own HIP runtime; when torch is present it must be loaded
    # first so that this library binds to the same runtime instance (one HIP runtime per process)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    P = C.POINTER
    sig = {
        "rt_abi_version": (C.c_int, []),
        "rt_build_info": (C.c_char_p, []),
        "rt_device_count": (C.c_int, []),
        "rt_last_error": (C.c_int, [C.c_char_p, C.c_int32]),
        "rt_scene_create": (C.c_int, [P(rt_scene_params), P(rt_prim), C.c_int32, C.c_int32, P(C.c_void_p)]),
        "rt_scene_set_camera": (C.c_int, [C.c_void_p, P(rt_camera)]),
        "rt_scene_set_traversal": (C.c_int, [C.c_void_p, C.c_int32]),
        "rt_scene_get_info": (C.c_int, [C.c_void_p, P(rt_scene_info)]),
        "rt_scene_destroy": (None, [C.c_void_p]),
        "rt_set_bvh_builder": (C.c_int, [C.c_int32]),
        "rt_scene_get_build_stats": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int32]),
        "rt_scene_check_bvh": (C.c_int, [C.c_void_p]),
        "rt_set_jit": (C.c_int, [C.c_int32]),
        "rt_scene_get_jit_error": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
        "rt_debug_jit_compile": (C.c_int, [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32]),
        "rt_debug_jit_header": (C.c_int, [P(rt_scene_params), P(rt_prim), C.c_int32, P(rt_camera), C.c_int32,
                                          C.c_char_p, C.c_int64]),
        "rt_render_tile": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_uint64, C.c_uint64,
                                     P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_tile_1spp": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_uint64, C.c_uint64, P(rt_color)]),
        "rt_trace_paths": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_uint64, C.c_uint64, P(rt_debug_ray),
                                     P(C.c_int32), P(rt_color)]),
        "rt_primary_ids": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [P(C.c_int32)]),
        "rt_bvh_counts": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [P(C.c_int32)]),
        "rt_render_device": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_uint64, C.c_uint64] +
                             [C.c_void_p] * 4 + [C.c_void_p]),
        "rt_primary_ids_device": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
        "rt_last_kernel_ms": (C.c_int, [C.c_void_p, P(C.c_float)]),
        "rt_kernel_times": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float)]),
        "rt_scene_set_stats": (C.c_int, [C.c_void_p, C.c_int32]),
        "rt_scene_get_stats": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_int32]),
        "rt_render_frame_multi": (C.c_int, [P(rt_scene_params), P(rt_prim), C.c_int32, P(rt_camera), C.c_int32,
                                            C.c_int32, C.c_uint64, C.c_uint64, P(rt_color), P(C.c_uint32),
                                            P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_bands": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_uint64, C.c_uint64, P(rt_color),
                                      P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_bands_device": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_uint64, C.c_uint64] +
                                   [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_void_p]),
        "rt_band_rows": (C.c_int, [C.c_int32] * 4),
        "rt_band_slot_rows": (C.c_int, [C.c_int32] * 3),
        "rt_scatter_band_slot": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_int32] * 5 + [P(rt_color), P(C.c_uint32),
                                                                                       P(C.c_uint32)]),
        "rt_frame_create": (C.c_int, [P(rt_scene_params), P(rt_prim), C.c_int32, P(rt_camera), C.c_int32,
                                      P(C.c_void_p)]),
        "rt_frame_set_camera": (C.c_int, [C.c_void_p, P(rt_camera)]),
        "rt_frame_render": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, P(rt_color), P(C.c_uint32),
                                      P(C.c_uint32), P(C.c_uint64)]),
        "rt_frame_submit": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64]),
        "rt_frame_collect": (C.c_int, [C.c_void_p, P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_frame_inject_fault": (C.c_int, [C.c_void_p, C.c_int32]),
        "rt_frame_destroy": (None, [C.c_void_p]),
        "rt_parse_scene": (C.c_int, [C.c_char_p, P(rt_scene_params), P(rt_prim), P(C.c_int32), P(rt_camera),
                                     P(C.c_int32)]),
        "rt_sample_output": (C.c_int32, [rt_color, C.c_uint32, C.c_uint32, rt_color, C.c_double, C.c_double]),
        "rt_tonemap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, rt_color, C.c_double,
                                        C.c_double, C.c_void_p, C.c_void_p]),
        "rt_ref_bvh_export": (C.c_int, [P(rt_prim), C.c_int32, P(C.c_int32), P(C.c_double), P(C.c_int32),
                                        P(C.c_int32)]),
        "rt_debug_item_order": (C.c_int, [C.c_int32] * 8 + [P(C.c_uint32), C.c_int64, P(C.c_int32)]),
        "rt_debug_scene_bound": (C.c_int, [P(rt_prim), C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float)]),
        "rt_debug_block_cull": (C.c_int, [P(rt_prim), C.c_int32, P(rt_camera)] + [C.c_int32] * 9 +
                                [P(C.c_uint8), C.c_int64, P(C.c_int32)]),
        "rt_debug_block_units": (C.c_int, [P(rt_prim), C.c_int32, P(rt_camera)] + [C.c_int32] * 9 +
                                 [P(C.c_int32), P(C.c_int32), C.c_int64, P(C.c_float), P(C.c_uint8), P(C.c_uint64),
                                  C.c_int64, P(C.c_int32)]),
        "rt_debug_start_rows": (C.c_int, [C.c_int32, P(rt_camera)] + [C.c_int32] * 6 + [P(C.c_int64)]),
        "rt_debug_launch_overlap": (C.c_int, [C.c_int32, C.c_uint64, C.c_int32, P(C.c_int32)]),
        "rt_debug_kernel_times_raw": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float)]),
        "rt_debug_ray_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
        "rt_debug_vn_rehit": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double), C.c_int32, C.c_double,
                                        C.c_double, P(C.c_float), P(C.c_int32), P(C.c_double), P(C.c_double)]),
        "rt_debug_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, P(C.c_float)]),
        "rt_query_rays": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_query_rays_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
        "rt_camera_rays": (C.c_int, [P(rt_camera)] + [C.c_int32] * 6 + [C.c_void_p]),
        "rt_select_pixels": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p]),
        "rt_select_pixels_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
        "rt_select_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_select_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p]),
        "rt_debug_select_rays": (C.c_int, [P(rt_prim), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                           C.c_void_p]),
        "rt_render_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                     P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                            C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p]),
        "rt_render_beams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                      P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_beams_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                             C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p]),
        "rt_debug_beam_rays": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_void_p]),
        "rt_camera_beams": (C.c_int, [P(rt_camera)] + [C.c_int32] * 6 + [C.c_void_p]),
        "rt_render_surfels": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                        C.c_uint64, P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_surfels_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64,
                                               C.c_uint64, C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p]),
        "rt_debug_surfel_rays_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                                  C.c_uint64, C.c_void_p, C.c_void_p]),
        "rt_render_probes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                       P(rt_probe_sh), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_probes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                              C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p]),
        "rt_debug_sh_basis": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_debug_probe_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(rt_probe_sh),
                                          P(C.c_uint32), P(C.c_uint32)]),
        "rt_render_probe_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                                  C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6),
        "rt_debug_probe_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
        "rt_probe_select_device": (C.c_int, [P(rt_probe_select_params)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_void_p]),
        "rt_debug_probe_select": (C.c_int64, [P(rt_probe_select_params)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p,
                                              C.c_uint32]),
        "rt_debug_probe_error": (C.c_int, [P(rt_probe_select_params)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p,
                                           C.c_void_p]),
        "rt_probe_radiance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, rt_color, C.c_void_p,
                                               C.c_void_p]),
        "rt_debug_probe_radiance": (C.c_int, [P(rt_probe_sh), P(C.c_uint32), P(C.c_uint32), C.c_int64, rt_color,
                                              P(C.c_double)]),
        "rt_shade_probes_device": (C.c_int, [C.c_void_p, P(rt_probe_grid), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
        "rt_shade_probes": (C.c_int, [C.c_void_p, P(rt_probe_grid), P(C.c_double), C.c_void_p, C.c_int64, P(rt_color),
                                      P(C.c_double)]),
        "rt_debug_probe_segments_device": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
        "rt_debug_probe_segments": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_int64, C.c_void_p, P(C.c_double)]),
        "rt_debug_shade_probes": (C.c_int, [P(rt_probe_grid), P(C.c_double), C.c_void_p, C.c_int64, C.c_void_p,
                                            P(rt_color), P(C.c_double)]),
        "rt_render_probe_depth_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                                   C.c_uint64, P(rt_probe_depth_params), C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_probe_depth_fold": (C.c_int, [P(rt_probe_depth_params), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                                C.c_void_p, C.c_void_p]),
        "rt_probe_depth_close_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
        "rt_debug_probe_depth_close": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_shade_probes_depth_device": (C.c_int, [P(rt_probe_grid), P(rt_probe_depth_params), C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_shade_probes_depth": (C.c_int, [P(rt_probe_grid), P(rt_probe_depth_params), C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
        "rt_probe_positions_device": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_probe_positions": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_void_p]),
        "rt_relocate_probes_device": (C.c_int, [C.c_void_p, P(rt_probe_grid), P(rt_probe_relocate_params), C.c_int32, C.c_uint64,
                                                C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_probe_relocate": (C.c_int, [P(rt_probe_grid), P(rt_probe_relocate_params), C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p]),
        "rt_shade_probes_placed_device": (C.c_int, [C.c_void_p, P(rt_probe_grid)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]),
        "rt_shade_probes_placed": (C.c_int, [C.c_void_p, P(rt_probe_grid)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p,
                                             C.c_void_p]),
        "rt_debug_probe_segments_placed_device": (C.c_int, [P(rt_probe_grid)] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p,
                                                            C.c_void_p, C.c_void_p]),
        "rt_debug_probe_segments_placed": (C.c_int, [P(rt_probe_grid)] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p]),
        "rt_debug_shade_probes_placed": (C.c_int, [P(rt_probe_grid)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
        "rt_shade_probes_depth_placed_device": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_void_p, P(rt_probe_depth_params)] +
                                                [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_shade_probes_depth_placed": (C.c_int, [P(rt_probe_grid), C.c_void_p, C.c_void_p, P(rt_probe_depth_params)] +
                                               [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p]),
        "rt_obscurance_surfels_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                   P(rt_obscurance_params), C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                                   C.c_void_p, C.c_void_p]),
        "rt_debug_obscurance_fold": (C.c_int, [P(rt_obscurance_params), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                               C.c_void_p]),
        "rt_obscurance_select_device": (C.c_int, [P(rt_obscurance_select_params), C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_uint32, C.c_void_p, C.c_void_p]),
        "rt_debug_obscurance_select": (C.c_int64, [P(rt_obscurance_select_params), C.c_void_p, C.c_int64, C.c_void_p,
                                                   C.c_uint32]),
        "rt_debug_obscurance_error": (C.c_int, [P(rt_obscurance_select_params), C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p]),
        "rt_debug_oct_texel_dirs": (C.c_int, [C.c_void_p]),
        "rt_debug_oct_texel": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_render_list": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, P(rt_color), P(C.c_uint32),
                                     P(C.c_uint32), P(C.c_double), P(C.c_uint32), P(C.c_uint64)]),
        "rt_render_list_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5 +
                                  [C.c_uint64, C.c_void_p, C.c_void_p]),
        "rt_occluded_rays": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        "rt_occluded_rays_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p]),
        "rt_occluded_surfels": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_uint64,
                                          C.c_uint64, C.c_uint64, P(C.c_uint32), P(C.c_uint32)]),
        "rt_occluded_surfels_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                 C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
        "rt_render_pixels":(C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                       P(rt_color), P(C.c_uint32), P(C.c_uint32), P(C.c_double), P(C.c_uint32),
                                       P(C.c_uint64)]),
        "rt_render_pixels_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64] +
                                    [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_void_p]),
        "rt_adaptive_select_device": (C.c_int, [P(rt_adaptive_params)] + [C.c_void_p] * 5 + [C.c_uint64, C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "rt_debug_adaptive_select": (C.c_int64, [P(rt_adaptive_params)] + [C.c_void_p] * 5 + [C.c_uint64, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_uint32]),
        "rt_debug_pixels_plan": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, P(C.c_int32)]),
        "rt_primary_hits_device": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
        "rt_denoise_device": (C.c_int, [P(rt_denoise_params)] + [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_debug_denoise": (C.c_int, [P(rt_denoise_params)] + [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p]),
        "rt_reproject_device": (C.c_int, [P(rt_reproject_params), P(rt_camera)] + [C.c_void_p] * 7 +
                                [C.c_uint64, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
        "rt_debug_reproject": (C.c_int, [P(rt_reproject_params), P(rt_camera)] + [C.c_void_p] * 7 +
                               [C.c_uint64, C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    }
    for name, (res, args) in sig.items():
        if (name.startswith("rt_debug_") or name in _OPTIONAL) and not hasattr(lib, name):
            continue  # an older build (RTCORE_LIB, A/B measurements) without a newer debug entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.rt_abi_version() != ABI_VERSION:
        raise RtError(f"{path}: ABI version {lib.rt_abi_version()}, this module binds {ABI_VERSION} (rebuild)")
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != RT_OK:
        buf = C.create_string_buffer(1024)
        _lib.rt_last_error(buf, 1024)
        raise RtError(f"rtcore error {rc}: {buf.value.decode(errors='replace')}")


@dataclass
class ParsedScene:
    """SceneLoader.FromFile output in ABI form (Scene.cs fields + Primitives + Cameras)."""
    params: rt_scene_params
    prims: "C.Array[rt_prim]"
    cameras: "C.Array[rt_camera]"

    @property
    def n_prims(self) -> int:
        return len(self.prims)


class SceneLoader:
    """Mirror of RaytracerCore.SceneLoader (SceneLoader.cs:28-440) over rt_parse_scene."""

    @staticmethod
    def from_text(text: str) -> ParsedScene:
        lib = load_library()
        n_p, n_c = C.c_int32(0), C.c_int32(0)
        params = rt_scene_params()
        _check(lib.rt_parse_scene(text.encode(), C.byref(params), None, C.byref(n_p), None, C.byref(n_c)))
        prims = (rt_prim * max(1, n_p.value))()
        cams = (rt_camera * max(1, n_c.value))()
        _check(lib.rt_parse_scene(text.encode(), C.byref(params), prims, C.byref(n_p), cams, C.byref(n_c)))
        return ParsedScene(params, (rt_prim * n_p.value).from_buffer(prims), (rt_camera * n_c.value).from_buffer(cams))

    @staticmethod
    def from_file(path: str) -> ParsedScene:
        with open(path, "r", encoding="utf-8") as f:
            return SceneLoader.from_text(f.read())


LAYOUT_NAMES = ("rects", "boxes", "frames", "frame_boxes", "frame_rects", "tris", "spheres", "planes",
                "groups", "grouped_slots")


def jit_header(scene: "SceneLoader", camera: int = 0, size: Optional[Tuple[int, int]] = None,
               grouped: bool = False) -> str:
    """rt_debug_jit_header (host code, no GPU): the generated header of the scene-specialised build
    for this scene and camera (tools/jit_isa.py compiles it and writes the listing)."""
    lib = load_library()
    params = rt_scene_params.from_buffer_copy(scene.params)
    if size:
        params.width, params.height = size
    n = len(scene.prims)
    arr = (rt_prim * max(1, n))(*scene.prims)
    cam = rt_camera.from_buffer_copy(scene.cameras[camera])
    k = lib.rt_debug_jit_header(C.byref(params), arr, n, C.byref(cam), 1 if grouped else 0, None, 0)
    if k < 0:
        _check(k)
    buf = C.create_string_buffer(k + 1)
    k2 = lib.rt_debug_jit_header(C.byref(params), arr, n, C.byref(cam), 1 if grouped else 0, buf, k + 1)
    if k2 < 0:
        _check(k2)
    return buf.value.decode()


def brute_layout(prims: Sequence[rt_prim]) -> dict:
    """rt_debug_brute_layout (host code, no GPU): how the brute-force kernels would test these
    primitives -- world rectangles, boxes, frames, triangles, spheres, planes, and the grouping."""
    lib = load_library()
    n = len(prims)
    arr = (rt_prim * max(1, n))(*prims)
    out = (C.c_int32 * len(LAYOUT_NAMES))()
    _check(lib.rt_debug_brute_layout(arr, n, out, len(LAYOUT_NAMES)))
    return dict(zip(LAYOUT_NAMES, (int(v) for v in out)))


def item_order(w: int, h: int, spp: int, chunks: int = 0, pool: int = 0,
               bands: Optional[Tuple[int, int, int]] = None) -> Tuple[np.ndarray, dict]:
    """rt_debug_item_order (host code, no GPU): the tickets the path kernels' dispensers deal for a
    launch over a w x h tile (bands = (band, stride, offset): that band set of an h-row frame), as
    an (n, 3) array of (item range, first item, items) in dealing order per range, and the launch's
    n_chunks, chunk (samples per item), pool (items per full ticket) and n_split."""
    lib = load_library()
    b = bands or (0, 0, 0)
    info = (C.c_int32 * 4)()
    n = lib.rt_debug_item_order(w, h, spp, chunks, pool, b[0], b[1], b[2], None, 0, info)
    if n < 0:
        _check(n)
    out = np.zeros((max(1, n), 3), np.uint32)
    n2 = lib.rt_debug_item_order(w, h, spp, chunks, pool, b[0], b[1], b[2],
                                 out.ctypes.data_as(C.POINTER(C.c_uint32)), 3 * n, info)
    if n2 < 0:
        _check(n2)
    return out[:n], dict(zip(("n_chunks", "chunk", "pool", "n_split"), (int(v) for v in info)))


def scene_bound(prims: Sequence[rt_prim]) -> dict:
    """rt_debug_scene_bound (host code, no GPU): the padded fp32 box over every primitive but the planes
    that the flat brute-force path kernel tests camera rays against -- lo, hi (float32[3]), limit (origins
    with |x| + |y| + |z| above it are not tested), pad, and state: 0 a box, 1 empty, 2 no skip."""
    lib = load_library()
    n = len(prims)
    arr = (rt_prim * max(1, n))(*prims)
    lo, hi, info = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 2)()
    state = lib.rt_debug_scene_bound(arr, n, lo, hi, info)
    if state < 0:
        _check(state)
    return {"lo": np.array(lo, np.float32), "hi": np.array(hi, np.float32), "limit": np.float32(info[0]),
            "pad": np.float32(info[1]), "state": int(state)}


def block_cull(prims: Sequence[rt_prim], camera: rt_camera, size: Tuple[int, int],
               window: Optional[Tuple[int, int, int, int]] = None,
               bands: Optional[Tuple[int, int, int]] = None) -> Tuple[np.ndarray, int]:
    """rt_debug_block_cull (host code, no GPU): the 8x8 pixel blocks of a brute-force launch that the path
    kernels are not dealt, because no camera ray of their pixels can meet the scene bound.  size: the
    frame; window = (x0, y0, w, h), default the frame; bands = (band, stride, offset): that band set of
    the frame (window rows then count the set's rows, default all of them).  Returns the flags as a
    bool array [block rows, blocks per row] (True = dead) and the number of live blocks."""
    lib = load_library()
    n = len(prims)
    arr = (rt_prim * max(1, n))(*prims)
    cam = rt_camera.from_buffer_copy(camera)
    b = bands or (0, 0, 0)
    W, H = size
    rows = lib.rt_band_rows(H, b[0], b[1], b[2]) if bands else H
    x0, y0, w, h = window or (0, 0, W, rows)
    bx, by = (w + 7) // 8, (h + 7) // 8
    dead = np.zeros(max(1, bx * by), np.uint8)
    info = (C.c_int32 * 2)()
    live = lib.rt_debug_block_cull(arr, n, C.byref(cam), W, H, x0, y0, w, h, b[0], b[1], b[2],
                                   dead.ctypes.data_as(C.POINTER(C.c_uint8)), bx * by, info)
    if live < 0:
        _check(live)
    return dead[:bx * by].reshape(by, bx).astype(bool), int(live)


def block_units(prims: Sequence[rt_prim], camera: rt_camera, size: Tuple[int, int],
                window: Optional[Tuple[int, int, int, int]] = None,
                bands: Optional[Tuple[int, int, int]] = None) -> dict:
    """rt_debug_block_units (host code, no GPU): the flat order's test units and, per live 8x8 block of a
    brute-force launch, the units its camera rays can meet.  Arguments as block_cull's.  Returns n_units,
    ids (per unit, the primitive IDs it stands for), box (float32 [n_units, 2, 3]: each unit's padded box;
    empty past 64 units), pad, dead (bool [block rows, blocks per row]), live, masks (uint64 per live
    block, in the blocks' order; bit u clear: unit u cannot be met) and on (the masks are in use)."""
    lib = load_library()
    n = len(prims)
    arr = (rt_prim * max(1, n))(*prims)
    cam = rt_camera.from_buffer_copy(camera)
    b = bands or (0, 0, 0)
    W, H = size
    rows = lib.rt_band_rows(H, b[0], b[1], b[2]) if bands else H
    x0, y0, w, h = window or (0, 0, W, rows)
    bx, by = (w + 7) // 8, (h + 7) // 8
    dead = np.zeros(max(1, bx * by), np.uint8)
    masks = np.zeros(max(1, bx * by), np.uint64)
    cap_ids = 8 * max(1, n) + 64
    first = np.zeros(65, np.int32)
    ids = np.zeros(cap_ids, np.int32)
    box = np.zeros((64, 2, 3), np.float32)
    info = (C.c_int32 * 6)()
    nu = lib.rt_debug_block_units(arr, n, C.byref(cam), W, H, x0, y0, w, h, b[0], b[1], b[2],
                                  first.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                  cap_ids, box.ctypes.data_as(C.POINTER(C.c_float)),
                                  dead.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  masks.ctypes.data_as(C.POINTER(C.c_uint64)), bx * by, info)
    if nu < 0:
        _check(nu)
    live = int(info[2])
    per_unit = [ids[first[u]:first[u + 1]].tolist() for u in range(nu)] if nu <= 64 and info[4] <= cap_ids else []
    return {"n_units": int(nu), "ids": per_unit, "box": box[:nu] if nu <= 64 else box[:0],
            "pad": float(np.array([info[5]], np.int32).view(np.float32)[0]),
            "dead": dead[:bx * by].reshape(by, bx).astype(bool), "live": live, "masks": masks[:live].copy(),
            "on": bool(info[3])}


def start_rows(kernel: int, camera: rt_camera, w: int, h: int, spp: int, chunks: int = 0, grid_blocks: int = 1792,
               instrumented: bool = False, vertex_normals: bool = False) -> dict:
    """rt_debug_start_rows (host code, no GPU): whether a brute-force launch over a w x h tile at spp
    samples per pixel keeps its camera rays in start rows, and what they take -- on, rows (per wave),
    bytes (of the buffer) and chunk (samples per work item).  grid_blocks: blocks of the persistent
    grid (default: 256 CUs x 7)."""
    lib = load_library()
    cam = rt_camera.from_buffer_copy(camera)
    info = (C.c_int64 * 3)()
    on = lib.rt_debug_start_rows(kernel, C.byref(cam), w, h, spp, chunks, grid_blocks,
                                 int(bool(instrumented)) | int(bool(vertex_normals)) << 1, info)
    if on < 0:
        _check(on)
    return {"on": bool(on), "rows": int(info[0]), "bytes": int(info[1]), "chunk": int(info[2])}


def launch_overlap(device_entry: bool = True, repeats: bool = True, bvh: bool = False, instrumented: bool = False, tracing: bool = False, partial_bytes: int = 0,
                   pkeys_rebuilt: bool = False, cull_fresh: bool = False, cull_replaced: bool = False,
                   jit_rebuilt: bool = False, buffer_grown: bool = False) -> Tuple[bool, int]:
    """rt_debug_launch_overlap (host code, no GPU): (whether such a launch overlaps the one before it, what it
    waits for before it rewrites shared state: 0 nothing, 1 the other launch set's path kernel on the set's
    stream, 2 the same on the host)."""
    lib = load_library()
    wait = C.c_int32(-1)
    on = lib.rt_debug_launch_overlap(int(bool(device_entry)) | int(bool(instrumented)) << 1 | int(bool(tracing)) << 2
                                     | int(bool(repeats)) << 3 | int(bool(bvh)) << 4,
                                     int(partial_bytes),
                                     int(bool(pkeys_rebuilt)) | int(bool(cull_fresh)) << 1 | int(bool(cull_replaced)) << 2
                                     | int(bool(jit_rebuilt)) << 3 | int(bool(buffer_grown)) << 4, C.byref(wait))
    if on < 0:
        _check(on)
    return bool(on), int(wait.value)


def ref_bvh_export(prims: Sequence[rt_prim]) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """The library's reference-BVH build (host code, no GPU): (leaf prim order, node boxes, nodes, depth)."""
    lib = load_library()
    n = len(prims)
    arr = (rt_prim * max(1, n))(*prims)
    order = np.zeros(max(1, n), np.int32)
    boxes = np.zeros((max(1, 2 * n), 8), np.float64)
    nodes, depth = C.c_int32(0), C.c_int32(0)
    _check(lib.rt_ref_bvh_export(arr, n, order.ctypes.data_as(C.POINTER(C.c_int32)),
                                 boxes.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nodes), C.byref(depth)))
    return order[:n], boxes[:nodes.value], nodes.value, depth.value


def sample_output(sum_rgb: Tuple[float, float, float], samples: int, misses: int,
                  background=(0.0, 0.0, 0.0), background_alpha: float = 0.0, exposure: float = 1.0) -> int:
    """SampleSet.GetOutput (SampleSet.cs:61-113): ARGB int32."""
    lib = load_library()
    return lib.rt_sample_output(rt_color(*sum_rgb), samples, misses, rt_color(*background), background_alpha, exposure)


def device_count() -> int:
    return load_library().rt_device_count()


def camera_rays(camera: rt_camera, size: Tuple[int, int], x0: int = 0, y0: int = 0, w: Optional[int] = None,
                h: Optional[int] = None) -> np.ndarray:
    """rt_camera_rays (host code, no GPU): Camera.GetRay(x, y).Offset(imagePlane) for the integer pixels
    of a tile of a size[0] x size[1] frame, as a RAY_DTYPE array indexed [x, y]: the rays primary_ids traces."""
    lib = load_library()
    if not hasattr(lib, "rt_camera_rays"):
        raise RtError("this build of the library has no rt_camera_rays")
    W, H = int(size[0]), int(size[1])
    w = W - x0 if w is None else w
    h = H - y0 if h is None else h
    out = np.zeros((max(w, 0), max(h, 0)), RAY_DTYPE)
    cam = rt_camera.from_buffer_copy(camera)
    _check(lib.rt_camera_rays(C.byref(cam), W, H, x0, y0, w, h, out.ctypes.data_as(C.c_void_p)))
    return out


def _pack_rays(origins, directions) -> np.ndarray:
    """(n, 3) or (n, 4) origins and directions -> a contiguous RAY_DTYPE array; w is filled with 1 / 0."""
    o = np.asarray(origins, np.float64)
    d = np.asarray(directions, np.float64)
    if o.ndim != 2 or d.ndim != 2 or o.shape[0] != d.shape[0] or o.shape[1] not in (3, 4) or d.shape[1] not in (3, 4):
        raise ValueError("origins and directions must be (n, 3) or (n, 4) arrays of the same n")
    rays = np.zeros(o.shape[0], RAY_DTYPE)
    rays["origin"][:, 3] = 1.0
    rays["origin"][:, :o.shape[1]] = o
    rays["direction"][:, :d.shape[1]] = d
    return rays


def _pack_beams(origins, directions, origin_du, origin_dv, direction_du, direction_dv) -> np.ndarray:
    """Six (n, 3) or (n, 4) arrays -> a contiguous BEAM_DTYPE array (origin w = 1, every other w = 0); or
    one BEAM_DTYPE array as camera_beams returns it, with the other five None."""
    rest = (directions, origin_du, origin_dv, direction_du, direction_dv)
    if all(a is None for a in rest):
        return np.ascontiguousarray(origins, BEAM_DTYPE).reshape(-1)
    if any(a is None for a in rest):
        raise ValueError("beams: six arrays, or one BEAM_DTYPE array and None for the other five")
    parts = [np.asarray(a, np.float64) for a in (origins,) + rest]
    n = parts[0].shape[0] if parts[0].ndim == 2 else -1
    if any(a.ndim != 2 or a.shape[0] != n or a.shape[1] not in (3, 4) for a in parts):
        raise ValueError("origins, directions and the four footprint arrays must be (n, 3) or (n, 4) arrays of the same n")
    beams = np.zeros(n, BEAM_DTYPE)
    beams["origin"][:, 3] = 1.0
    for name, a in zip(BEAM_DTYPE.names, parts):
        beams[name][:, :a.shape[1]] = a
    return beams


def beam_rays_host(origins, directions, origin_du, origin_dv, direction_du, direction_dv, spp: int, seed: int,
                   sample_base: int = 0, stream_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_beam_rays (host code, no GPU): the kernels' sample start compiled for the CPU.  Returns
    (rays [n, spp] of RAY_DTYPE, uv [n, spp, 2] f64): the fp32 ray of sample k of beam i, widened (all zero
    for a degenerate sample or an invalid beam), and its point in the footprint.  render_rays of rays[:, k]
    at spp 1, sample_base + k and the same stream_base gives render_beams' sample k, bit for bit."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_beam_rays"):
        raise RtError("this build of the library has no rt_debug_beam_rays")
    beams = _pack_beams(origins, directions, origin_du, origin_dv, direction_du, direction_dv)
    n = beams.shape[0]
    rays = np.zeros((n, max(spp, 0)), RAY_DTYPE)
    uv = np.zeros((n, max(spp, 0), 2), np.float64)
    _check(lib.rt_debug_beam_rays(beams.ctypes.data_as(C.c_void_p), n, spp, seed, sample_base, stream_base,
                                  rays.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p)))
    return rays, uv


def camera_beams(camera: rt_camera, size: Tuple[int, int], x0: int = 0, y0: int = 0, w: Optional[int] = None,
                 h: Optional[int] = None) -> np.ndarray:
    """rt_camera_beams (host code, no GPU): the beams of the pixels of a tile of a size[0] x size[1] frame
    for the library's own cameras, as a BEAM_DTYPE array indexed [x, y] (the pinhole footprint: no image
    plane offset, no depth of field)."""
    lib = load_library()
    if not hasattr(lib, "rt_camera_beams"):
        raise RtError("this build of the library has no rt_camera_beams")
    W, H = int(size[0]), int(size[1])
    w = W - x0 if w is None else w
    h = H - y0 if h is None else h
    out = np.zeros((max(w, 0), max(h, 0)), BEAM_DTYPE)
    cam = rt_camera.from_buffer_copy(camera)
    _check(lib.rt_camera_beams(C.byref(cam), W, H, x0, y0, w, h, out.ctypes.data_as(C.c_void_p)))
    return out


def _pack_surfels(positions, normals) -> np.ndarray:
    """(n, 3) or (n, 4) positions and normals -> a contiguous SURFEL_DTYPE array (position w = 1, normal
    w = 0); or one SURFEL_DTYPE array with normals None."""
    if normals is None:
        return np.ascontiguousarray(positions, SURFEL_DTYPE).reshape(-1)
    p, nrm = np.asarray(positions, np.float64), np.asarray(normals, np.float64)
    if p.ndim != 2 or p.shape != nrm.shape or p.shape[1] not in (3, 4):
        raise ValueError("positions and normals must be (n, 3) or (n, 4) arrays of the same shape")
    surfels = np.zeros(p.shape[0], SURFEL_DTYPE)
    surfels["position"][:, 3] = 1.0
    surfels["position"][:, :p.shape[1]] = p
    surfels["normal"][:, :p.shape[1]] = nrm
    return surfels


def gather_mean(sum_rgb, samples, misses, ambient) -> np.ndarray:
    """The gathered mean of render_surfels' accumulators, (sum + misses * ambient) / (samples + misses) per
    surfel: a gather sample that meets nothing is a primary miss, for which the reference returns the
    untinted ambient colour (Raytracer.cs:90).  ambient: three floats or an rt_color.  NaN where a surfel
    has no sample at all."""
    amb = np.array([ambient.r, ambient.g, ambient.b] if isinstance(ambient, rt_color) else ambient, np.float64).reshape(3)
    s = np.asarray(sum_rgb, np.float64)
    ns, ms = np.asarray(samples, np.float64), np.asarray(misses, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s + ms[..., None] * amb) / (ns + ms)[..., None]


def _probe_out(n: int, out):
    """render_probes' and probe_fold_host's `out` = (sh f64 [n, 9, 4], samples u32 [n], misses u32 [n]), new
    zeroed arrays for None; checked."""
    if out is None:
        out = (np.zeros((n, 9, 4), np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    if len(out) != 3:
        raise ValueError("out must be (sh, samples, misses)")
    for a, shape, dt in zip(out, ((n, 9, 4), (n,), (n,)), (np.float64, np.uint32, np.uint32)):
        if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
            raise ValueError("out must be C-contiguous (sh f64 [n, 9, 4], samples u32 [n], misses u32 [n])")
    return out


def sh_basis(dirs) -> np.ndarray:
    """rt_debug_sh_basis (host code, no GPU): the nine L2 real spherical-harmonic basis functions of each
    direction of dirs (..., 3), taken as given, as (..., 9): the probes' fold kernel's function compiled for
    the CPU (order Y00, Y1-1, Y10, Y11, Y2-2, Y2-1, Y20, Y21, Y22)."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_sh_basis"):
        raise RtError("this build of the library has no rt_debug_sh_basis")
    d = np.ascontiguousarray(dirs, np.float64)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("dirs must be a (..., 3) array")
    y = np.zeros(d.shape[:-1] + (9,), np.float64)
    _check(lib.rt_debug_sh_basis(d.ctypes.data_as(C.c_void_p), d.size // 3, y.ctypes.data_as(C.c_void_p)))
    return y


def probe_fold_host(rays, rgb, miss, out=None):
    """rt_debug_probe_fold (host code, no GPU): render_probes' accumulation over per-sample results.  rays
    (n, spp) of RAY_DTYPE as surfel_rays reports them in RT_GATHER_SPHERE (a direction of all zeros: a sample
    of an invalid probe), rgb (n, spp, 3) the samples' fp32 colours and miss (n, spp) true for a primary miss:
    what render_rays gives for rays[:, k] at spp 1.  Returns (sh, samples, misses), new or the caller's `out`,
    which the call adds into."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_fold"):
        raise RtError("this build of the library has no rt_debug_probe_fold")
    r = np.ascontiguousarray(rays, RAY_DTYPE)
    if r.ndim != 2:
        raise ValueError("rays must be an (n, spp) RAY_DTYPE array")
    n, spp = r.shape
    col = np.ascontiguousarray(rgb, np.float32)
    ms = np.ascontiguousarray(np.asarray(miss) != 0, np.uint8)
    if col.shape != (n, spp, 3) or ms.shape != (n, spp):
        raise ValueError("rgb must be (n, spp, 3) and miss (n, spp)")
    sh, ns, nm = _probe_out(n, out)
    _check(lib.rt_debug_probe_fold(r.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                   ms.ctypes.data_as(C.c_void_p), n, spp, sh.ctypes.data_as(C.POINTER(rt_probe_sh)),
                                   ns.ctypes.data_as(C.POINTER(C.c_uint32)), nm.ctypes.data_as(C.POINTER(C.c_uint32))))
    return sh, ns, nm


def probe_radiance_sh(sh, samples, misses, ambient) -> np.ndarray:
    """The radiance coefficients of render_probes' accumulators, L[..., l, ch] = 4 pi / N * (c[l][ch] + c[l][3] *
    ambient[ch]) with N = samples + misses: a sample that met nothing saw the untinted ambient colour (three
    floats or an rt_color) in its direction.  sh (..., 9, 4) -> (..., 9, 3); NaN where a probe has no sample."""
    amb = np.array([ambient.r, ambient.g, ambient.b] if isinstance(ambient, rt_color) else ambient, np.float64).reshape(3)
    c = np.asarray(sh, np.float64)
    total = np.asarray(samples, np.float64) + np.asarray(misses, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (4.0 * math.pi / total)[..., None, None] * (c[..., :3] + c[..., 3:4] * amb)


SH_COSINE_LOBE = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)  # A_l of bands 0, 1, 2


def sh_radiance(L, dirs) -> np.ndarray:
    """The radiance the coefficients L (..., 9, 3) reconstruct in the unit directions dirs (..., 3):
    sum over l of L[l] Y_l(dir), (..., 3); the leading shapes broadcast."""
    return np.einsum("...lc,...l->...c", np.asarray(L, np.float64), sh_basis(dirs))


def sh_irradiance(L, normals) -> np.ndarray:
    """The irradiance of a diffuse receiver with the unit normals (..., 3) under the radiance L (..., 9, 3):
    sum over l of A_l L[l] Y_l(n), A = pi, 2 pi / 3 (l = 1 .. 3) and pi / 4 (l = 4 .. 8), the cosine lobe's
    zonal coefficients (Ramamoorthi and Hanrahan 2001); (..., 3).  Exact for radiance of bands 0 .. 2."""
    return np.einsum("...lc,...l->...c", np.asarray(L, np.float64), sh_basis(normals) * SH_COSINE_LOBE)


def _ambient_arg(ambient) -> rt_color:
    return ambient if isinstance(ambient, rt_color) else rt_color(*[float(v) for v in np.asarray(ambient, np.float64).reshape(3)])


def probe_radiance_host(sh, samples, misses, ambient) -> np.ndarray:
    """rt_debug_probe_radiance (host code, no GPU): probe_radiance_sh by the device pass's function compiled for
    the CPU, bit for bit the same numbers, except that a probe without a sample is all NaN by an explicit
    store.  sh (n, 9, 4), samples and misses (n,) -> L (n, 9, 3)."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_radiance"):
        raise RtError("this build of the library has no rt_debug_probe_radiance")
    c = np.ascontiguousarray(sh, np.float64)
    if c.ndim != 3 or c.shape[1:] != (9, 4):
        raise ValueError("sh must be an (n, 9, 4) array")
    n = c.shape[0]
    ns, nm = np.ascontiguousarray(samples, np.uint32), np.ascontiguousarray(misses, np.uint32)
    if ns.shape != (n,) or nm.shape != (n,):
        raise ValueError("samples and misses must be (n,) arrays")
    L = np.zeros((n, 9, 3), np.float64)
    _check(lib.rt_debug_probe_radiance(c.ctypes.data_as(C.POINTER(rt_probe_sh)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       nm.ctypes.data_as(C.POINTER(C.c_uint32)), n, _ambient_arg(ambient),
                                       L.ctypes.data_as(C.POINTER(C.c_double))))
    return L


def probe_radiance_device(d_sh, d_samples, d_misses, n: int, ambient, d_L, stream: int = 0) -> None:
    """rt_probe_radiance_device: L (n x 9 x 3 doubles at d_L) from rt_render_probes' device accumulators, on the
    current device, asynchronous on `stream`.  The device arrays as torch tensors or as pointers (integers)."""
    lib = load_library()
    if not hasattr(lib, "rt_probe_radiance_device"):
        raise RtError("this build of the library has no rt_probe_radiance_device")
    _check(lib.rt_probe_radiance_device(C.c_void_p(_ptr(d_sh)), C.c_void_p(_ptr(d_samples)), C.c_void_p(_ptr(d_misses)), n,
                                        _ambient_arg(ambient), C.c_void_p(_ptr(d_L)), C.c_void_p(stream)))


def probe_moments_host(rays, rgb, miss, out=None) -> np.ndarray:
    """rt_debug_probe_moments (host code, no GPU): render_probe_list_device's moments over probe_fold_host's
    inputs (rays (n, spp) of RAY_DTYPE, rgb (n, spp, 3), miss (n, spp)).  Returns the moments f64 [n, 4, 2], new
    or the caller's `out`, which the call adds into."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_moments"):
        raise RtError("this build of the library has no rt_debug_probe_moments")
    r = np.ascontiguousarray(rays, RAY_DTYPE)
    if r.ndim != 2:
        raise ValueError("rays must be an (n, spp) RAY_DTYPE array")
    n, spp = r.shape
    col = np.ascontiguousarray(rgb, np.float32)
    ms = np.ascontiguousarray(np.asarray(miss) != 0, np.uint8)
    if col.shape != (n, spp, 3) or ms.shape != (n, spp):
        raise ValueError("rgb must be (n, spp, 3) and miss (n, spp)")
    mom = np.zeros((n, 4, 2), np.float64) if out is None else out
    if mom.shape != (n, 4, 2) or mom.dtype != np.float64 or not mom.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous f64 [n, 4, 2] array")
    _check(lib.rt_debug_probe_moments(r.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                      ms.ctypes.data_as(C.c_void_p), n, spp, mom.ctypes.data_as(C.c_void_p)))
    return mom


def probe_select_params(rel_tol: float, min_samples: int, max_samples: int, ambient=(0.0, 0.0, 0.0),
                        irr_floor: float = 1e-3) -> rt_probe_select_params:
    """rt_probe_select_params; ambient as three floats or an rt_color.  The library checks the values."""
    return rt_probe_select_params(float(rel_tol), float(irr_floor), _ambient_arg(ambient), int(min_samples), int(max_samples))


def _probe_acc_host(sh, samples, misses, moments):
    c = np.ascontiguousarray(sh, np.float64)
    if c.ndim != 3 or c.shape[1:] != (9, 4):
        raise ValueError("sh must be an (n, 9, 4) array")
    n = c.shape[0]
    ns, nm = np.ascontiguousarray(samples, np.uint32), np.ascontiguousarray(misses, np.uint32)
    mom = np.ascontiguousarray(moments, np.float64)
    if ns.shape != (n,) or nm.shape != (n,) or mom.shape != (n, 4, 2):
        raise ValueError("samples and misses must be (n,) arrays and moments (n, 4, 2)")
    return c, ns, nm, mom, n


def probe_select_device(params: rt_probe_select_params, d_sh, d_samples, d_misses, d_moments, n_records: int, d_list,
                        cap: int, d_count, stream: int = 0) -> None:
    """rt_probe_select_device: from n_records probes' device accumulators (render_probe_list_device's) the
    entry numbers of the probes that still need samples, ascending, into d_list (at most cap), their number into
    the uint32 at d_count.  Works on the current device; asynchronous on `stream`.  The device arrays as torch
    tensors or as pointers (integers)."""
    lib = load_library()
    if not hasattr(lib, "rt_probe_select_device"):
        raise RtError("this build of the library has no rt_probe_select_device")
    _check(lib.rt_probe_select_device(C.byref(params), C.c_void_p(_ptr(d_sh)), C.c_void_p(_ptr(d_samples)),
                                      C.c_void_p(_ptr(d_misses)), C.c_void_p(_ptr(d_moments)), n_records,
                                      C.c_void_p(0 if d_list is None else _ptr(d_list)), cap, C.c_void_p(_ptr(d_count)),
                                      C.c_void_p(stream)))


def probe_select_host(params: rt_probe_select_params, sh, samples, misses, moments,
                      cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """rt_debug_probe_select, the host twin of probe_select_device (no GPU): sh (n, 9, 4), samples and misses
    (n,), moments (n, 4, 2).  Returns (the first min(count, cap) list entries, count)."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_select"):
        raise RtError("this build of the library has no rt_debug_probe_select")
    c, ns, nm, mom, n = _probe_acc_host(sh, samples, misses, moments)
    cap = n if cap is None else int(cap)
    out = np.zeros(max(cap, 1), np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.rt_debug_probe_select(C.byref(params), ptr(c), ptr(ns), ptr(nm), ptr(mom), n, ptr(out), cap)
    if k < 0:
        _check(int(k))
    return out[:min(int(k), cap)].copy(), int(k)


def probe_error(params: rt_probe_select_params, sh, samples, misses, moments) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_probe_error (host code, no GPU): (se, level) per probe as the selection rule's last step reads
    them: the estimated standard error of the band-0/1 irradiance and its mean luminance; NaN where a probe has
    fewer than two samples."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_error"):
        raise RtError("this build of the library has no rt_debug_probe_error")
    c, ns, nm, mom, n = _probe_acc_host(sh, samples, misses, moments)
    se, level = np.zeros(n, np.float64), np.zeros(n, np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(lib.rt_debug_probe_error(C.byref(params), ptr(c), ptr(ns), ptr(nm), ptr(mom), n, ptr(se), ptr(level)))
    return se, level


def _grid_L(grid: rt_probe_grid, L) -> np.ndarray:
    """A grid's radiance as contiguous (n_probes, 9, 3) doubles; checked against the grid's dims."""
    a = np.ascontiguousarray(L, np.float64)
    n = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    if a.size != n * 27 or a.shape[-2:] != (9, 3):
        raise ValueError("L must hold nx * ny * nz probes of (9, 3) coefficients")
    return a.reshape(n, 9, 3)


def probe_segments_host(grid: rt_probe_grid, positions, normals) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_probe_segments (host code, no GPU): the eight visibility segments of every point, from the
    point (pushed grid.bias along its unit normal) to each probe of its cell, as (rays (n, 8) RAY_DTYPE,
    t_max (n, 8) f64); all zeros for a corner of weight 0, an invalid point or a grid without visibility."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_segments"):
        raise RtError("this build of the library has no rt_debug_probe_segments")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    rays, t_max = np.zeros((n, 8), RAY_DTYPE), np.zeros((n, 8), np.float64)
    _check(lib.rt_debug_probe_segments(C.byref(grid), pts.ctypes.data_as(C.c_void_p), n, rays.ctypes.data_as(C.c_void_p),
                                       t_max.ctypes.data_as(C.POINTER(C.c_double))))
    return rays, t_max


def shade_probes_host(grid: rt_probe_grid, L, positions, normals, occluded=None) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_shade_probes (host code, no GPU): shade_probes' blend with the visibility answers given:
    occluded (n, 8), true where occluded_rays answers True for the segment probe_segments_host reports, or
    None for nothing hidden.  Returns (irradiance (n, 3), weight (n,))."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_shade_probes"):
        raise RtError("this build of the library has no rt_debug_shade_probes")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    coeffs = _grid_L(grid, L)
    occ = None
    if occluded is not None:
        occ = np.ascontiguousarray(np.asarray(occluded) != 0, np.uint8)
        if occ.shape != (n, 8):
            raise ValueError("occluded must be (n, 8)")
    irr, w = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
    _check(lib.rt_debug_shade_probes(C.byref(grid), coeffs.ctypes.data_as(C.POINTER(C.c_double)),
                                     pts.ctypes.data_as(C.c_void_p), n, occ.ctypes.data_as(C.c_void_p) if occ is not None else None,
                                     irr.ctypes.data_as(C.POINTER(rt_color)), w.ctypes.data_as(C.POINTER(C.c_double))))
    return irr, w


def _oct_sgn(a: np.ndarray) -> np.ndarray:
    return np.where(a >= 0.0, 1.0, -1.0)


def oct_texel_dirs() -> np.ndarray:
    """The unit directions T_t of the 64 texels of a probe's 8 x 8 octahedral depth map (rtcore.h, "probe depth
    maps"), t = ty * 8 + tx, as (64, 3) doubles: the definition in numpy, operation by operation."""
    t = np.arange(64)
    u = (2 * (t & 7) + 1).astype(np.float64) / 8.0 - 1.0
    v = (2 * (t >> 3) + 1).astype(np.float64) / 8.0 - 1.0
    z = (1.0 - np.abs(u)) - np.abs(v)
    x = np.where(z < 0.0, (1.0 - np.abs(v)) * _oct_sgn(u), u)
    y = np.where(z < 0.0, (1.0 - np.abs(u)) * _oct_sgn(v), v)
    ln = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / ln, y / ln, z / ln], axis=-1)


def oct_texel(v) -> np.ndarray:
    """The texel (0 .. 63) of vectors v (..., 3), finite and not zero, of any length, by the same definition."""
    a = np.asarray(v, np.float64)
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    s1 = (np.abs(x) + np.abs(y)) + np.abs(z)
    u, w = x / s1, y / s1
    uo = np.where(z < 0.0, (1.0 - np.abs(w)) * _oct_sgn(x), u)
    wo = np.where(z < 0.0, (1.0 - np.abs(u)) * _oct_sgn(y), w)
    tx = np.clip(((uo + 1.0) * 4.0).astype(np.int64), 0, 7)
    ty = np.clip(((wo + 1.0) * 4.0).astype(np.int64), 0, 7)
    return (ty * 8 + tx).astype(np.int32)


def oct_texel_dirs_host() -> np.ndarray:
    """rt_debug_oct_texel_dirs (host code, no GPU): oct_texel_dirs by the kernels' function compiled for the CPU."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_oct_texel_dirs"):
        raise RtError("this build of the library has no rt_debug_oct_texel_dirs")
    out = np.zeros((64, 3), np.float64)
    _check(lib.rt_debug_oct_texel_dirs(out.ctypes.data_as(C.c_void_p)))
    return out


def oct_texel_host(v) -> np.ndarray:
    """rt_debug_oct_texel (host code, no GPU): oct_texel by the kernels' function; -1 for a vector that is zero
    or not finite."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_oct_texel"):
        raise RtError("this build of the library has no rt_debug_oct_texel")
    a = np.ascontiguousarray(v, np.float64)
    if a.shape[-1:] != (3,):
        raise ValueError("v must be (..., 3)")
    out = np.zeros(a.shape[:-1], np.int32)
    _check(lib.rt_debug_oct_texel(a.ctypes.data_as(C.c_void_p), out.size, out.ctypes.data_as(C.c_void_p)))
    return out


def _depth_out(n: int, out):
    """The depth bake's `out` = (depth f64 [n, 3, 64], counts u32 [n, 4]), new zeroed arrays for None."""
    if out is None:
        return np.zeros((n, 3, 64), np.float64), np.zeros((n, 4), np.uint32)
    depth, counts = out
    if (depth.dtype != np.float64 or depth.shape != (n, 3, 64) or counts.dtype != np.uint32 or counts.shape != (n, 4)
            or not depth.flags.c_contiguous or not counts.flags.c_contiguous):
        raise ValueError("out must be contiguous (f64 [n, 3, 64], u32 [n, 4])")
    return depth, counts


def probe_depth_fold_host(params: rt_probe_depth_params, rays, hits, out=None) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_probe_depth_fold (host code, no GPU): render_probe_depth's accumulation over per-sample results.
    rays (n, spp) RAY_DTYPE as surfel_rays reports them in RT_GATHER_SPHERE mode, hits (n, spp) HIT_DTYPE as
    query_rays answers for them.  Added into out = (depth [n, 3, 64], counts [n, 4]); returns them."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_depth_fold"):
        raise RtError("this build of the library has no rt_debug_probe_depth_fold")
    r, h = np.ascontiguousarray(rays, RAY_DTYPE), np.ascontiguousarray(hits, HIT_DTYPE)
    if r.ndim != 2 or r.shape != h.shape:
        raise ValueError("rays and hits must be (n, spp)")
    n, spp = r.shape
    depth, counts = _depth_out(n, out)
    _check(lib.rt_debug_probe_depth_fold(C.byref(params), r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), n, spp,
                                         depth.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
    return depth, counts


def probe_depth_close_host(depth) -> np.ndarray:
    """rt_debug_probe_depth_close (host code, no GPU): D (n, 64, 2) = (mean distance, mean squared distance) per
    texel from the accumulators (n, 3, 64); NaN where a texel has no weight."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_depth_close"):
        raise RtError("this build of the library has no rt_debug_probe_depth_close")
    a = np.ascontiguousarray(depth, np.float64)
    if a.ndim != 3 or a.shape[1:] != (3, 64):
        raise ValueError("depth must be (n, 3, 64)")
    D = np.zeros((a.shape[0], 64, 2), np.float64)
    _check(lib.rt_debug_probe_depth_close(a.ctypes.data_as(C.c_void_p), a.shape[0], D.ctypes.data_as(C.c_void_p)))
    return D


def probe_depth_close_device(d_depth, n: int, d_D, stream: int = 0) -> None:
    """rt_probe_depth_close_device: D (n x 64 x 2 doubles at d_D) from the depth bake's device accumulators, on
    the current device, asynchronous on `stream`.  The device arrays as torch tensors or as pointers."""
    lib = load_library()
    if not hasattr(lib, "rt_probe_depth_close_device"):
        raise RtError("this build of the library has no rt_probe_depth_close_device")
    _check(lib.rt_probe_depth_close_device(C.c_void_p(_ptr(d_depth)), n, C.c_void_p(_ptr(d_D)), C.c_void_p(stream)))


def _grid_D(grid: rt_probe_grid, D) -> np.ndarray:
    a = np.ascontiguousarray(D, np.float64)
    n = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    if a.size != n * 128 or a.shape[-2:] != (64, 2):
        raise ValueError("D must hold nx * ny * nz probes of (64, 2) moments")
    return a.reshape(n, 64, 2)


def shade_probes_depth_host(grid: rt_probe_grid, L, D, params: rt_probe_depth_params, positions,
                            normals) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_shade_probes_depth (host code, no GPU): shade_probes_depth's blend, bit for bit.  Returns
    (irradiance (n, 3), weight (n,))."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_shade_probes_depth"):
        raise RtError("this build of the library has no rt_debug_shade_probes_depth")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    coeffs, moments = _grid_L(grid, L), _grid_D(grid, D)
    irr, w = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
    _check(lib.rt_debug_shade_probes_depth(C.byref(grid), C.byref(params), coeffs.ctypes.data_as(C.c_void_p),
                                           moments.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), n,
                                           irr.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)))
    return irr, w


def shade_probes_depth_device(grid: rt_probe_grid, params: rt_probe_depth_params, d_L, d_D, d_points, n: int, d_irradiance,
                              d_weight=0, stream: int = 0) -> None:
    """rt_shade_probes_depth_device: asynchronous depth-weighted shading of n rt_surfel at d_points under the
    grid's L (n_probes x 9 x 3 doubles) and D (n_probes x 64 x 2 doubles), written to n x 3 doubles at
    d_irradiance and n doubles at d_weight (0: not wanted), on the current device and `stream`."""
    lib = load_library()
    if not hasattr(lib, "rt_shade_probes_depth_device"):
        raise RtError("this build of the library has no rt_shade_probes_depth_device")
    _check(lib.rt_shade_probes_depth_device(C.byref(grid), C.byref(params), C.c_void_p(_ptr(d_L)), C.c_void_p(_ptr(d_D)),
                                            C.c_void_p(_ptr(d_points)), n, C.c_void_p(_ptr(d_irradiance)),
                                            C.c_void_p(_ptr(d_weight)), C.c_void_p(stream)))


def _grid_n(grid: rt_probe_grid) -> int:
    return int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])


def _grid_placement(grid: rt_probe_grid, offsets, state):
    """A grid's placement as contiguous ((n_probes, 3) f64 or None, (n_probes,) u32 or None), checked against dims."""
    n = _grid_n(grid)
    o = s = None
    if offsets is not None:
        o = np.ascontiguousarray(offsets, np.float64)
        if o.size != n * 3 or o.shape[-1:] != (3,):
            raise ValueError("offsets must hold nx * ny * nz probes of 3 doubles")
        o = o.reshape(n, 3)
    if state is not None:
        s = np.ascontiguousarray(state, np.uint32).reshape(-1)
        if s.size != n:
            raise ValueError("state must hold nx * ny * nz uint32")
    return o, s


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def probe_positions_host(grid: rt_probe_grid, offsets=None) -> np.ndarray:
    """rt_debug_probe_positions (host code, no GPU): the grid's probes as (n_probes,) SURFEL_DTYPE, position
    (origin + i * step) + offset and normal (0, 0, 1); a probe with a non-finite offset is four NaNs."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_positions"):
        raise RtError("this build of the library has no rt_debug_probe_positions")
    o, _ = _grid_placement(grid, offsets, None)
    out = np.zeros(_grid_n(grid), SURFEL_DTYPE)
    _check(lib.rt_debug_probe_positions(C.byref(grid), _np_ptr(o), _np_ptr(out)))
    return out


def probe_positions_device(grid: rt_probe_grid, d_offsets, d_probes_out, stream: int = 0) -> None:
    """rt_probe_positions_device: n_probes rt_surfel (64 B each) at d_probes_out from the grid and the offsets at
    d_offsets (0: none), on the current device, asynchronous on `stream`."""
    lib = load_library()
    if not hasattr(lib, "rt_probe_positions_device"):
        raise RtError("this build of the library has no rt_probe_positions_device")
    _check(lib.rt_probe_positions_device(C.byref(grid), C.c_void_p(_optr(d_offsets)), C.c_void_p(_ptr(d_probes_out)),
                                         C.c_void_p(stream)))


def probe_relocate_host(grid: rt_probe_grid, params: rt_probe_relocate_params, rays, hits, offsets=None):
    """rt_debug_probe_relocate (host code, no GPU): one relocation step's fold and rule over per-sample results.
    rays (n_probes, spp) RAY_DTYPE as surfel_rays reports them in RT_GATHER_SPHERE mode at probe_positions, hits
    (n_probes, spp) HIT_DTYPE as query_rays answers for them, offsets (n_probes, 3) or None for zeros.  Returns
    (offsets after the step, info (n_probes,) RELOCATION_DTYPE); the argument is not changed."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_relocate"):
        raise RtError("this build of the library has no rt_debug_probe_relocate")
    r, h = np.ascontiguousarray(rays, RAY_DTYPE), np.ascontiguousarray(hits, HIT_DTYPE)
    n = _grid_n(grid)
    if r.ndim != 2 or r.shape != h.shape or r.shape[0] != n:
        raise ValueError("rays and hits must be (n_probes, spp)")
    o, _ = _grid_placement(grid, np.zeros((n, 3)) if offsets is None else offsets, None)
    o = o.copy()
    info = np.zeros(n, RELOCATION_DTYPE)
    _check(lib.rt_debug_probe_relocate(C.byref(grid), C.byref(params), _np_ptr(r), _np_ptr(h), r.shape[1], _np_ptr(o),
                                       _np_ptr(info)))
    return o, info


def probe_segments_placed_host(grid: rt_probe_grid, offsets, state, positions, normals) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_probe_segments_placed (host code, no GPU): probe_segments_host for probes at their placed
    positions; the empty segment also for a probe that is RT_PROBE_INSIDE or has a non-finite offset."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_probe_segments_placed"):
        raise RtError("this build of the library has no rt_debug_probe_segments_placed")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    o, s = _grid_placement(grid, offsets, state)
    rays, t_max = np.zeros((n, 8), RAY_DTYPE), np.zeros((n, 8), np.float64)
    _check(lib.rt_debug_probe_segments_placed(C.byref(grid), _np_ptr(o), _np_ptr(s), _np_ptr(pts), n, _np_ptr(rays),
                                              _np_ptr(t_max)))
    return rays, t_max


def shade_probes_placed_host(grid: rt_probe_grid, offsets, state, L, positions, normals,
                             occluded=None) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_shade_probes_placed (host code, no GPU): shade_probes_host without the probes the placement makes
    absent; occluded as there, for probe_segments_placed_host's segments."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_shade_probes_placed"):
        raise RtError("this build of the library has no rt_debug_shade_probes_placed")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    coeffs = _grid_L(grid, L)
    o, s = _grid_placement(grid, offsets, state)
    occ = None
    if occluded is not None:
        occ = np.ascontiguousarray(np.asarray(occluded) != 0, np.uint8)
        if occ.shape != (n, 8):
            raise ValueError("occluded must be (n, 8)")
    irr, w = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
    _check(lib.rt_debug_shade_probes_placed(C.byref(grid), _np_ptr(o), _np_ptr(s), _np_ptr(coeffs), _np_ptr(pts), n, _np_ptr(occ),
                                            _np_ptr(irr), _np_ptr(w)))
    return irr, w


def shade_probes_depth_placed_host(grid: rt_probe_grid, offsets, state, L, D, params: rt_probe_depth_params, positions,
                                   normals) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_shade_probes_depth_placed (host code, no GPU): shade_probes_depth_host with the distances and
    texels taken from the placed positions and without the absent probes."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_shade_probes_depth_placed"):
        raise RtError("this build of the library has no rt_debug_shade_probes_depth_placed")
    pts = _pack_surfels(positions, normals)
    n = pts.shape[0]
    coeffs, moments = _grid_L(grid, L), _grid_D(grid, D)
    o, s = _grid_placement(grid, offsets, state)
    irr, w = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
    _check(lib.rt_debug_shade_probes_depth_placed(C.byref(grid), _np_ptr(o), _np_ptr(s), C.byref(params), _np_ptr(coeffs),
                                                  _np_ptr(moments), _np_ptr(pts), n, _np_ptr(irr), _np_ptr(w)))
    return irr, w


def shade_probes_depth_placed_device(grid: rt_probe_grid, d_offsets, d_state, params: rt_probe_depth_params, d_L, d_D, d_points,
                                     n: int, d_irradiance, d_weight=0, stream: int = 0) -> None:
    """rt_shade_probes_depth_placed_device: shade_probes_depth_device with n_probes x 3 doubles at d_offsets and
    n_probes uint32 at d_state (0: none)."""
    lib = load_library()
    if not hasattr(lib, "rt_shade_probes_depth_placed_device"):
        raise RtError("this build of the library has no rt_shade_probes_depth_placed_device")
    _check(lib.rt_shade_probes_depth_placed_device(C.byref(grid), C.c_void_p(_optr(d_offsets)), C.c_void_p(_optr(d_state)),
                                                   C.byref(params), C.c_void_p(_ptr(d_L)), C.c_void_p(_ptr(d_D)),
                                                   C.c_void_p(_ptr(d_points)), n, C.c_void_p(_ptr(d_irradiance)),
                                                   C.c_void_p(_ptr(d_weight)), C.c_void_p(stream)))


def probe_backface_share(counts) -> np.ndarray:
    """Inside hits divided by hits of the depth bake's counts (..., 4) = (hits, inside hits, misses, skipped):
    the share of a probe's hits that met a back face; near 1 for a probe inside geometry.  NaN without a hit."""
    c = np.asarray(counts, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c[..., 0] > 0, c[..., 1] / c[..., 0], np.nan)


def ambient_occlusion(occluded, samples) -> np.ndarray:
    """1 - occluded / samples of occluded_surfels' counts: the share of a point's sample segments that
    reach their end unhindered (in RT_GATHER_COSINE mode the ambient occlusion term).  NaN where a point has
    no sample.  Its standard error is sqrt(p (1 - p) / samples)."""
    occ, ns = np.asarray(occluded, np.float64), np.asarray(samples, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ns > 0, 1.0 - occ / ns, np.nan)


def obscurance_fold_host(params: rt_obscurance_params, rays, hits, out=None) -> np.ndarray:
    """rt_debug_obscurance_fold (host code, no GPU): obscurance_surfels' accumulation over per-sample results.
    rays (n, spp) RAY_DTYPE as surfel_rays reports them, hits (n, spp) HIT_DTYPE as query_rays answers for them.
    Added into out (n,) OBSCURANCE_DTYPE (a new zeroed array without it); returns it."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_obscurance_fold"):
        raise RtError("this build of the library has no rt_debug_obscurance_fold")
    r, h = np.ascontiguousarray(rays, RAY_DTYPE), np.ascontiguousarray(hits, HIT_DTYPE)
    if r.ndim != 2 or r.shape != h.shape:
        raise ValueError("rays and hits must be (n, spp)")
    n, spp = r.shape
    if out is None:
        out = np.zeros(n, OBSCURANCE_DTYPE)
    if out.dtype != OBSCURANCE_DTYPE or out.shape != (n,) or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous (n,) OBSCURANCE_DTYPE array")
    _check(lib.rt_debug_obscurance_fold(C.byref(params), r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), n, spp,
                                        out.ctypes.data_as(C.c_void_p)))
    return out


def obscurance_select_device(params: rt_obscurance_select_params, d_acc, n_records: int, d_list, cap: int, d_count,
                             stream: int = 0) -> None:
    """rt_obscurance_select_device: from n_records entries' device accumulators (48 B each) the entry numbers of
    those that still need samples, ascending, into d_list (at most cap), their number into the uint32 at d_count.
    Works on the current device; asynchronous on `stream`.  The device arrays as torch tensors or as pointers."""
    lib = load_library()
    if not hasattr(lib, "rt_obscurance_select_device"):
        raise RtError("this build of the library has no rt_obscurance_select_device")
    _check(lib.rt_obscurance_select_device(C.byref(params), C.c_void_p(_ptr(d_acc)), n_records,
                                           C.c_void_p(0 if d_list is None else _ptr(d_list)), cap, C.c_void_p(_ptr(d_count)),
                                           C.c_void_p(stream)))


def obscurance_select_host(params: rt_obscurance_select_params, acc, cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """rt_debug_obscurance_select, the host twin of obscurance_select_device (no GPU): acc (n,) OBSCURANCE_DTYPE.
    Returns (the first min(count, cap) list entries, count)."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_obscurance_select"):
        raise RtError("this build of the library has no rt_debug_obscurance_select")
    a = np.ascontiguousarray(acc, OBSCURANCE_DTYPE).reshape(-1)
    cap = a.shape[0] if cap is None else int(cap)
    out = np.zeros(max(cap, 1), np.uint32)
    k = lib.rt_debug_obscurance_select(C.byref(params), a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p), cap)
    if k < 0:
        _check(int(k))
    return out[:min(int(k), cap)].copy(), int(k)


def obscurance_error(params: rt_obscurance_select_params, acc) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_obscurance_error (host code, no GPU): (se, mean) per entry as the stopping rule's last step reads
    them: the estimated standard error of the mean obscurance, and o / samples; NaN where an entry has fewer than
    two samples."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_obscurance_error"):
        raise RtError("this build of the library has no rt_debug_obscurance_error")
    a = np.ascontiguousarray(acc, OBSCURANCE_DTYPE).reshape(-1)
    se, mean = np.zeros(a.shape[0], np.float64), np.zeros(a.shape[0], np.float64)
    _check(lib.rt_debug_obscurance_error(C.byref(params), a.ctypes.data_as(C.c_void_p), a.shape[0], se.ctypes.data_as(C.c_void_p),
                                         mean.ctypes.data_as(C.c_void_p)))
    return se, mean


def ambient_access(acc) -> np.ndarray:
    """1 - o / samples of obscurance accumulators (OBSCURANCE_DTYPE): the share of a point's surroundings that is
    open, hits weighed by their falloff; 1 where an entry has no sample."""
    a = np.asarray(acc)
    o, ns = a["o"].astype(np.float64), a["samples"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ns > 0, 1.0 - o / ns, 1.0)


def bent_normals(acc, normals) -> np.ndarray:
    """The bent normal of obscurance accumulators: acc["bent"] normalised, the mean unoccluded direction; the
    surfel's own unit normal (normals (n, 3) or wider) where bent is zero or not finite."""
    b = np.asarray(acc)["bent"].astype(np.float64)
    nr = np.asarray(normals, np.float64)[..., :3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        own = nr / np.linalg.norm(nr, axis=-1, keepdims=True)
        length = np.linalg.norm(b, axis=-1, keepdims=True)
        ok = np.isfinite(b).all(axis=-1, keepdims=True) & np.isfinite(length) & (length > 0)
        return np.where(ok, b / np.where(ok, length, 1.0), own)


def _surfel_t_max(t_max, n: int) -> Optional[np.ndarray]:
    """occluded_surfels' t_max (None, a scalar or an array of n) as n contiguous doubles, or None."""
    if t_max is None:
        return None
    t = np.asarray(t_max, np.float64)
    if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != n):
        raise ValueError("t_max must be None, a scalar or an array with one value per surfel")
    return np.ascontiguousarray(np.broadcast_to(t, (n,)))


def prim_surfels(prim: rt_prim, width: int, height: int, offset: float, flip: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The texel centres of a triangle primitive's parallelogram as surfels: with v0, e01, e02 = prim.p,
    positions[i, j] = v0 + (i + 1/2) / width * e01 + (j + 1/2) / height * e02 pushed `offset` along the unit
    normal, which is e01 x e02 normalised (negated with flip).  Returns (positions, normals), both
    (width, height, 3) f64.  Raises for any other primitive kind."""
    if prim.kind != RT_PRIM_TRIANGLE:
        raise ValueError("prim_surfels: a triangle primitive (v0, e01, e02) is needed")
    if width <= 0 or height <= 0:
        raise ValueError("prim_surfels: width and height must be positive")
    v0, e01, e02 = (np.array([v.x, v.y, v.z], np.float64) for v in prim.p)
    nrm = np.cross(e01, e02)
    length = np.sqrt(nrm @ nrm)
    if not length > 0.0:
        raise ValueError("prim_surfels: the triangle is degenerate")
    nrm = nrm / length * (-1.0 if flip else 1.0)
    u = ((np.arange(width) + 0.5) / width)[:, None, None]
    v = ((np.arange(height) + 0.5) / height)[None, :, None]
    positions = v0 + u * e01 + v * e02 + offset * nrm
    return positions, np.broadcast_to(nrm, positions.shape).copy()


def _ptr(a) -> int:
    """A device pointer as an integer: a torch tensor's data_ptr(), or the integer itself."""
    return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a)


def _optr(a) -> int:
    """_ptr with None for a null pointer."""
    return 0 if a is None else _ptr(a)


def _to_numpy(a):
    """A device tensor brought to the host; None and host arrays as they are."""
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def _pack_items(items) -> np.ndarray:
    """A selection list -- an (n, 2) int array, a sequence of (kind, index) pairs or a SELECT_ITEM_DTYPE
    array -- as a contiguous SELECT_ITEM_DTYPE array."""
    if isinstance(items, np.ndarray) and items.dtype == SELECT_ITEM_DTYPE:
        return np.ascontiguousarray(items.reshape(-1))
    a = np.asarray(items, np.int64)
    if a.size == 0:
        return np.zeros(0, SELECT_ITEM_DTYPE)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("items must be an (n, 2) int array or a sequence of (kind, index) pairs")
    if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
        raise ValueError("items: kind and index must fit in int32")
    out = np.zeros(a.shape[0], SELECT_ITEM_DTYPE)
    out["kind"], out["index"] = a[:, 0], a[:, 1]
    return out


def _rays_arg(origins, directions) -> np.ndarray:
    return np.ascontiguousarray(origins, RAY_DTYPE) if directions is None else _pack_rays(origins, directions)


def segment_rays(points_a, points_b) -> Tuple[np.ndarray, np.ndarray]:
    """The segments a -> b as rays for occluded_rays (GpuRaytracer.visible): points as (..., 3) arrays of
    one shape.  Returns a RAY_DTYPE array of the leading shape with origin a and direction
    normalize(b - a), and t_max = |b - a| (fp64, hypot-scaled so that tiny and huge separations keep
    their precision).  Coincident points give a zero direction and t_max 0: an empty segment, which
    nothing occludes."""
    a = np.asarray(points_a, np.float64)
    b = np.asarray(points_b, np.float64)
    if a.shape != b.shape or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("points_a and points_b must be (..., 3) arrays of the same shape")
    v = b - a
    scale = np.max(np.abs(v), axis=-1)
    safe = np.where(scale > 0, scale, 1.0)
    u = v / safe[..., None]
    norm = np.sqrt(np.sum(u * u, axis=-1))
    t_max = np.where(scale > 0, norm * safe, 0.0)
    d = u / np.where(scale > 0, norm, 1.0)[..., None]
    # one more normalisation step: |d| = 1 to the last bit or two
    d = d / np.where(scale > 0, np.sqrt(np.sum(d * d, axis=-1)), 1.0)[..., None]
    rays = np.zeros(a.shape[:-1], RAY_DTYPE)
    rays["origin"][..., :3] = a
    rays["origin"][..., 3] = 1.0
    rays["direction"][..., :3] = d
    return rays, t_max


def select_rays_host(prims: Sequence[rt_prim], items, origins, directions=None) -> np.ndarray:
    """rt_debug_select_rays (host code, no GPU): GpuRaytracer.select_rays for the scene these primitives
    make, by the same fold compiled for the CPU.  Returns a SELECTION_DTYPE array of the rays' shape."""
    lib = load_library()
    if not hasattr(lib, "rt_debug_select_rays"):
        raise RtError("this build of the library has no rt_debug_select_rays")
    n = len(prims)
    arr = prims if isinstance(prims, C.Array) and n > 0 else (rt_prim * max(1, n))(*prims)
    it = _pack_items(items)
    rays = _rays_arg(origins, directions)
    out = np.zeros(rays.shape, SELECTION_DTYPE)
    _check(lib.rt_debug_select_rays(arr, n, it.ctypes.data_as(C.c_void_p), it.size, rays.ctypes.data_as(C.c_void_p),
                                    rays.size, out.ctypes.data_as(C.c_void_p)))
    return out


class GpuRaytracer:
    """One device scene: the drop-in for a `Raytracer` worker (Raytracer.cs:12-49, 294-330).

    Tile buffers follow the C# DoubleColor[w, h] order: element (x, y) at x*h + y.
    """

    def __init__(self, scene: ParsedScene, camera_index: int = 0, device: int = 0,
                 size: Optional[Tuple[int, int]] = None, traversal: int = RT_TRAVERSAL_AUTO,
                 builder: Optional[int] = None):
        lib = load_library()
        self.lib = lib
        self.params = rt_scene_params.from_buffer_copy(scene.params)
        if size is not None:
            self.params.width, self.params.height = int(size[0]), int(size[1])
        self.width, self.height = self.params.width, self.params.height
        self.handle = C.c_void_p()
        n = scene.n_prims
        prims = scene.prims if isinstance(scene.prims, C.Array) and n > 0 else (rt_prim * max(1, n))(*scene.prims)
        if builder is not None:  # process-wide in the library: set for this create only
            _check(lib.rt_set_bvh_builder(builder))
        try:
            _check(lib.rt_scene_create(C.byref(self.params), prims, n, device, C.byref(self.handle)))
        finally:
            if builder is not None:
                lib.rt_set_bvh_builder(RT_BVH_BUILDER_AUTO)
        self.device = device
        if len(scene.cameras) == 0:
            raise RtError("scene has no camera")
        self.camera = rt_camera.from_buffer_copy(scene.cameras[camera_index])
        _check(lib.rt_scene_set_camera(self.handle, C.byref(self.camera)))
        if traversal != RT_TRAVERSAL_AUTO:
            self.set_traversal(traversal)

    def close(self) -> None:
        if self.handle:
            self.lib.rt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_traversal(self, traversal: int) -> None:
        _check(self.lib.rt_scene_set_traversal(self.handle, traversal))

    def set_camera(self, camera: rt_camera) -> None:
        """rt_scene_set_camera: the renders that follow use this camera (the frame size stays)."""
        self.camera = rt_camera.from_buffer_copy(camera)
        _check(self.lib.rt_scene_set_camera(self.handle, C.byref(self.camera)))

    def info(self) -> rt_scene_info:
        inf = rt_scene_info()
        _check(self.lib.rt_scene_get_info(self.handle, C.byref(inf)))
        return inf

    def check_bvh(self) -> None:
        """rt_scene_check_bvh: structural validation of the device BVHs (raises RtError)."""
        _check(self.lib.rt_scene_check_bvh(self.handle))

    def jit_error(self) -> str:
        """rt_scene_get_jit_error: why the last scene-specialised build failed ("" if it did not)."""
        buf = C.create_string_buffer(4096)
        self.lib.rt_scene_get_jit_error(self.handle, buf, len(buf))
        return buf.value.decode(errors="replace")

    def build_stats(self) -> dict:
        """rt_scene_get_build_stats: scene-creation timings and the BVH builder's figures."""
        out = (C.c_double * len(BUILD_STAT_NAMES))()
        _check(self.lib.rt_scene_get_build_stats(self.handle, out, len(BUILD_STAT_NAMES)))
        return dict(zip(BUILD_STAT_NAMES, (float(v) for v in out)))

    def primary_ids(self, x0: int = 0, y0: int = 0, w: Optional[int] = None, h: Optional[int] = None) -> np.ndarray:
        """DebugRaycaster Primitives-mode IDs as an int32 array indexed [x, y]."""
        w = self.width - x0 if w is None else w
        h = self.height - y0 if h is None else h
        ids = np.empty((w, h), np.int32)
        _check(self.lib.rt_primary_ids(self.handle, x0, y0, w, h, ids.ctypes.data_as(C.POINTER(C.c_int32))))
        return ids

    def bvh_counts(self, x0: int = 0, y0: int = 0, w: Optional[int] = None, h: Optional[int] = None) -> np.ndarray:
        """DebugRaycaster BoundingVolumes mode: reference-BVH node counts as int32 [x, y]."""
        w = self.width - x0 if w is None else w
        h = self.height - y0 if h is None else h
        out = np.empty((w, h), np.int32)
        _check(self.lib.rt_bvh_counts(self.handle, x0, y0, w, h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def render_tile(self, x0: int, y0: int, w: int, h: int, spp: int, seed: int = 0, sample_base: int = 0, out=None):
        """Accumulators (sum[w,h,3] f64, samples[w,h] u32, misses[w,h] u32, rays): new zeroed arrays, or
        the caller's `out` = (sum, samples, misses), which the call adds into (SampleSet's merge)."""
        if out is None:
            out = (np.zeros((w, h, 3), np.float64), np.zeros((w, h), np.uint32), np.zeros((w, h), np.uint32))
        s, n, m = out
        for a, shape, dt in ((s, (w, h, 3), np.float64), (n, (w, h), np.uint32), (m, (w, h), np.uint32)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous (sum f64 [w, h, 3], samples u32 [w, h], misses u32 [w, h])")
        rays = C.c_uint64(0)
        _check(self.lib.rt_render_tile(self.handle, x0, y0, w, h, spp, seed, sample_base,
                                       s.ctypes.data_as(C.POINTER(rt_color)),
                                       n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       m.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rays)))
        return s, n, m, rays.value

    def render_bands(self, band: int, band_stride: int, band_offset: int, spp: int, seed: int = 0,
                     sample_base: int = 0, out=None):
        """rt_render_bands: one band set of the frame added into whole-frame accumulators
        (sum[W,H,3] f64, samples[W,H] u32, misses[W,H] u32; new zeroed arrays unless `out`), plus rays."""
        W, H = self.width, self.height
        if out is None:
            out = (np.zeros((W, H, 3), np.float64), np.zeros((W, H), np.uint32), np.zeros((W, H), np.uint32))
        s, n, m = out
        rays = C.c_uint64(0)
        _check(self.lib.rt_render_bands(self.handle, band, band_stride, band_offset, spp, seed, sample_base,
                                        s.ctypes.data_as(C.POINTER(rt_color)), n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        m.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rays)))
        return s, n, m, rays.value

    def render_bands_device(self, band, band_stride, band_offset, spp, seed, sample_base, d_sum, d_samples, d_misses,
                            plane, d_rays, stream: int = 0) -> None:
        """rt_render_bands_device: asynchronous band-set render into device accumulators (pointers)."""
        _check(self.lib.rt_render_bands_device(self.handle, band, band_stride, band_offset, spp, seed, sample_base,
                                               C.c_void_p(d_sum), C.c_void_p(d_samples), C.c_void_p(d_misses), plane,
                                               C.c_void_p(d_rays), C.c_void_p(stream)))

    def render_tile_1spp(self, x0: int, y0: int, w: int, h: int, seed: int = 0, sample_index: int = 0,
                         out: Optional[np.ndarray] = None) -> np.ndarray:
        """Raytracer.Render one pass: DoubleColor[w, h] with Placeholder (-1) for misses (into `out`,
        a C-contiguous float64 [w, h, 3] array, when given)."""
        if out is None:
            out = np.empty((w, h, 3), np.float64)
        elif out.shape != (w, h, 3) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (w, h, 3)")
        _check(self.lib.rt_render_tile_1spp(self.handle, x0, y0, w, h, seed, sample_index,
                                            out.ctypes.data_as(C.POINTER(rt_color))))
        return out

    def trace_paths(self, x0: int, y0: int, w: int, h: int, spp: int, seed: int = 0, sample_base: int = 0):
        """rt_trace_paths (Raytracer.GetDebugTrace for the library's own samples): the samples
        sample_base .. sample_base+spp-1 of every pixel of the tile as a render with this seed traces
        them.  Returns (records [w, h, spp, recursion+1] of DEBUG_RAY_DTYPE, zero past a path's end;
        n_rays int32 [w, h, spp]; colors float64 [w, h, spp, 3], each as render_tile_1spp returns it)."""
        per = self.params.recursion + 1
        if w <= 0 or h <= 0 or spp <= 0:
            raise ValueError("trace_paths: w, h and spp must be positive")
        if w * h * spp * per > RT_TRACE_MAX_RECORDS:
            raise ValueError(f"trace_paths: more than {RT_TRACE_MAX_RECORDS} records; trace fewer pixels or samples")
        records = np.zeros((w, h, spp, per), DEBUG_RAY_DTYPE)
        n_rays = np.zeros((w, h, spp), np.int32)
        colors = np.zeros((w, h, spp, 3), np.float64)
        _check(self.lib.rt_trace_paths(self.handle, x0, y0, w, h, spp, seed, sample_base,
                                       records.ctypes.data_as(C.POINTER(rt_debug_ray)),
                                       n_rays.ctypes.data_as(C.POINTER(C.c_int32)),
                                       colors.ctypes.data_as(C.POINTER(rt_color))))
        return records, n_rays, colors

    def query_rays(self, origins, directions=None, exact: bool = False) -> np.ndarray:
        """rt_query_rays (Scene.RayTrace(ray, null) for the caller's rays): origins and directions as
        (n, 3) or (n, 4) arrays (w filled with 1 / 0), or one RAY_DTYPE array as camera_rays returns it.
        exact: the fp64 reference query; else the path kernels' fp32 closest hit in the scene's
        traversal mode.  Returns a HIT_DTYPE array of the rays' shape; prim_id -1 marks a miss."""
        if directions is None:
            rays = np.ascontiguousarray(origins, RAY_DTYPE)
        else:
            rays = _pack_rays(origins, directions)
        hits = np.zeros(rays.shape, HIT_DTYPE)
        _check(self.lib.rt_query_rays(self.handle, RT_QUERY_EXACT if exact else RT_QUERY_FAST,
                                      rays.ctypes.data_as(C.c_void_p), rays.size, hits.ctypes.data_as(C.c_void_p)))
        return hits

    def query_rays_device(self, d_rays: int, n: int, d_hits: int, exact: bool = False, stream: int = 0) -> None:
        """rt_query_rays_device: asynchronous query of n rt_ray at device pointer d_rays into n rt_hit at
        d_hits (e.g. torch data_ptr()) on `stream` (a hipStream_t as an integer, 0 = the default stream)."""
        _check(self.lib.rt_query_rays_device(self.handle, RT_QUERY_EXACT if exact else RT_QUERY_FAST, C.c_void_p(d_rays),
                                             n, C.c_void_p(d_hits), C.c_void_p(stream)))

    def occluded_rays(self, origins, directions=None, t_max=None, exact: bool = False) -> np.ndarray:
        """rt_occluded_rays (any-hit visibility): True where Scene.RayTrace(ray, null) hits something at a
        distance < t_max.  Rays as for query_rays; t_max None (+inf for every ray), a scalar, or an array
        of the rays' shape.  A NaN or non-positive t_max, and an invalid ray, give False.  exact: the fp64
        reference query; else the path kernels' fp32 tests, unordered and ending at the first hit.
        Returns a bool array of the rays' shape."""
        rays = _rays_arg(origins, directions)
        if t_max is None:
            tm, ptr = None, None
        else:
            tm = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float64), rays.shape))
            ptr = tm.ctypes.data_as(C.c_void_p)
        out = np.zeros(rays.shape, np.uint8)
        _check(self.lib.rt_occluded_rays(self.handle, RT_QUERY_EXACT if exact else RT_QUERY_FAST,
                                         rays.ctypes.data_as(C.c_void_p), ptr, rays.size, out.ctypes.data_as(C.c_void_p)))
        return out.view(np.bool_)

    def occluded_rays_device(self, d_rays: int, d_t_max: int, n: int, d_out: int, exact: bool = False, stream: int = 0) -> None:
        """rt_occluded_rays_device: asynchronous query of n rt_ray at device pointer d_rays, bounded by the
        n doubles at d_t_max (0: unbounded), into n bytes at d_out (0 / 1; exact: 255 on a traversal-stack
        overflow) on `stream` (a hipStream_t as an integer, 0 = the default stream)."""
        _check(self.lib.rt_occluded_rays_device(self.handle, RT_QUERY_EXACT if exact else RT_QUERY_FAST, C.c_void_p(d_rays),
                                                C.c_void_p(d_t_max) if d_t_max else None, n, C.c_void_p(d_out),
                                                C.c_void_p(stream)))

    def visible(self, points_a, points_b, exact: bool = False) -> np.ndarray:
        """True where nothing lies on the segment from points_a[i] to points_b[i] ((..., 3) arrays of one
        shape): occluded_rays with direction normalize(b - a) and t_max = |b - a| (segment_rays), negated.
        Coincident points count as visible.  The segment is taken as given: a far point that lies on a
        surface is hidden by that surface whenever rounding puts the hit just short of |b - a|, and a
        near point on a surface by its own, unless the caller shortens the segment or offsets its ends
        (e.g. a + eps * n, and t_max * (1 - eps))."""
        rays, t_max = segment_rays(points_a, points_b)
        return ~self.occluded_rays(rays, None, t_max, exact=exact)

    def render_rays(self, origins, directions, spp: int, seed: int, sample_base: int = 0, stream_base: int = 0,
                    normalize: bool = False, out=None):
        """rt_render_rays (Raytracer.GetColor(ray) for the caller's rays): spp path-traced samples of each
        ray, sample k of ray i from the stream (seed, stream_base + i, sample_base + k).  origins and
        directions as (n, 3) or (n, 4) arrays, or one RAY_DTYPE array with directions None (as query_rays).
        The directions are taken as given, already normalised; normalize=True normalises them in fp64 here.
        Returns (sum[n, 3] f64, samples[n] u32, misses[n] u32, rays): new zeroed arrays, or the caller's
        `out` = (sum, samples, misses), which the call adds into."""
        rays = np.ascontiguousarray(origins, RAY_DTYPE).reshape(-1) if directions is None \
            else _pack_rays(origins, directions)
        if normalize:
            if directions is None:
                rays = rays.copy()  # (the caller's array is not written)
            d = rays["direction"]
            d[:, :3] /= np.sqrt(np.sum(d[:, :3] * d[:, :3], axis=1))[:, None]
        n = rays.shape[0]
        if out is None:
            out = (np.zeros((n, 3), np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        s, ns, ms = out
        for a, shape, dt in ((s, (n, 3), np.float64), (ns, (n,), np.uint32), (ms, (n,), np.uint32)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous (sum f64 [n, 3], samples u32 [n], misses u32 [n])")
        count = C.c_uint64(0)
        _check(self.lib.rt_render_rays(self.handle, rays.ctypes.data_as(C.c_void_p), n, spp, seed, sample_base,
                                       stream_base, s.ctypes.data_as(C.POINTER(rt_color)),
                                       ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count)))
        return s, ns, ms, count.value

    def render_rays_device(self, d_ray_list: int, n: int, spp: int, seed: int, sample_base: int, stream_base: int,
                           d_sum: int, d_samples: int, d_misses: int, d_rays: int = 0, stream: int = 0) -> None:
        """rt_render_rays_device: asynchronous radiance query of n rt_ray at device pointer d_ray_list, added
        into device accumulators (d_sum: planes R | G | B of n doubles; d_samples, d_misses: n uint32;
        d_rays: one uint64 ray counter or 0) on `stream` (a hipStream_t as an integer, 0 = the default)."""
        _check(self.lib.rt_render_rays_device(self.handle, C.c_void_p(d_ray_list), n, spp, seed, sample_base,
                                              stream_base, C.c_void_p(d_sum), C.c_void_p(d_samples),
                                              C.c_void_p(d_misses), C.c_void_p(d_rays), C.c_void_p(stream)))

    def render_beams(self, origins, directions, origin_du, origin_dv, direction_du, direction_dv, spp: int, seed: int,
                     sample_base: int = 0, stream_base: int = 0, out=None):
        """rt_render_beams: render_rays with each sample at its own point of the beam's footprint,
        origin + u origin_du + v origin_dv and direction + u direction_du + v direction_dv (normalised on the
        device), (u, v) from the two draws render_rays discards.  Six (n, 3) or (n, 4) arrays, or one
        BEAM_DTYPE array (camera_beams) with the other five None.  Returns and `out` as render_rays."""
        beams = _pack_beams(origins, directions, origin_du, origin_dv, direction_du, direction_dv)
        n = beams.shape[0]
        if out is None:
            out = (np.zeros((n, 3), np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        s, ns, ms = out
        for a, shape, dt in ((s, (n, 3), np.float64), (ns, (n,), np.uint32), (ms, (n,), np.uint32)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous (sum f64 [n, 3], samples u32 [n], misses u32 [n])")
        count = C.c_uint64(0)
        _check(self.lib.rt_render_beams(self.handle, beams.ctypes.data_as(C.c_void_p), n, spp, seed, sample_base,
                                        stream_base, s.ctypes.data_as(C.POINTER(rt_color)),
                                        ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count)))
        return s, ns, ms, count.value

    def render_beams_device(self, d_beam_list: int, n: int, spp: int, seed: int, sample_base: int, stream_base: int,
                            d_sum: int, d_samples: int, d_misses: int, d_rays: int = 0, stream: int = 0) -> None:
        """rt_render_beams_device: render_rays_device for n rt_beam (192 B each) at device pointer d_beam_list."""
        _check(self.lib.rt_render_beams_device(self.handle, C.c_void_p(d_beam_list), n, spp, seed, sample_base,
                                               stream_base, C.c_void_p(d_sum), C.c_void_p(d_samples),
                                               C.c_void_p(d_misses), C.c_void_p(d_rays), C.c_void_p(stream)))

    def render_surfels(self, positions, normals, spp: int, seed: int, mode: int = RT_GATHER_DIFFUSE, sample_base: int = 0,
                       stream_base: int = 0, out=None):
        """rt_render_surfels: the radiance arriving at surface points.  spp path-traced samples per surfel,
        each along its own direction about the normal (need not be unit), drawn on the device from the two
        draws render_rays discards: the reference's diffuse bounce (RT_GATHER_DIFFUSE), Lambert's cosine
        (RT_GATHER_COSINE) or the uniform sphere (RT_GATHER_SPHERE).  positions and normals as (n, 3) or
        (n, 4) arrays, or one SURFEL_DTYPE array with normals None.  A caller that leaves a surface offsets
        the positions itself.  Returns and `out` as render_rays; gather_mean turns them into the mean."""
        surfels = _pack_surfels(positions, normals)
        n = surfels.shape[0]
        if out is None:
            out = (np.zeros((n, 3), np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        s, ns, ms = out
        for a, shape, dt in ((s, (n, 3), np.float64), (ns, (n,), np.uint32), (ms, (n,), np.uint32)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous (sum f64 [n, 3], samples u32 [n], misses u32 [n])")
        count = C.c_uint64(0)
        _check(self.lib.rt_render_surfels(self.handle, mode, surfels.ctypes.data_as(C.c_void_p), n, spp, seed, sample_base,
                                          stream_base, s.ctypes.data_as(C.POINTER(rt_color)),
                                          ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count)))
        return s, ns, ms, count.value

    def render_surfels_device(self, d_surfel_list, n: int, spp: int, seed: int, mode: int, sample_base: int,
                              stream_base: int, d_sum, d_samples, d_misses, d_rays=0, stream: int = 0) -> None:
        """rt_render_surfels_device: render_rays_device for n rt_surfel (64 B each) at d_surfel_list.  The
        device arrays as torch tensors or as pointers (integers)."""
        _check(self.lib.rt_render_surfels_device(self.handle, mode, C.c_void_p(_ptr(d_surfel_list)), n, spp, seed,
                                                 sample_base, stream_base, C.c_void_p(_ptr(d_sum)),
                                                 C.c_void_p(_ptr(d_samples)), C.c_void_p(_ptr(d_misses)),
                                                 C.c_void_p(_ptr(d_rays)), C.c_void_p(stream)))

    def render_probes(self, positions, spp: int, seed: int, normals=None, sample_base: int = 0, stream_base: int = 0,
                      out=None):
        """rt_render_probes: light probes.  spp RT_GATHER_SPHERE gather samples per point, sample k of probe i
        render_surfels' (the ray surfel_rays reports), summed under the nine L2 spherical-harmonic basis
        functions of its direction: sh[i, l, 0:3] += colour * Y_l for a hit, sh[i, l, 3] += Y_l for a sample
        that met nothing.  positions (n, 3) or (n, 4); normals only fix the frame the directions are drawn in,
        default (0, 0, 1); or one SURFEL_DTYPE array as positions.  Returns (sh f64 [n, 9, 4], samples u32 [n],
        misses u32 [n], rays): new zeroed arrays, or the caller's `out` = (sh, samples, misses), which the call
        continues from (a + b samples are a samples, then b at sample_base + a, bit for bit).
        probe_radiance_sh turns them into radiance coefficients."""
        if normals is None and not (isinstance(positions, np.ndarray) and positions.dtype == SURFEL_DTYPE):
            pos = np.asarray(positions, np.float64)
            normals = np.zeros_like(pos)
            if pos.ndim == 2 and pos.shape[1] >= 3:
                normals[:, 2] = 1.0
        probes = _pack_surfels(positions, normals)
        n = probes.shape[0]
        sh, ns, ms = _probe_out(n, out)
        count = C.c_uint64(0)
        _check(self.lib.rt_render_probes(self.handle, probes.ctypes.data_as(C.c_void_p), n, spp, seed, sample_base,
                                         stream_base, sh.ctypes.data_as(C.POINTER(rt_probe_sh)),
                                         ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count)))
        return sh, ns, ms, count.value

    def render_probes_device(self, d_probes, n: int, spp: int, seed: int, sample_base: int, stream_base: int, d_sh,
                             d_samples, d_misses, d_rays=0, stream: int = 0) -> None:
        """rt_render_probes_device: asynchronous probes for n rt_surfel (64 B each) at d_probes, added into n
        rt_probe_sh (288 B each: [n, 9, 4] doubles) at d_sh and n uint32 each at d_samples and d_misses (d_rays:
        one uint64 ray counter or 0) on `stream`; 64 * ceil(n / 64) * (spp rounded up to a power of two) must
        not pass 2^26.  The device arrays as torch tensors or as pointers (integers)."""
        _check(self.lib.rt_render_probes_device(self.handle, C.c_void_p(_ptr(d_probes)), n, spp, seed, sample_base,
                                                stream_base, C.c_void_p(_ptr(d_sh)), C.c_void_p(_ptr(d_samples)),
                                                C.c_void_p(_ptr(d_misses)), C.c_void_p(_ptr(d_rays)), C.c_void_p(stream)))

    def render_probe_list_device(self, d_probes, n_records: int, d_index, n: int, spp: int, seed: int, sample_base: int,
                                 stream_base: int, d_sh, d_samples, d_misses, d_moments=0, d_rays=0, stream: int = 0) -> None:
        """rt_render_probe_list_device: asynchronous probes for the n entries listed (uint32 entry numbers at
        d_index, or None: every entry, n == n_records) of the n_records rt_surfel resident at d_probes, added at
        the entry into n_records rt_probe_sh at d_sh, uint32 each at d_samples and d_misses and, where given,
        rt_probe_moments (64 B each: [n_records, 4, 2] doubles) at d_moments (d_rays: one uint64 ray counter or
        0) on `stream`; 64 * ceil(n / 64) * (spp rounded up to a power of two) must not pass 2^26.  The device
        arrays as torch tensors or as pointers (integers)."""
        if not hasattr(self.lib, "rt_render_probe_list_device"):
            raise RtError("this build of the library has no rt_render_probe_list_device")
        _check(self.lib.rt_render_probe_list_device(self.handle, C.c_void_p(_ptr(d_probes)), n_records,
                                                    C.c_void_p(0 if d_index is None else _ptr(d_index)), n, spp, seed,
                                                    sample_base, stream_base, C.c_void_p(_ptr(d_sh)),
                                                    C.c_void_p(_ptr(d_samples)), C.c_void_p(_ptr(d_misses)),
                                                    C.c_void_p(_ptr(d_moments)), C.c_void_p(_ptr(d_rays)),
                                                    C.c_void_p(stream)))

    def bake_probes_adaptive(self, positions, rel_tol: float, min_spp: int, max_spp: int, batch_spp: int, seed: int = 0,
                             normals=None, ambient=None, irr_floor: float = 1e-3, stream_base: int = 0,
                             sample_base: int = 0):
        """gather_adaptive's loop for light probes: render until the estimated standard error of every probe's
        band-0/1 irradiance is at most rel_tol of its mean luminance (rtcore.h, "adaptive light probes"), with
        the probes, the accumulators and the list held on this scene's device.  Each iteration:
        rt_probe_select_device builds the ascending list of probes that still need samples; the list's length
        is read (one 4-byte copy, the loop's only synchronisation); rt_render_probe_list_device adds batch_spp
        samples of the listed probes at sample_base + iteration * batch_spp.  The loop stops when the list is
        empty.  A probe that leaves the list never comes back (its accumulators no longer change), so every
        listed probe has N = iteration * batch_spp.  min_spp and max_spp are rounded up to multiples of
        batch_spp.  positions and normals as render_probes takes them; ambient (three floats or an rt_color)
        defaults to the scene's.
        Returns device tensors sh (n, 9, 4) f64, samples, misses (n,) i32 (the uint32 bits), moments (n, 4, 2)
        f64, spp (n,) i64, and counts, lists, rays, params."""
        import torch

        if batch_spp <= 0 or min_spp <= 0 or max_spp < min_spp:
            raise ValueError("need batch_spp > 0 and 0 < min_spp <= max_spp")
        if normals is None and not (isinstance(positions, np.ndarray) and positions.dtype == SURFEL_DTYPE):
            pos = np.asarray(positions, np.float64)
            normals = np.zeros_like(pos)
            if pos.ndim == 2 and pos.shape[1] >= 3:
                normals[:, 2] = 1.0
        probes = _pack_surfels(positions, normals)
        n = probes.shape[0]
        if n == 0:
            raise ValueError("no probes")
        if ambient is None:
            ambient = self.params.ambient
        up = lambda v: -(-int(v) // batch_spp) * batch_spp  # noqa: E731
        par = probe_select_params(rel_tol, up(min_spp), up(max_spp), ambient, irr_floor)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_probes = torch.from_numpy(probes.view(np.uint8).copy()).to(dev)
            acc = {"sh": torch.zeros((n, 9, 4), dtype=torch.float64, device=dev),
                   "samples": torch.zeros(n, dtype=torch.int32, device=dev),
                   "misses": torch.zeros(n, dtype=torch.int32, device=dev),
                   "moments": torch.zeros((n, 4, 2), dtype=torch.float64, device=dev)}
            d_count = torch.zeros(1, dtype=torch.int32, device=dev)
            d_rays = torch.zeros(1, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts, lists = [], []
            while True:
                lst = torch.empty(n if not counts else counts[-1], dtype=torch.int32, device=dev)
                probe_select_device(par, acc["sh"], acc["samples"], acc["misses"], acc["moments"], n, lst, lst.numel(),
                                    d_count, stream=stream)
                m = int(d_count.item()) & 0xFFFFFFFF
                if m == 0:
                    break
                if m > lst.numel():
                    raise RtError("bake_probes_adaptive: the list of active probes grew")
                lst = lst[:m]
                self.render_probe_list_device(d_probes, n, lst, m, batch_spp, seed,
                                              int(sample_base) + len(counts) * batch_spp, stream_base, acc["sh"],
                                              acc["samples"], acc["misses"], acc["moments"], d_rays, stream)
                counts.append(m)
                lists.append(lst)
            torch.cuda.synchronize(dev)
        acc["spp"] = acc["samples"].to(torch.int64) + acc["misses"].to(torch.int64)
        acc.update(counts=counts, lists=lists, rays=int(d_rays.item()), params=par)
        return acc

    def shade_probes(self, grid: rt_probe_grid, L, positions, normals, offsets=None,
                     state=None) -> Tuple[np.ndarray, np.ndarray]:
        """rt_shade_probes: the irradiance a grid of light probes (probe_grid; L (n_probes, 9, 3) as
        probe_radiance_sh returns it, x fastest) gives at surface points: the trilinear blend of the cell's
        eight probes, without those an any-hit query from the point cannot reach (grid.flags) or that hold a
        NaN, then the nine-term dot product for the point's normal.  positions and normals as render_surfels
        takes them.  Returns (irradiance (n, 3), weight (n,)): weight is the share of the trilinear weight that
        contributed; 0 (and irradiance 0) where no probe did.  With offsets (n_probes, 3) or state (n_probes,)
        given (relocate_probes), rt_shade_probes_placed: the probes sit at their placed positions and those that
        are RT_PROBE_INSIDE or have a non-finite offset are left out."""
        placed = offsets is not None or state is not None
        if not hasattr(self.lib, "rt_shade_probes_placed" if placed else "rt_shade_probes"):
            raise RtError("this build of the library has no rt_shade_probes" + ("_placed" if placed else ""))
        pts = _pack_surfels(positions, normals)
        n = pts.shape[0]
        coeffs = _grid_L(grid, L)
        irr, w = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
        if placed:
            o, s = _grid_placement(grid, _to_numpy(offsets), _to_numpy(state))
            _check(self.lib.rt_shade_probes_placed(self.handle, C.byref(grid), _np_ptr(o), _np_ptr(s), _np_ptr(coeffs),
                                                   _np_ptr(pts), n, _np_ptr(irr), _np_ptr(w)))
            return irr, w
        _check(self.lib.rt_shade_probes(self.handle, C.byref(grid), coeffs.ctypes.data_as(C.POINTER(C.c_double)),
                                        pts.ctypes.data_as(C.c_void_p), n, irr.ctypes.data_as(C.POINTER(rt_color)),
                                        w.ctypes.data_as(C.POINTER(C.c_double))))
        return irr, w

    def shade_probes_device(self, grid: rt_probe_grid, d_L, d_points, n: int, d_irradiance, d_weight=0, stream: int = 0) -> None:
        """rt_shade_probes_device: asynchronous shade_probes for n rt_surfel (64 B each) at d_points under the
        grid's n_probes x 9 x 3 doubles at d_L, written to n x 3 doubles at d_irradiance and n doubles at
        d_weight (0: not wanted) on `stream`.  The device arrays as torch tensors or as pointers (integers)."""
        if not hasattr(self.lib, "rt_shade_probes_device"):
            raise RtError("this build of the library has no rt_shade_probes_device")
        _check(self.lib.rt_shade_probes_device(self.handle, C.byref(grid), C.c_void_p(_ptr(d_L)), C.c_void_p(_ptr(d_points)), n,
                                               C.c_void_p(_ptr(d_irradiance)), C.c_void_p(_ptr(d_weight)), C.c_void_p(stream)))

    def render_probe_depth_device(self, d_probes, n: int, spp: int, seed: int, sample_base: int, stream_base: int,
                                  params: rt_probe_depth_params, d_depth, d_counts, stream: int = 0) -> None:
        """rt_render_probe_depth_device: asynchronous depth bake for n rt_surfel (64 B each) at d_probes, added into
        n rt_probe_depth (1536 B each: [n, 3, 64] doubles) at d_depth and n x 4 uint32 at d_counts on `stream`.
        The device arrays as torch tensors or as pointers (integers)."""
        if not hasattr(self.lib, "rt_render_probe_depth_device"):
            raise RtError("this build of the library has no rt_render_probe_depth_device")
        _check(self.lib.rt_render_probe_depth_device(self.handle, C.c_void_p(_ptr(d_probes)), n, spp, seed, sample_base,
                                                     stream_base, C.byref(params), C.c_void_p(_ptr(d_depth)),
                                                     C.c_void_p(_ptr(d_counts)), C.c_void_p(stream)))

    def render_probe_depth(self, positions, spp: int, seed: int, d_max: float, sharpness: int = 5, normals=None,
                           sample_base: int = 0, stream_base: int = 0, out=None, close: bool = True):
        """Probe depth maps (rtcore.h, "probe depth maps"): spp RT_GATHER_SPHERE samples per point, the ones
        render_probes takes for the same (seed, sample_base, stream_base), folded into each probe's 8 x 8
        octahedral map of distance moments.  positions (n, 3) with normals None (any unit normal: a sphere
        sample's distribution does not depend on it, its directions do) or as render_surfels takes them.
        Everything stays on this scene's device; returns a dict of torch tensors: depth (n, 3, 64) f64, counts
        (n, 4) int32 holding the uint32 counts (hits, inside hits, misses, skipped), and with close D (n, 64, 2)
        f64 for shade_probes_depth.  out: a dict from an earlier call to add into (sample_base continues)."""
        import torch

        if normals is None and not (hasattr(positions, "dtype") and positions.dtype == SURFEL_DTYPE):
            p = np.asarray(positions, np.float64)
            normals = np.tile([0.0, 0.0, 1.0] + [0.0] * (p.shape[1] - 3), (p.shape[0], 1))
        probes = _pack_surfels(positions, normals)
        n = probes.shape[0]
        params = probe_depth_params(d_max, sharpness)
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_probes = torch.from_numpy(probes.view(np.uint8).copy()).to(dev)
            acc = out if out is not None else {"depth": torch.zeros((n, 3, 64), dtype=torch.float64, device=dev),
                                               "counts": torch.zeros((n, 4), dtype=torch.int32, device=dev)}
            if tuple(acc["depth"].shape) != (n, 3, 64) or tuple(acc["counts"].shape) != (n, 4):
                raise ValueError("out does not hold n probes")
            torch.cuda.synchronize()
            self.render_probe_depth_device(d_probes, n, spp, seed, sample_base, stream_base, params, acc["depth"],
                                           acc["counts"])
            if close:
                acc["D"] = torch.empty((n, 64, 2), dtype=torch.float64, device=dev)
                probe_depth_close_device(acc["depth"], n, acc["D"])
            torch.cuda.synchronize()
        return acc

    def _device_placement(self, grid: rt_probe_grid, offsets, state, dev):
        """offsets and state as contiguous device tensors (f64 (n_probes, 3), int32 (n_probes,)) or None."""
        import torch

        n = _grid_n(grid)
        d_o = d_s = None
        if offsets is not None:
            d_o = (offsets if hasattr(offsets, "data_ptr") else torch.from_numpy(_grid_placement(grid, offsets, None)[0].copy()).to(dev))
            if d_o.numel() != n * 3 or d_o.dtype != torch.float64:
                raise ValueError("offsets must hold nx * ny * nz probes of 3 doubles")
            d_o = d_o.contiguous()
        if state is not None:
            d_s = (state if hasattr(state, "data_ptr")
                   else torch.from_numpy(_grid_placement(grid, None, state)[1].view(np.int32).copy()).to(dev))
            if d_s.numel() != n or d_s.dtype != torch.int32:
                raise ValueError("state must hold nx * ny * nz 32-bit words")
            d_s = d_s.contiguous()
        return d_o, d_s

    def probe_positions(self, grid: rt_probe_grid, offsets=None):
        """rt_probe_positions_device on this scene's device: the grid's probes at their placed positions as a
        device tensor (n_probes, 64) uint8 of rt_surfel records, the array the probe bakes take (render_probes_device,
        render_probe_list_device, render_probe_depth_device).  offsets: (n_probes, 3) doubles, host or device, or None."""
        import torch

        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_o, _ = self._device_placement(grid, offsets, None, dev)
            out = torch.empty((_grid_n(grid), 64), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            probe_positions_device(grid, d_o, out)
            torch.cuda.synchronize()
        return out

    def relocate_probes_device(self, grid: rt_probe_grid, params: rt_probe_relocate_params, spp: int, seed: int,
                               sample_base: int, stream_base: int, d_offsets, d_info, stream: int = 0) -> None:
        """rt_relocate_probes_device: one asynchronous relocation step of the grid's probes: n_probes x 3 doubles
        at d_offsets (in/out) and n_probes rt_probe_relocation (64 B each) at d_info (written) on `stream`."""
        if not hasattr(self.lib, "rt_relocate_probes_device"):
            raise RtError("this build of the library has no rt_relocate_probes_device")
        _check(self.lib.rt_relocate_probes_device(self.handle, C.byref(grid), C.byref(params), spp, seed, sample_base, stream_base,
                                                  C.c_void_p(_optr(d_offsets)), C.c_void_p(_optr(d_info)), C.c_void_p(stream)))

    def relocate_probes(self, grid: rt_probe_grid, params: rt_probe_relocate_params, spp: int, steps: int, seed: int,
                        sample_base: int = 0, offsets=None):
        """Probe relocation (rtcore.h, "probe relocation"): `steps` steps on the device, step j with the samples
        sample_base + j * spp .. + spp - 1 of every probe, then one RT_PROBE_RELOCATE_CLASSIFY_ONLY pass with the
        samples after them.  Starts from offsets (n_probes, 3; None: zeros).  Returns (offsets (n_probes, 3) f64,
        state (n_probes,) int32 holding the uint32 bits, info (n_probes, 64) uint8 of rt_probe_relocation records
        -- .cpu().numpy().view(RELOCATION_DTYPE) -- all device tensors, and the list of probes moved per step)."""
        import torch

        n = _grid_n(grid)
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_o, _ = self._device_placement(grid, np.zeros((n, 3)) if offsets is None else offsets, None, dev)
            d_o = d_o.clone().reshape(n, 3)
            d_info = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            moved = []
            torch.cuda.synchronize()
            for j in range(int(steps)):
                self.relocate_probes_device(grid, params, spp, seed, int(sample_base) + j * spp, 0, d_o, d_info)
                moved.append(int(d_info.view(torch.int32)[:, 1].sum().item()))
            last = rt_probe_relocate_params.from_buffer_copy(params)
            last.flags |= RT_PROBE_RELOCATE_CLASSIFY_ONLY
            self.relocate_probes_device(grid, last, spp, seed, int(sample_base) + int(steps) * spp, 0, d_o, d_info)
            torch.cuda.synchronize()
            state = d_info.view(torch.int32)[:, 0].contiguous()
        return d_o, state, d_info, moved

    def shade_probes_placed_device(self, grid: rt_probe_grid, d_offsets, d_state, d_L, d_points, n: int, d_irradiance, d_weight=0,
                                   stream: int = 0) -> None:
        """rt_shade_probes_placed_device: shade_probes_device with n_probes x 3 doubles at d_offsets and n_probes
        uint32 at d_state (None or 0: none)."""
        if not hasattr(self.lib, "rt_shade_probes_placed_device"):
            raise RtError("this build of the library has no rt_shade_probes_placed_device")
        _check(self.lib.rt_shade_probes_placed_device(self.handle, C.byref(grid), C.c_void_p(_optr(d_offsets)),
                                                      C.c_void_p(_optr(d_state)), C.c_void_p(_ptr(d_L)), C.c_void_p(_ptr(d_points)), n,
                                                      C.c_void_p(_ptr(d_irradiance)), C.c_void_p(_optr(d_weight)), C.c_void_p(stream)))

    def probe_segments_placed_device(self, grid: rt_probe_grid, offsets, state, positions, normals) -> Tuple[np.ndarray, np.ndarray]:
        """rt_debug_probe_segments_placed_device on this scene's device: probe_segments_placed_host's (rays, t_max)
        as the device pass makes them, bit for bit the same."""
        import torch

        if not hasattr(self.lib, "rt_debug_probe_segments_placed_device"):
            raise RtError("this build of the library has no rt_debug_probe_segments_placed_device")
        pts = _pack_surfels(positions, normals)
        n = pts.shape[0]
        rays, t_max = np.zeros((n, 8), RAY_DTYPE), np.zeros((n, 8), np.float64)
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_o, d_s = self._device_placement(grid, offsets, state, dev)
            d_in = torch.from_numpy(pts.view(np.uint8).copy()).to(dev)
            d_rays = torch.zeros(max(rays.nbytes, 1), dtype=torch.uint8, device=dev)
            d_t = torch.zeros(max(n * 8, 1), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            _check(self.lib.rt_debug_probe_segments_placed_device(C.byref(grid), C.c_void_p(_optr(d_o)), C.c_void_p(_optr(d_s)),
                                                                  C.c_void_p(d_in.data_ptr() if n else 0), n,
                                                                  C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_t.data_ptr()), None))
            torch.cuda.synchronize()
            if n:
                rays.view(np.uint8).reshape(-1)[:] = d_rays.cpu().numpy()[:rays.nbytes]
                t_max.reshape(-1)[:] = d_t.cpu().numpy()[:n * 8]
        return rays, t_max

    def shade_probes_depth(self, grid: rt_probe_grid, L, D, params: rt_probe_depth_params, positions,
                           normals, offsets=None, state=None) -> Tuple[np.ndarray, np.ndarray]:
        """rt_shade_probes_depth_device on this scene's device: shade_probes without a ray, each corner weighed by
        a Chebyshev test of the point's distance against the probe's depth map D (and by the wrap weight with
        RT_PROBE_DEPTH_WRAP).  grid with flags 0 (probe_grid(..., visibility=False)); L (n_probes, 9, 3) and D
        (n_probes, 64, 2) as numpy arrays or device tensors.  Returns (irradiance (n, 3), weight (n,))."""
        import torch

        pts = _pack_surfels(positions, normals)
        n = pts.shape[0]
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_L = L if hasattr(L, "data_ptr") else torch.from_numpy(_grid_L(grid, L).copy()).to(dev)
            d_D = D if hasattr(D, "data_ptr") else torch.from_numpy(_grid_D(grid, D).copy()).to(dev)
            n_probes = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
            if d_L.numel() != n_probes * 27 or d_D.numel() != n_probes * 128 or d_L.dtype != torch.float64 or d_D.dtype != torch.float64:
                raise ValueError("L and D must hold nx * ny * nz probes of (9, 3) and (64, 2) doubles")
            d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to(dev)
            d_irr = torch.zeros((n, 3), dtype=torch.float64, device=dev)
            d_w = torch.zeros(n, dtype=torch.float64, device=dev)
            d_o, d_s = self._device_placement(grid, offsets, state, dev)
            torch.cuda.synchronize()
            if d_o is not None or d_s is not None:  # the probes at their placed positions, the absent ones left out
                shade_probes_depth_placed_device(grid, d_o, d_s, params, d_L.contiguous(), d_D.contiguous(), d_pts, n, d_irr, d_w)
            else:
                shade_probes_depth_device(grid, params, d_L.contiguous(), d_D.contiguous(), d_pts, n, d_irr, d_w)
            torch.cuda.synchronize()
            return d_irr.cpu().numpy(), d_w.cpu().numpy()

    def probe_segments_device(self, grid: rt_probe_grid, positions, normals) -> Tuple[np.ndarray, np.ndarray]:
        """rt_debug_probe_segments_device on this scene's device: probe_segments_host's (rays, t_max) as the
        device pass makes them, bit for bit the same."""
        import torch

        if not hasattr(self.lib, "rt_debug_probe_segments_device"):
            raise RtError("this build of the library has no rt_debug_probe_segments_device")
        pts = _pack_surfels(positions, normals)
        n = pts.shape[0]
        rays, t_max = np.zeros((n, 8), RAY_DTYPE), np.zeros((n, 8), np.float64)
        with torch.cuda.device(self.device):
            d_in = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
            d_rays = torch.zeros(max(rays.nbytes, 1), dtype=torch.uint8, device="cuda")
            d_t = torch.zeros(max(n * 8, 1), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            _check(self.lib.rt_debug_probe_segments_device(C.byref(grid), C.c_void_p(d_in.data_ptr() if n else 0), n,
                                                           C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_t.data_ptr()), None))
            torch.cuda.synchronize()
            if n:
                rays.view(np.uint8).reshape(-1)[:] = d_rays.cpu().numpy()[:rays.nbytes]
                t_max.reshape(-1)[:] = d_t.cpu().numpy()[:n * 8]
        return rays, t_max

    def surfel_rays(self, positions, normals, spp: int, seed: int, mode: int = RT_GATHER_DIFFUSE, sample_base: int = 0,
                    stream_base: int = 0) -> np.ndarray:
        """rt_debug_surfel_rays_device on this scene's device: the fp32 ray of sample k of surfel i, widened,
        as an (n, spp) RAY_DTYPE array (all zero for an invalid surfel).  render_rays of [:, k] at spp 1,
        sample_base + k and the same stream_base gives render_surfels' sample k, bit for bit."""
        import torch

        surfels = _pack_surfels(positions, normals)
        n = surfels.shape[0]
        rays = np.zeros((n, max(spp, 0)), RAY_DTYPE)
        with torch.cuda.device(self.device):
            d_in = torch.from_numpy(surfels.view(np.uint8).copy()).cuda()
            d_out = torch.zeros(max(rays.nbytes, 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _check(self.lib.rt_debug_surfel_rays_device(mode, C.c_void_p(d_in.data_ptr() if n else 0), n, spp, seed,
                                                        sample_base, stream_base, C.c_void_p(d_out.data_ptr()), None))
            torch.cuda.synchronize()
            if rays.nbytes:
                rays.view(np.uint8).reshape(-1)[:] = d_out.cpu().numpy()[:rays.nbytes]
        return rays

    def occluded_surfels(self, positions, normals, spp: int, seed: int, mode: int = RT_GATHER_COSINE, t_max=None,
                         sample_base: int = 0, stream_base: int = 0, out=None):
        """rt_occluded_surfels: how many of spp sample segments of each surface point are occluded.  The
        directions are render_surfels' (sample k of surfel i from the stream (seed, stream_base + i,
        sample_base + k), the rays surfel_rays reports), each segment starts at the position and ends at t_max:
        None (+inf), a scalar, or one value per surfel.  A sample counts exactly when occluded_rays answers
        True for its ray and t_max.  positions and normals as render_surfels takes them; a caller that leaves
        a surface offsets the positions itself.  Returns (occluded u32[n], samples u32[n]): new zeroed arrays,
        or the caller's `out` = (occluded, samples), which the call adds into; ambient_occlusion turns them
        into 1 - occluded / samples."""
        surfels = _pack_surfels(positions, normals)
        n = surfels.shape[0]
        tm = _surfel_t_max(t_max, n)
        if out is None:
            out = (np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        if len(out) != 2:
            raise ValueError("out must be (occluded, samples)")
        for a in out:
            if a.shape != (n,) or a.dtype != np.uint32 or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous (occluded u32 [n], samples u32 [n])")
        occ, ns = out
        _check(self.lib.rt_occluded_surfels(self.handle, mode, surfels.ctypes.data_as(C.c_void_p), n,
                                            tm.ctypes.data_as(C.c_void_p) if tm is not None else None, spp, seed,
                                            sample_base, stream_base, occ.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            ns.ctypes.data_as(C.POINTER(C.c_uint32))))
        return occ, ns

    def occluded_surfels_device(self, mode: int, d_surfels, n_records: int, d_index, n: int, d_t_max, spp: int, seed: int,
                                sample_base: int, stream_base: int, d_occluded, d_samples=0, stream: int = 0) -> None:
        """rt_occluded_surfels_device: asynchronous counts for the n entries listed (uint32 entry numbers at
        d_index, or None: every entry, n == n_records) of the n_records rt_surfel resident at d_surfels, bounded
        by the n_records doubles at d_t_max (None or 0: unbounded), added into n_records uint32 at d_occluded and
        (unless 0) d_samples on `stream`.  The device arrays as torch tensors or as pointers (integers)."""
        _check(self.lib.rt_occluded_surfels_device(self.handle, mode, C.c_void_p(_ptr(d_surfels)), n_records,
                                                   C.c_void_p(0 if d_index is None else _ptr(d_index)), n,
                                                   C.c_void_p(0 if d_t_max is None else _ptr(d_t_max)), spp, seed, sample_base,
                                                   stream_base, C.c_void_p(_ptr(d_occluded)), C.c_void_p(_ptr(d_samples)),
                                                   C.c_void_p(stream)))

    def obscurance_surfels_device(self, mode: int, d_surfels, n_records: int, d_index, n: int, params: rt_obscurance_params,
                                  spp: int, seed: int, sample_base: int, stream_base: int, d_acc, stream: int = 0) -> None:
        """rt_obscurance_surfels_device: asynchronous falloff obscurance for the n entries listed (uint32 entry
        numbers at d_index, or None: every entry, n == n_records) of the n_records rt_surfel resident at d_surfels,
        added into n_records rt_obscurance (48 B each) at d_acc on `stream`.  The device arrays as torch tensors or
        as pointers (integers)."""
        if not hasattr(self.lib, "rt_obscurance_surfels_device"):
            raise RtError("this build of the library has no rt_obscurance_surfels_device")
        _check(self.lib.rt_obscurance_surfels_device(self.handle, mode, C.c_void_p(_ptr(d_surfels)), n_records,
                                                     C.c_void_p(0 if d_index is None else _ptr(d_index)), n, C.byref(params),
                                                     spp, seed, sample_base, stream_base, C.c_void_p(_ptr(d_acc)),
                                                     C.c_void_p(stream)))

    def obscurance_select_device(self, params: rt_obscurance_select_params, d_acc, n_records: int, d_list, cap: int, d_count,
                                 stream: int = 0) -> None:
        """rt_obscurance_select_device on this scene's device (the module's obscurance_select_device)."""
        import torch

        with torch.cuda.device(self.device):
            obscurance_select_device(params, d_acc, n_records, d_list, cap, d_count, stream)

    def obscurance_surfels(self, positions, normals, spp: int, seed: int, radius: float, power: int = 1,
                           mode: int = RT_GATHER_COSINE, index=None, sample_base: int = 0, stream_base: int = 0,
                           out=None) -> np.ndarray:
        """Obscurance at surface points (rtcore.h, "obscurance at surfels"): spp samples per point, the rays
        surfel_rays reports, each weighed by its closest hit: 0 beyond `radius` or on a miss, else
        (1 - distance / radius)^power (power 0: 1).  Returns an (n,) OBSCURANCE_DTYPE array: o and o2 the sums of
        the weights and of their squares, bent the sum of (1 - weight) * direction, samples and hits; a new zeroed
        array, or the caller's `out`, which the call adds into (sample_base continues).  index: the entries to
        sample (None: all); the others are left as they are.  ambient_access and bent_normals read the result."""
        import torch

        surfels = _pack_surfels(positions, normals)
        n = surfels.shape[0]
        idx = None
        if index is not None:
            idx = np.asarray(index).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= 1 << 32):
                raise ValueError("entry numbers must lie in [0, 2^32)")
            idx = np.ascontiguousarray(idx, np.uint32)
        if out is None:
            out = np.zeros(n, OBSCURANCE_DTYPE)
        if out.dtype != OBSCURANCE_DTYPE or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous (n,) OBSCURANCE_DTYPE array")
        m = n if idx is None else idx.size
        if n == 0 or m == 0:
            return out
        params = obscurance_params(radius, power)
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_surfels = torch.from_numpy(surfels.view(np.uint8).copy()).to(dev)
            d_acc = torch.from_numpy(out.view(np.uint8).copy()).to(dev)
            d_idx = torch.from_numpy(idx.view(np.int32).copy()).to(dev) if idx is not None else None
            torch.cuda.synchronize()
            self.obscurance_surfels_device(mode, d_surfels, n, d_idx, m, params, spp, seed, sample_base, stream_base, d_acc)
            torch.cuda.synchronize()
            out.view(np.uint8)[:] = d_acc.cpu().numpy()
        return out

    def obscurance_adaptive(self, positions, normals, tol: float, min_spp: int, max_spp: int, batch_spp: int, seed: int = 0,
                            radius: float = 1.0, power: int = 1, mode: int = RT_GATHER_COSINE, stream_base: int = 0,
                            sample_base: int = 0):
        """bake_probes_adaptive's loop for obscurance: sample until the estimated standard error of every point's
        mean obscurance is at most tol (rtcore.h, "obscurance at surfels", the rule), with the surfels, the
        accumulators and the list held on this scene's device.  Each iteration: rt_obscurance_select_device builds
        the ascending list of entries that still need samples; the list's length is read (one 4-byte copy, the
        loop's only synchronisation); rt_obscurance_surfels_device adds batch_spp samples of the listed entries at
        sample_base + iteration * batch_spp.  The loop stops when the list is empty.  min_spp and max_spp are
        rounded up to multiples of batch_spp.
        Returns a dict: device tensors acc (n, 48) uint8 (view the host copy as OBSCURANCE_DTYPE) and surfels, and
        counts, lists and params."""
        import torch

        if batch_spp <= 0 or min_spp <= 0 or max_spp < min_spp:
            raise ValueError("need batch_spp > 0 and 0 < min_spp <= max_spp")
        surfels = _pack_surfels(positions, normals)
        n = surfels.shape[0]
        if n == 0:
            raise ValueError("no surfels")
        up = lambda v: -(-int(v) // batch_spp) * batch_spp  # noqa: E731
        par = obscurance_select_params(tol, up(min_spp), up(max_spp))
        fall = obscurance_params(radius, power)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_surfels = torch.from_numpy(surfels.view(np.uint8).copy()).to(dev)
            d_acc = torch.zeros((n, OBSCURANCE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            d_count = torch.zeros(1, dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts, lists = [], []
            while True:
                lst = torch.empty(n if not counts else counts[-1], dtype=torch.int32, device=dev)
                obscurance_select_device(par, d_acc, n, lst, lst.numel(), d_count, stream=stream)
                m = int(d_count.item()) & 0xFFFFFFFF
                if m == 0:
                    break
                if m > lst.numel():
                    raise RtError("obscurance_adaptive: the list of active entries grew")
                lst = lst[:m]
                self.obscurance_surfels_device(mode, d_surfels, n, lst, m, fall, batch_spp, seed,
                                               int(sample_base) + len(counts) * batch_spp, stream_base, d_acc, stream)
                counts.append(m)
                lists.append(lst)
            torch.cuda.synchronize(dev)
        return {"acc": d_acc, "surfels": d_surfels, "counts": counts, "lists": lists, "params": par}

    def render_list(self, kind: int, records, index=None, spp: int = 1, seed: int = 0, mode: int = 0, sample_base: int = 0,
                    stream_base: int = 0, out=None, moments: bool = False):
        """rt_render_list: render_rays, render_beams or render_surfels (kind RT_LIST_RAYS, RT_LIST_BEAMS,
        RT_LIST_SURFELS; mode: the surfels' gather mode, 0 otherwise) for the entries `index` lists of
        `records`, one RAY_DTYPE, BEAM_DTYPE or SURFEL_DTYPE array as _pack_rays, _pack_beams or
        _pack_surfels make it; index None lists every entry.  Sample k of entry e draws from (seed,
        stream_base + e, sample_base + k) wherever e stands in the list, and everything is added at e, into
        arrays over all n_records entries: new zeroed ones, or the caller's `out` = (sum, samples, misses),
        with moments (sum, samples, misses, q, batches), which continues earlier calls as render_pixels' does.
        Returns (sum[n_records, 3] f64, samples u32, misses u32, rays), with moments (.., q f64, batches u32):
        the standard error of an entry's mean luminance follows from them (pixel_standard_error)."""
        dtype = {RT_LIST_RAYS: RAY_DTYPE, RT_LIST_BEAMS: BEAM_DTYPE, RT_LIST_SURFELS: SURFEL_DTYPE}.get(kind)
        if dtype is None:
            raise ValueError("kind must be RT_LIST_RAYS, RT_LIST_BEAMS or RT_LIST_SURFELS")
        recs = np.ascontiguousarray(records, dtype).reshape(-1)
        n = recs.shape[0]
        idx = None
        if index is not None:
            idx = np.asarray(index).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= 1 << 32):
                raise ValueError("entry numbers must lie in [0, 2^32)")
            idx = np.ascontiguousarray(idx, np.uint32)
        if out is None:
            out = (np.zeros((n, 3), np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
            if moments:
                out += (np.zeros(n, np.float64), np.zeros(n, np.uint32))
        if len(out) != (5 if moments else 3):
            raise ValueError("out must be (sum, samples, misses), with moments (sum, samples, misses, q, batches)")
        shapes = (((n, 3), np.float64), ((n,), np.uint32), ((n,), np.uint32), ((n,), np.float64), ((n,), np.uint32))
        for a, (shape, dt) in zip(out, shapes):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous arrays over the records (sum f64 [n, 3], samples, misses, "
                                 "batches u32 [n], q f64 [n])")
        s, ns, ms = out[:3]
        q = out[3].ctypes.data_as(C.POINTER(C.c_double)) if moments else None
        b = out[4].ctypes.data_as(C.POINTER(C.c_uint32)) if moments else None
        count = C.c_uint64(0)
        _check(self.lib.rt_render_list(self.handle, kind, mode, recs.ctypes.data_as(C.c_void_p), n,
                                       idx.ctypes.data_as(C.c_void_p) if idx is not None else None,
                                       n if idx is None else idx.size, spp, seed, sample_base, stream_base,
                                       s.ctypes.data_as(C.POINTER(rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       ms.ctypes.data_as(C.POINTER(C.c_uint32)), q, b, C.byref(count)))
        return (s, ns, ms, count.value) + tuple(out[3:])

    def render_list_device(self, kind: int, mode: int, d_records, n_records: int, d_index, n: int, spp: int, seed: int,
                           sample_base: int, stream_base: int, d_sum, d_samples, d_misses, d_q=0, d_batches=0,
                           plane: int = 0, d_rays=0, stream: int = 0) -> None:
        """rt_render_list_device: asynchronous render of the n entries listed (uint32 entry numbers at d_index,
        or 0: every entry, n == n_records) of the n_records records resident at d_records, into device
        accumulators of n_records elements (d_sum planes R | G | B `plane` doubles apart, 0 = n_records; d_q,
        d_batches both or 0; d_rays one uint64 ray counter or 0) on `stream`.  The device arrays as torch
        tensors or as pointers (integers)."""
        _check(self.lib.rt_render_list_device(self.handle, kind, mode, C.c_void_p(_ptr(d_records)), n_records,
                                              C.c_void_p(0 if d_index is None else _ptr(d_index)), n, spp, seed, sample_base,
                                              stream_base,
                                              C.c_void_p(_ptr(d_sum)), C.c_void_p(_ptr(d_samples)),
                                              C.c_void_p(_ptr(d_misses)), C.c_void_p(_ptr(d_q)), C.c_void_p(_ptr(d_batches)),
                                              plane, C.c_void_p(_ptr(d_rays)), C.c_void_p(stream)))

    def gather_adaptive(self, kind: int, records, rel_tol: float, min_spp: int, max_spp: int, batch_spp: int, seed: int = 0,
                        mode: int = 0, lum_floor: float = 1e-3, shape: Optional[Tuple[int, int]] = None, stream_base: int = 0,
                        sample_base: int = 0):
        """render_adaptive's loop over an array of rays, beams or surfels (`kind`, `records` and `mode` as
        render_list takes them): render until every entry's standard error is at most rel_tol of its mean
        luminance (rtcore.h, "adaptive sampling" and "indexed radiance queries"), with the records, the
        accumulators and the list held on this scene's device.  Each iteration: rt_adaptive_select_device
        over the per-entry accumulators as a frame of shape = (width, height), width * height == n_records,
        builds the list of entries that still need samples; the list's length is read (one 4-byte copy, the
        loop's only synchronisation); rt_render_list_device adds batch_spp samples of the listed entries at
        sample_base + iteration * batch_spp.  The default shape (n_records, 1) lists the entries in ascending
        order; a lightmap passes its texel grid (entry y * width + x) and gets select's 8 x 8 block order,
        neighbouring texels in one wave.  An entry's result does not depend on the order.
        The loop stops when the list is empty.  The first select names every entry (N = 0 < min_spp), so
        there is no special first pass.  Once an entry leaves the list its accumulators no longer change, so
        the rule gives the same answer for ever and it never comes back; every listed entry has therefore
        been in every earlier list and has the same N = iteration * batch_spp, which is why one sample_base
        per iteration is right.  min_spp and max_spp are rounded up to multiples of batch_spp.
        The estimate is that of sum / N with a miss counted as black: for a gather under a non-black ambient
        colour it over-estimates the error of gather_mean where an entry has misses.
        Returns render_adaptive's dict as flat device tensors of n_records: sum (3, n) f64, samples, misses,
        batches (n,) i32 (the uint32 bits), q (n,) f64, spp (n,) i64, counts, lists, rays, params."""
        import torch

        if batch_spp <= 0 or min_spp <= 0 or max_spp < min_spp:
            raise ValueError("need batch_spp > 0 and 0 < min_spp <= max_spp")
        dtype = {RT_LIST_RAYS: RAY_DTYPE, RT_LIST_BEAMS: BEAM_DTYPE, RT_LIST_SURFELS: SURFEL_DTYPE}.get(kind)
        if dtype is None:
            raise ValueError("kind must be RT_LIST_RAYS, RT_LIST_BEAMS or RT_LIST_SURFELS")
        recs = np.ascontiguousarray(records, dtype).reshape(-1)
        n = recs.shape[0]
        W, H = (n, 1) if shape is None else (int(shape[0]), int(shape[1]))
        if n == 0 or W <= 0 or H <= 0 or W * H != n:
            raise ValueError("shape = (width, height) must have width * height == n_records > 0")
        up = lambda v: -(-int(v) // batch_spp) * batch_spp  # noqa: E731
        par = rt_adaptive_params(float(rel_tol), float(lum_floor), up(min_spp), up(max_spp))
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
            acc = {"sum": torch.zeros((3, n), dtype=torch.float64, device=dev),
                   "samples": torch.zeros(n, dtype=torch.int32, device=dev),
                   "misses": torch.zeros(n, dtype=torch.int32, device=dev),
                   "q": torch.zeros(n, dtype=torch.float64, device=dev),
                   "batches": torch.zeros(n, dtype=torch.int32, device=dev)}
            d_count = torch.zeros(1, dtype=torch.int32, device=dev)
            d_rays = torch.zeros(1, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts, lists = [], []
            while True:
                lst = torch.empty(n if not counts else counts[-1], dtype=torch.int32, device=dev)
                adaptive_select_device(par, acc["sum"].data_ptr(), acc["samples"].data_ptr(), acc["misses"].data_ptr(),
                                       acc["q"].data_ptr(), acc["batches"].data_ptr(), W, H, lst.data_ptr(), lst.numel(),
                                       d_count.data_ptr(), stream=stream)
                m = int(d_count.item()) & 0xFFFFFFFF
                if m == 0:
                    break
                if m > lst.numel():
                    raise RtError("gather_adaptive: the list of active entries grew")
                lst = lst[:m]
                self.render_list_device(kind, mode, d_recs, n, lst, m, batch_spp, seed,
                                        int(sample_base) + len(counts) * batch_spp, stream_base, acc["sum"], acc["samples"],
                                        acc["misses"], acc["q"], acc["batches"], 0, d_rays, stream)
                counts.append(m)
                lists.append(lst)
            torch.cuda.synchronize(dev)
        acc["spp"] = acc["samples"].to(torch.int64) + acc["misses"].to(torch.int64)
        acc.update(counts=counts, lists=lists, rays=int(d_rays.item()), params=par)
        return acc

    def _pixel_list(self, pixels) -> np.ndarray:
        p = np.asarray(pixels)
        if p.ndim == 2 and p.shape[1] == 2:  # (x, y) pairs
            p = p[:, 1].astype(np.int64) * self.width + p[:, 0].astype(np.int64)
        p = p.reshape(-1)
        if p.size and (p.min() < 0 or p.max() >= 1 << 32):
            raise ValueError("pixel indices must lie in [0, 2^32)")
        return np.ascontiguousarray(p, np.uint32)

    def render_pixels(self, pixels, spp: int, seed: int = 0, sample_base: int = 0, out=None, moments: bool = False):
        """rt_render_pixels: spp of the camera's own samples (those a tile render draws, sample indices
        sample_base ..) for a list of frame pixels, given as frame indices y * width + x or as an (n, 2)
        array of (x, y).  Whole-frame arrays in render_tile's [x, y] shape, added to: new zeroed arrays, or
        the caller's `out` = (sum, samples, misses), with moments (sum, samples, misses, q, batches).
        Returns (sum[W,H,3] f64, samples[W,H] u32, misses[W,H] u32, rays), with moments
        (sum, samples, misses, rays, q[W,H] f64, batches[W,H] u32): the standard error of a pixel's mean
        luminance follows from them (pixel_standard_error)."""
        W, H = self.width, self.height
        px = self._pixel_list(pixels)
        if out is None:
            out = (np.zeros((W, H, 3), np.float64), np.zeros((W, H), np.uint32), np.zeros((W, H), np.uint32))
            if moments:
                out += (np.zeros((W, H), np.float64), np.zeros((W, H), np.uint32))
        if len(out) != (5 if moments else 3):
            raise ValueError("out must be (sum, samples, misses), with moments (sum, samples, misses, q, batches)")
        shapes = (((W, H, 3), np.float64), ((W, H), np.uint32), ((W, H), np.uint32), ((W, H), np.float64), ((W, H), np.uint32))
        for a, (shape, dt) in zip(out, shapes):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("out must be C-contiguous whole-frame arrays (sum f64 [W, H, 3], samples, misses, "
                                 "batches u32 [W, H], q f64 [W, H])")
        s, ns, ms = out[:3]
        q = out[3].ctypes.data_as(C.POINTER(C.c_double)) if moments else None
        b = out[4].ctypes.data_as(C.POINTER(C.c_uint32)) if moments else None
        count = C.c_uint64(0)
        _check(self.lib.rt_render_pixels(self.handle, px.ctypes.data_as(C.c_void_p), px.size, spp, seed, sample_base,
                                         s.ctypes.data_as(C.POINTER(rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         ms.ctypes.data_as(C.POINTER(C.c_uint32)), q, b, C.byref(count)))
        return (s, ns, ms, count.value) + tuple(out[3:])

    def render_pixels_device(self, d_pixels: int, n: int, spp: int, seed: int, sample_base: int, d_sum: int,
                             d_samples: int, d_misses: int, d_q: int = 0, d_batches: int = 0, plane: int = 0,
                             d_rays: int = 0, stream: int = 0) -> None:
        """rt_render_pixels_device: asynchronous render of the n frame pixels listed (uint32 frame indices) at
        device pointer d_pixels into whole-frame device accumulators in render_device's layout (index
        y * width + x; d_sum planes R | G | B `plane` doubles apart, 0 = width * height; d_q, d_batches both
        or 0; d_rays one uint64 ray counter or 0) on `stream`."""
        _check(self.lib.rt_render_pixels_device(self.handle, C.c_void_p(d_pixels), n, spp, seed, sample_base,
                                                C.c_void_p(d_sum), C.c_void_p(d_samples), C.c_void_p(d_misses),
                                                C.c_void_p(d_q), C.c_void_p(d_batches), plane, C.c_void_p(d_rays),
                                                C.c_void_p(stream)))

    def render_adaptive(self, rel_tol: float, min_spp: int, max_spp: int, batch_spp: int, seed: int = 0,
                        lum_floor: float = 1e-3, history: Optional[dict] = None, sample_base: int = 0):
        """Render until every pixel's standard error is at most rel_tol of its luminance (rtcore.h, "adaptive
        sampling"), with the accumulators and the pixel list held as torch tensors on this scene's device.
        Each iteration: rt_adaptive_select_device builds the list of pixels that still need samples, the
        list's length is read (one 4-byte copy, the loop's only synchronisation), and
        rt_render_pixels_device adds batch_spp samples of the listed pixels at
        sample_base = iteration * batch_spp.  The loop stops when the list is empty.  The first select names
        every pixel (N = 0 < min_spp), so there is no special first pass.  Once a pixel leaves the list its
        accumulators no longer change, so the rule gives the same answer for ever and it never comes back;
        every listed pixel has therefore been in every earlier list and has the same N = iteration *
        batch_spp, which is why one sample_base per iteration is right.  min_spp and max_spp are rounded up
        to multiples of batch_spp.
        history: a dict with sum, samples, misses, q, batches in this method's own layout (reproject's
        result): the loop starts from clones of them instead of from zeros, so the caller's tensors are
        untouched.  The listed pixels then no longer share one N -- a carried pixel starts with up to
        max_history samples, an empty one with none -- but the stop argument still holds: a pixel that
        leaves the list never changes again, so the lists only shrink and the loop ends at the latest when
        every pixel has max_spp.  Iteration i draws at sample_base + i * batch_spp; the caller gives each
        frame its own sample_base range (or its own seed), so that a pixel that maps to itself does not
        draw the stream twice that its history already holds.  With both left out the result is bit for bit
        what it was without them.
        Returns a dict: sum (3, H, W) f64, samples, misses, batches (H, W) i32 (the uint32 bits), q (H, W) f64
        -- device tensors in render_device's layout -- spp (H, W) i64 = samples + misses, counts (the list
        sizes per iteration), lists (the lists themselves, device tensors), rays, params."""
        import torch

        if batch_spp <= 0 or min_spp <= 0 or max_spp < min_spp:
            raise ValueError("need batch_spp > 0 and 0 < min_spp <= max_spp")
        up = lambda v: -(-int(v) // batch_spp) * batch_spp  # noqa: E731
        par = rt_adaptive_params(float(rel_tol), float(lum_floor), up(min_spp), up(max_spp))
        W, H = self.width, self.height
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            acc = {"sum": torch.zeros((3, H, W), dtype=torch.float64, device=dev),
                   "samples": torch.zeros((H, W), dtype=torch.int32, device=dev),
                   "misses": torch.zeros((H, W), dtype=torch.int32, device=dev),
                   "q": torch.zeros((H, W), dtype=torch.float64, device=dev),
                   "batches": torch.zeros((H, W), dtype=torch.int32, device=dev)}
            if history is not None:
                for k, z in acc.items():
                    t = history[k]
                    if t.shape != z.shape or t.dtype != z.dtype or t.device != z.device:
                        raise ValueError(f"render_adaptive: history[{k!r}] is not a {tuple(z.shape)} {z.dtype} tensor on {dev}")
                    acc[k] = t.clone(memory_format=torch.contiguous_format)
            d_count = torch.zeros(1, dtype=torch.int32, device=dev)
            d_rays = torch.zeros(1, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts, lists = [], []
            while True:
                lst = torch.empty(W * H if not counts else counts[-1], dtype=torch.int32, device=dev)
                adaptive_select_device(par, acc["sum"].data_ptr(), acc["samples"].data_ptr(), acc["misses"].data_ptr(),
                                       acc["q"].data_ptr(), acc["batches"].data_ptr(), W, H, lst.data_ptr(), lst.numel(),
                                       d_count.data_ptr(), stream=stream)
                n = int(d_count.item()) & 0xFFFFFFFF
                if n == 0:
                    break
                if n > lst.numel():
                    raise RtError("render_adaptive: the list of active pixels grew")
                lst = lst[:n]
                self.render_pixels_device(lst.data_ptr(), n, batch_spp, seed, int(sample_base) + len(counts) * batch_spp,
                                          acc["sum"].data_ptr(), acc["samples"].data_ptr(), acc["misses"].data_ptr(),
                                          acc["q"].data_ptr(), acc["batches"].data_ptr(), 0, d_rays.data_ptr(), stream)
                counts.append(n)
                lists.append(lst)
            torch.cuda.synchronize(dev)
        acc["spp"] = acc["samples"].to(torch.int64) + acc["misses"].to(torch.int64)
        acc.update(counts=counts, lists=lists, rays=int(d_rays.item()), params=par)
        return acc

    def primary_hits_device(self, d_hits: int, x0: int = 0, y0: int = 0, w: Optional[int] = None, h: Optional[int] = None,
                            stream: int = 0) -> None:
        """rt_primary_hits_device: the fast first hit of every pixel centre of the tile into w * h rt_hit at
        device pointer d_hits, row-major (y * w + x): what query_rays answers for camera_rays of the tile,
        the rays made on the device.  Asynchronous on `stream`."""
        w = self.width - x0 if w is None else w
        h = self.height - y0 if h is None else h
        _check(self.lib.rt_primary_hits_device(self.handle, x0, y0, w, h, C.c_void_p(d_hits), C.c_void_p(stream)))

    def primary_hits(self):
        """The whole frame's first hits under the scene's current camera (rt_primary_hits_device on torch's
        current stream, waited for): a (H * W, 48) uint8 device tensor of rt_hit records, row-major, which
        denoise and reproject take as `hits`; .cpu().numpy().reshape(-1).view(HIT_DTYPE) reads it."""
        import torch

        W, H = self.width, self.height
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            hits = torch.empty((H * W, HIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            self.primary_hits_device(hits.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
        return hits

    def _check_hits(self, hits, name: str) -> None:
        import torch

        if (hits.dtype != torch.uint8 or hits.numel() != self.width * self.height * HIT_DTYPE.itemsize or
                not hits.is_contiguous() or hits.device != torch.device("cuda", self.device)):
            raise ValueError(f"{name}: not primary_hits' tensor for this frame and device")

    def reproject(self, res: dict, prev_camera: rt_camera, prev_hits, hits=None, **params):
        """Temporal reprojection (rtcore.h, "temporal reprojection"): the accumulators of `res`,
        render_adaptive's result under prev_camera, carried to the pixels of the scene's camera, which is
        already the new one.  prev_hits: primary_hits() taken under prev_camera; hits: primary_hits() under
        the current camera (made here when None).  params: the fields of rt_reproject_params
        (REPROJECT_DEFAULTS for the rest).  One rt_reproject_device call on torch's current stream.
        Returns a dict: sum, samples, misses, q, batches in render_adaptive's layout -- its `history`
        argument takes the dict as it is --, src (H, W) i32, the source pixel's frame index or -1 for a
        pixel that starts again, and hits, the current camera's, for denoise(..., hits=)."""
        import torch

        W, H = self.width, self.height
        par = reproject_params(**params)
        dev = torch.device("cuda", self.device)
        if hits is None:
            hits = self.primary_hits()
        self._check_hits(prev_hits, "reproject: prev_hits")
        self._check_hits(hits, "reproject: hits")
        src_t = {}
        for k, shape, dt in (("sum", (3, H, W), torch.float64), ("samples", (H, W), torch.int32), ("misses", (H, W), torch.int32),
                             ("q", (H, W), torch.float64), ("batches", (H, W), torch.int32)):
            t = res[k]
            if tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
                raise ValueError(f"reproject: res[{k!r}] is not a {shape} {dt} tensor on {dev}")
            src_t[k] = t.contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = {"sum": torch.empty((3, H, W), dtype=torch.float64, device=dev),
                   "samples": torch.empty((H, W), dtype=torch.int32, device=dev),
                   "misses": torch.empty((H, W), dtype=torch.int32, device=dev),
                   "q": torch.empty((H, W), dtype=torch.float64, device=dev),
                   "batches": torch.empty((H, W), dtype=torch.int32, device=dev),
                   "src": torch.empty((H, W), dtype=torch.int32, device=dev)}
            reproject_device(par, prev_camera, prev_hits.data_ptr(), hits.data_ptr(), src_t["sum"].data_ptr(),
                             src_t["samples"].data_ptr(), src_t["misses"].data_ptr(), src_t["q"].data_ptr(),
                             src_t["batches"].data_ptr(), W, H, out["sum"].data_ptr(), out["samples"].data_ptr(),
                             out["misses"].data_ptr(), out["q"].data_ptr(), out["batches"].data_ptr(), out["src"].data_ptr(),
                             stream=stream)
            torch.cuda.synchronize(dev)  # (the inputs' contiguous copies, if any, are released on return)
        out["hits"] = hits
        out["params"] = par
        return out

    def denoise(self, res: dict, return_var: bool = False, hits=None, **params):
        """The a-trous filter (rtcore.h, "denoising") over render_adaptive's result `res`: one
        rt_primary_hits_device pass for the frame's guides, then rt_denoise_device, on torch's current
        stream.  hits: primary_hits() of the scene's camera (reproject's result has it), so that a frame's
        guide pass runs once; None: the pass runs here into a private tensor.  params: the fields of
        rt_denoise_params (DENOISE_DEFAULTS for the rest, and
        denoise_iterations of the frame for the levels).  Returns the filtered sums as a (3, H, W) f64 device
        tensor in res["sum"]'s layout -- tonemap_device takes it with res["samples"] and res["misses"] -- and
        with return_var also the filtered variance, (H, W) f32."""
        import torch

        W, H = self.width, self.height
        params.setdefault("iterations", denoise_iterations(W, H))
        par = denoise_params(**params)
        dev = torch.device("cuda", self.device)
        if hits is not None:
            self._check_hits(hits, "denoise: hits")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((3, H, W), dtype=torch.float64, device=dev)
            var = torch.empty((H, W), dtype=torch.float32, device=dev) if return_var else None
            if hits is None:
                hits = torch.empty((H * W, HIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                self.primary_hits_device(hits.data_ptr(), stream=stream)
            denoise_device(par, res["sum"].data_ptr(), res["samples"].data_ptr(), res["misses"].data_ptr(),
                           res["q"].data_ptr(), res["batches"].data_ptr(), hits.data_ptr(), W, H, out.data_ptr(),
                           var.data_ptr() if return_var else 0, stream=stream)
            torch.cuda.synchronize(dev)  # (hits is released on return)
        return (out, var) if return_var else out

    def select_pixels(self, items, x0: int = 0, y0: int = 0, w: Optional[int] = None,
                      h: Optional[int] = None) -> np.ndarray:
        """rt_select_pixels (DebugRaycaster Selection mode): per pixel of the tile, which item of the list
        -- (kind, index) pairs, RT_SELECT_PRIM with a Primitive.ID or RT_SELECT_NODE with a reference-BVH
        node's pre-order index -- the primary ray meets nearest, the later of two at equal distances.
        Returns a SELECTION_DTYPE array indexed [x, y]; item -1 where nothing is met."""
        w = self.width - x0 if w is None else w
        h = self.height - y0 if h is None else h
        it = _pack_items(items)
        out = np.zeros((max(w, 0), max(h, 0)), SELECTION_DTYPE)
        _check(self.lib.rt_select_pixels(self.handle, it.ctypes.data_as(C.c_void_p), it.size, x0, y0, w, h,
                                         out.ctypes.data_as(C.c_void_p)))
        return out

    def select_pixels_device(self, items, x0: int, y0: int, w: int, h: int, d_out: int, stream: int = 0) -> None:
        """rt_select_pixels_device: asynchronous selection pass over the tile into w*h rt_selection at device
        pointer d_out, row-major (y*w + x), on `stream` (a hipStream_t as an integer, 0 = the default stream)."""
        it = _pack_items(items)
        _check(self.lib.rt_select_pixels_device(self.handle, it.ctypes.data_as(C.c_void_p), it.size, x0, y0, w, h,
                                                C.c_void_p(d_out), C.c_void_p(stream)))

    def select_rays(self, items, origins, directions=None) -> np.ndarray:
        """rt_select_rays: the selection fold for the caller's rays (given as for query_rays).  Returns a
        SELECTION_DTYPE array of the rays' shape; item -1 where nothing is met or the ray is invalid."""
        it = _pack_items(items)
        rays = _rays_arg(origins, directions)
        out = np.zeros(rays.shape, SELECTION_DTYPE)
        _check(self.lib.rt_select_rays(self.handle, it.ctypes.data_as(C.c_void_p), it.size,
                                       rays.ctypes.data_as(C.c_void_p), rays.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def select_rays_device(self, items, d_rays: int, n: int, d_out: int, stream: int = 0) -> None:
        """rt_select_rays_device: asynchronous selection of n rt_ray at device pointer d_rays into n
        rt_selection at d_out on `stream`; `items` is a host list, copied to the device by the call."""
        it = _pack_items(items)
        _check(self.lib.rt_select_rays_device(self.handle, it.ctypes.data_as(C.c_void_p), it.size, C.c_void_p(d_rays),
                                              n, C.c_void_p(d_out), C.c_void_p(stream)))

    def camera_rays(self, x0: int = 0, y0: int = 0, w: Optional[int] = None, h: Optional[int] = None) -> np.ndarray:
        """camera_rays for this scene's camera and frame size."""
        return camera_rays(self.camera, (self.width, self.height), x0, y0, w, h)

    def render_device(self, x0, y0, w, h, spp, seed, sample_base, d_sum, d_samples, d_misses, d_rays,
                      stream: int = 0) -> None:
        """Asynchronous device-resident render; d_* are device pointers (e.g. torch data_ptr())."""
        _check(self.lib.rt_render_device(self.handle, x0, y0, w, h, spp, seed, sample_base,
                                         C.c_void_p(d_sum), C.c_void_p(d_samples), C.c_void_p(d_misses),
                                         C.c_void_p(d_rays), C.c_void_p(stream)))

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        _check(self.lib.rt_last_kernel_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    KERNEL_TIME_RING = 64

    def kernel_times(self, n: int) -> List[float]:
        """rt_kernel_times: durations (ms) of the last n path kernels on this scene, oldest first
        (n <= 64): launches queued without a host sync, timed afterwards."""
        out = (C.c_float * max(n, 1))()
        _check(self.lib.rt_kernel_times(self.handle, n, out))
        return [float(v) for v in out[:n]]

    def kernel_times_raw(self, n: int) -> List[float]:
        """rt_debug_kernel_times_raw: the same n entries as their raw event pairs (end - start)."""
        out = (C.c_float * max(n, 1))()
        _check(self.lib.rt_debug_kernel_times_raw(self.handle, n, out))
        return [float(v) for v in out[:n]]

    STAT_NAMES = ("node_visits", "tri_tests", "sph_tests", "cyc_start", "cyc_trace", "cyc_shade", "wave_iters",
                  "max_query_steps", "stack_overflow_pushes", "max_stack_depth", "outer_tests")

    def set_stats(self, enable: bool) -> None:
        """rt_scene_set_stats: run the instrumented kernel variant (profiling only)."""
        _check(self.lib.rt_scene_set_stats(self.handle, 1 if enable else 0))

    def get_stats(self) -> dict:
        """rt_scene_get_stats: counters accumulated since the last read (then zeroed)."""
        out = (C.c_uint64 * len(self.STAT_NAMES))()
        _check(self.lib.rt_scene_get_stats(self.handle, out, len(self.STAT_NAMES)))
        return dict(zip(self.STAT_NAMES, (int(v) for v in out)))


def tonemap_device(d_sum: int, d_samples: int, d_misses: int, w: int, h: int, d_argb: int,
                   background=(0.0, 0.0, 0.0), background_alpha: float = 0.0, exposure: float = 1.0,
                   stream: int = 0) -> None:
    """rt_tonemap_device: SampleSet.GetOutput for every pixel of device accumulators (pointers)."""
    _check(load_library().rt_tonemap_device(d_sum, d_samples, d_misses, w, h, rt_color(*background),
                                            background_alpha, exposure, d_argb, stream))


def adaptive_select_device(params: rt_adaptive_params, d_sum: int, d_samples: int, d_misses: int, d_q: int,
                           d_batches: int, width: int, height: int, d_pixels: int, cap: int, d_count: int,
                           plane: int = 0, stream: int = 0) -> None:
    """rt_adaptive_select_device: from whole-frame device accumulators (render_pixels_device's layout) the
    compacted list of active pixels' frame indices into d_pixels (at most cap), their number into the
    uint32 at d_count; 8x8 block order.  Works on the current device; asynchronous on `stream`."""
    _check(load_library().rt_adaptive_select_device(C.byref(params), d_sum, d_samples, d_misses, d_q, d_batches, plane,
                                                    width, height, d_pixels, cap, d_count, stream))


def adaptive_select_host(params: rt_adaptive_params, sum_planes: np.ndarray, samples: np.ndarray, misses: np.ndarray,
                         q: np.ndarray, batches: np.ndarray, width: int, height: int, cap: Optional[int] = None,
                         plane: int = 0) -> Tuple[np.ndarray, int]:
    """rt_debug_adaptive_select, the host twin of adaptive_select_device (no GPU): host arrays in the device
    layout (sum: three planes `plane` doubles apart, 0 = width * height; the others row-major y * width +
    x).  Returns (the first min(count, cap) list entries, count)."""
    npix = width * height
    pl = plane or npix
    s = np.ascontiguousarray(sum_planes, np.float64).reshape(-1)
    arrs = [np.ascontiguousarray(a, dt).reshape(-1) for a, dt in
            ((samples, np.uint32), (misses, np.uint32), (q, np.float64), (batches, np.uint32))]
    if s.size < 2 * pl + npix or any(a.size < npix for a in arrs):
        raise ValueError("accumulator arrays smaller than the frame")
    cap = npix if cap is None else int(cap)
    out = np.zeros(max(cap, 1), np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = load_library().rt_debug_adaptive_select(C.byref(params), ptr(s), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]),
                                                ptr(arrs[3]), plane, width, height, ptr(out), cap)
    if n < 0:
        _check(int(n))
    return out[:min(int(n), cap)].copy(), int(n)


def denoise_device(params: rt_denoise_params, d_sum: int, d_samples: int, d_misses: int, d_q: int, d_batches: int,
                   d_hits: int, width: int, height: int, d_out_sum: int, d_out_var: int = 0, plane: int = 0,
                   stream: int = 0) -> None:
    """rt_denoise_device: the a-trous filter over whole-frame device accumulators with moments
    (render_pixels_device's layout) and the frame's first hits (primary_hits_device), into d_out_sum (d_sum's
    layout, not overlapping it) and, unless 0, width * height floats of filtered variance at d_out_var.
    Works on the current device; asynchronous on `stream`."""
    _check(load_library().rt_denoise_device(C.byref(params), d_sum, d_samples, d_misses, d_q, d_batches, plane, d_hits,
                                            width, height, d_out_sum, d_out_var or None, stream))


def denoise_host(params: rt_denoise_params, sum_planes: np.ndarray, samples: np.ndarray, misses: np.ndarray,
                 q: np.ndarray, batches: np.ndarray, hits: np.ndarray, width: int, height: int,
                 plane: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """rt_debug_denoise, the host twin of denoise_device (no GPU): host arrays in the device layout (sum: three
    planes `plane` doubles apart, 0 = width * height; the others and hits, a HIT_DTYPE array, row-major
    y * width + x).  Returns (out_sum, a flat f64 array of sum's size whose bytes outside the three planes
    are 0, and out_var, f32 (height, width))."""
    npix = width * height
    pl = plane or npix
    s = np.ascontiguousarray(sum_planes, np.float64).reshape(-1)
    arrs = [np.ascontiguousarray(a, dt).reshape(-1) for a, dt in
            ((samples, np.uint32), (misses, np.uint32), (q, np.float64), (batches, np.uint32), (hits, HIT_DTYPE))]
    if pl < npix or s.size < 2 * pl + npix or any(a.size < npix for a in arrs):
        raise ValueError("accumulator arrays smaller than the frame")
    out = np.zeros(s.size, np.float64)
    var = np.zeros((height, width), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(load_library().rt_debug_denoise(C.byref(params), ptr(s), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]),
                                           plane, ptr(arrs[4]), width, height, ptr(out), ptr(var)))
    return out, var


def reproject_device(params: rt_reproject_params, prev_camera: rt_camera, d_prev_hits: int, d_hits: int, d_sum: int,
                     d_samples: int, d_misses: int, d_q: int, d_batches: int, width: int, height: int, d_out_sum: int,
                     d_out_samples: int, d_out_misses: int, d_out_q: int, d_out_batches: int, d_out_src: int = 0,
                     plane: int = 0, stream: int = 0) -> None:
    """rt_reproject_device: whole-frame device accumulators with moments (render_pixels_device's layout) under
    prev_camera, carried to the pixels of the camera whose first hits are at d_hits (d_prev_hits: the first
    hits under prev_camera; both from primary_hits_device), into the d_out_* arrays of the same layout, which
    overlap no input, and, unless 0, width * height int32 source indices at d_out_src.  Works on the current
    device; asynchronous on `stream`."""
    _check(load_library().rt_reproject_device(C.byref(params), C.byref(prev_camera), d_prev_hits, d_hits, d_sum, d_samples,
                                              d_misses, d_q, d_batches, plane, width, height, d_out_sum, d_out_samples,
                                              d_out_misses, d_out_q, d_out_batches, d_out_src or None, stream or None))


def reproject_host(params: rt_reproject_params, prev_camera: rt_camera, prev_hits: np.ndarray, hits: np.ndarray,
                   sum_planes: np.ndarray, samples: np.ndarray, misses: np.ndarray, q: np.ndarray, batches: np.ndarray,
                   width: int, height: int, plane: int = 0, fill: float = 0.0) -> dict:
    """rt_debug_reproject, the host twin of reproject_device (no GPU): host arrays in the device layout (sum:
    three planes `plane` doubles apart, 0 = width * height; the others and the hits, HIT_DTYPE arrays,
    row-major y * width + x).  Returns a dict: sum, a flat f64 array of sum_planes' size whose elements
    outside the three planes keep `fill`, samples, misses, batches u32 and q f64 (height, width), and src
    i32 (height, width)."""
    npix = width * height
    pl = plane or npix
    s = np.ascontiguousarray(sum_planes, np.float64).reshape(-1)
    arrs = [np.ascontiguousarray(a, dt).reshape(-1) for a, dt in
            ((samples, np.uint32), (misses, np.uint32), (q, np.float64), (batches, np.uint32), (prev_hits, HIT_DTYPE),
             (hits, HIT_DTYPE))]
    if pl < npix or s.size < 2 * pl + npix or any(a.size < npix for a in arrs):
        raise ValueError("accumulator arrays smaller than the frame")
    out = {"sum": np.full(s.size, fill, np.float64), "samples": np.zeros((height, width), np.uint32),
           "misses": np.zeros((height, width), np.uint32), "q": np.zeros((height, width), np.float64),
           "batches": np.zeros((height, width), np.uint32), "src": np.zeros((height, width), np.int32)}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(load_library().rt_debug_reproject(C.byref(params), C.byref(prev_camera), ptr(arrs[4]), ptr(arrs[5]), ptr(s),
                                             ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), plane, width, height,
                                             ptr(out["sum"]), ptr(out["samples"]), ptr(out["misses"]), ptr(out["q"]),
                                             ptr(out["batches"]), ptr(out["src"])))
    return out


def pixels_plan(kernel: int, n: int, spp: int) -> dict:
    """rt_debug_pixels_plan (host code, no GPU): how rt_render_pixels plans n list entries at spp for
    kernel 0 (BRUTE), 1 (GROUPED) or 3 (BVH)."""
    info = (C.c_int32 * 4)()
    _check(load_library().rt_debug_pixels_plan(kernel, n, spp, info))
    return dict(zip(("n_chunks", "samples_per_item", "used_chunks", "blocks"), (int(v) for v in info)))


def pixel_standard_error(sum_rgb: np.ndarray, samples: np.ndarray, misses: np.ndarray, q: np.ndarray,
                         batches: np.ndarray) -> np.ndarray:
    """The standard error of each pixel's mean luminance from accumulators with moments (rtcore.h's
    estimate); sum_rgb has the colour as its last axis.  inf where fewer than two batches were taken.
    It serves render_list's per-entry accumulators as they are (sum [n, 3]; gather_adaptive's planar sum
    as sum.T): an entry is a pixel of a frame of n_records."""
    n = samples.astype(np.float64) + misses.astype(np.float64)
    y = 0.299 * sum_rgb[..., 0] + 0.587 * sum_rgb[..., 1] + 0.114 * sum_rgb[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.maximum(0.0, (q - y * y / n) / (batches.astype(np.float64) - 1.0))
        se = np.sqrt(var / n)
    return np.where(batches >= 2, se, np.inf)


def _frame_inputs(scene: ParsedScene, camera_index: int, size: Optional[Tuple[int, int]]):
    params = rt_scene_params.from_buffer_copy(scene.params)
    if size is not None:
        params.width, params.height = size
    prims = (rt_prim * max(1, scene.n_prims))(*scene.prims)
    cam = rt_camera.from_buffer_copy(scene.cameras[camera_index])
    return params, prims, cam


class GpuFrame:
    """rt_frame: persistent whole-frame renderer over devices 0..n_gpus-1 of this process (row-band
    split, one RCCL gather to device 0 per render).  Replaces FullRaytracer's worker pool
    (FullRaytracer.cs:297-302) on a multi-GPU host; accumulators in the [x, y] order of SampleSet[w, h]."""

    def __init__(self, scene: ParsedScene, camera_index: int = 0, n_gpus: int = 1,
                 size: Optional[Tuple[int, int]] = None):
        self.lib = load_library()
        params, prims, cam = _frame_inputs(scene, camera_index, size)
        self.width, self.height = params.width, params.height
        self.handle = C.c_void_p()
        _check(self.lib.rt_frame_create(C.byref(params), prims, scene.n_prims, C.byref(cam), n_gpus,
                                        C.byref(self.handle)))

    def set_camera(self, camera: rt_camera) -> None:
        _check(self.lib.rt_frame_set_camera(self.handle, C.byref(camera)))

    def render(self, spp: int, seed: int = 0, sample_base: int = 0, out=None):
        """Adds spp samples of every pixel into (sum[W,H,3], samples[W,H], misses[W,H]) (new if out is None)."""
        W, H = self.width, self.height
        if out is None:
            out = (np.zeros((W, H, 3), np.float64), np.zeros((W, H), np.uint32), np.zeros((W, H), np.uint32))
        s, n, m = self._check_out(out)
        rays = C.c_uint64(0)
        _check(self.lib.rt_frame_render(self.handle, spp, seed, sample_base, s.ctypes.data_as(C.POINTER(rt_color)),
                                        n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        m.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rays)))
        return s, n, m, rays.value

    def submit(self, spp: int, seed: int = 0, sample_base: int = 0) -> None:
        """rt_frame_submit: queue a render (band sets, gather, host copy) and return at once."""
        _check(self.lib.rt_frame_submit(self.handle, spp, seed, sample_base))

    def collect(self, out):
        """rt_frame_collect: wait for the oldest submitted render and add it into out = (sum[W,H,3],
        samples[W,H], misses[W,H]); returns (sum, samples, misses, rays)."""
        s, n, m = self._check_out(out)
        rays = C.c_uint64(0)
        _check(self.lib.rt_frame_collect(self.handle, s.ctypes.data_as(C.POINTER(rt_color)),
                                         n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         m.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rays)))
        return s, n, m, rays.value

    def inject_fault(self, point: int) -> None:
        """rt_frame_inject_fault (test hook): 1 = the next gather fails inside its RCCL group."""
        _check(self.lib.rt_frame_inject_fault(self.handle, point))

    def _check_out(self, out):
        W, H = self.width, self.height
        s, n, m = out
        for a, dt, shape in ((s, np.float64, (W, H, 3)), (n, np.uint32, (W, H)), (m, np.uint32, (W, H))):
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous):
                raise ValueError(f"GpuFrame: outputs must be C-contiguous {np.dtype(dt).name}{shape} arrays")
        return s, n, m

    def close(self) -> None:
        if self.handle:
            self.lib.rt_frame_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def band_rows_count(height: int, band: int, band_stride: int, band_offset: int) -> int:
    """rt_band_rows: rows of band set (band, band_stride, band_offset) of a frame (host only)."""
    n = load_library().rt_band_rows(height, band, band_stride, band_offset)
    _check(min(n, 0))
    return n


def band_slot_rows(height: int, band: int, band_stride: int) -> int:
    """rt_band_slot_rows: rows of the tallest band set of the split (host only)."""
    n = load_library().rt_band_slot_rows(height, band, band_stride)
    _check(min(n, 0))
    return n


def scatter_band_slot(slot: np.ndarray, plane: int, width: int, height: int, band: int, band_stride: int,
                      band_offset: int, out) -> None:
    """rt_scatter_band_slot (host only): rt_frame_render's merge of one device's gathered slot (a
    float64 array of 4 * plane: sum planes, then the samples / misses u32 planes) into
    (sum[W,H,3], samples[W,H], misses[W,H])."""
    s, n, m = out
    slot = np.ascontiguousarray(slot, dtype=np.float64)
    # the C side writes through raw pointers: refuse anything but the exact layouts it assumes
    for a, dt, shape in ((s, np.float64, (width, height, 3)), (n, np.uint32, (width, height)),
                         (m, np.uint32, (width, height))):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous
                and a.flags.writeable):
            raise ValueError(f"scatter_band_slot: outputs must be writeable C-contiguous {np.dtype(dt).name}"
                             f"{shape} arrays")
    if plane < 0 or slot.size < 4 * plane:
        raise ValueError(f"scatter_band_slot: slot holds {slot.size} float64, needs 4 * plane = {4 * plane}")
    _check(load_library().rt_scatter_band_slot(slot.ctypes.data_as(C.c_void_p), plane, width, height, band,
                                               band_stride, band_offset, s.ctypes.data_as(C.POINTER(rt_color)),
                                               n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               m.ctypes.data_as(C.POINTER(C.c_uint32))))


def render_frame_multi(scene: ParsedScene, camera_index: int, n_gpus: int, spp: int, seed: int = 0,
                       size: Optional[Tuple[int, int]] = None, sample_base: int = 0):
    """rt_render_frame_multi: row-interleaved bands on n_gpus devices + RCCL gather (one shot)."""
    lib = load_library()
    params, prims, cam = _frame_inputs(scene, camera_index, size)
    W, H = params.width, params.height
    s = np.zeros((W, H, 3), np.float64)
    n = np.zeros((W, H), np.uint32)
    m = np.zeros((W, H), np.uint32)
    rays = C.c_uint64(0)
    _check(lib.rt_render_frame_multi(C.byref(params), prims, scene.n_prims, C.byref(cam), n_gpus, spp, seed,
                                     sample_base, s.ctypes.data_as(C.POINTER(rt_color)),
                                     n.ctypes.data_as(C.POINTER(C.c_uint32)), m.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     C.byref(rays)))
    return s, n, m, rays.value


def scene_path(name: str) -> str:
    """Path of a scene fixture shipped in tests/golden/scenes (bounce.txt, die.txt, ...)."""
    return os.path.join(REPO_ROOT, "tests", "golden", "scenes", name)
