"""ctypes binding of tyrant_amd/lib/libtyrant_hip.so (the C ABI of include/tyr_c.h).

This is glue for the tests and bench.py; the product is the shared library.  There is
no fallback: if the library is missing or no HIP device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import scenes

_HERE = os.path.dirname(os.path.abspath(__file__))
# TYRANT_HIP_LIBRARY: load another build of the same ABI (diagnostic builds made by tools/*.sh); never a CPU path
LIB_PATH = os.environ.get("TYRANT_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libtyrant_hip.so")

TYR_FLAG_TRIANGLE_MATERIALS = 1
TYR_FLAG_PROFILE = 2
TYR_FLAG_COUNT_VISITS = 4
TYR_FLAG_LIGHT_LIST = 8
TYR_FLAG_TRIANGLE_COLORS = 16
TYR_FLAG_DEBUG_BVH = 32
TYR_FLAG_REFIT = 64
TYR_FLAG_WINDING = 128
TYR_ERR_INVALID = -1
TYR_ERR_NO_DEVICE = -2
TYR_ERR_NO_SCENE = -3
TYR_ERR_DEVICE = -6
TYR_ERR_UNSUPPORTED = -7
TYR_QUERY_SPHERES = 1
TYR_QUERY_TWO_SIDED = 2  # tyr_query_hits only
TYR_QUERY_HITS_MAX = 32
TYR_QUERY_BOX_ANY = 4  # tyr_query_box only
TYR_QUERY_BOX_MAX = 32
TYR_QUERY_TRI_ANY = 4  # tyr_query_tri only
TYR_QUERY_TRI_SKIP_SHARED = 8  # tyr_query_tri and tyr_query_tri_distance
TYR_QUERY_TRI_MAX = 32
TYR_QUERY_NEAREST_K_MAX = 32
TYR_QUERY_OCCLUSION_MAX_SAMPLES = 1024
AOV_CHAIN_MAX = 8  # TYR_AOV_CHAIN_MAX
TYR_REFIT_DEVICE = 1
TYR_DENOISE_RESOLVE = 1
# tyr_denoise's defaults (host/denoise.cpp)
DENOISE_PASSES, DENOISE_SIGMA_COLOR, DENOISE_SIGMA_DEPTH, DENOISE_NORMAL_POWER_LOG2 = 5, 32.0, 0.02, 7
TYR_TEMPORAL_RESET = 1
# tyr_temporal's defaults (host/temporal.cpp)
TEMPORAL_MAX_HISTORY, TEMPORAL_DEPTH_TOLERANCE, TEMPORAL_NORMAL_COS = 16, 0.05, 0.9
TYR_SVGF_RESET, TYR_SVGF_RESOLVE = 1, 2
# tyr_svgf's defaults (host/svgf.cpp)
SVGF_MAX_HISTORY, SVGF_DEPTH_TOLERANCE, SVGF_NORMAL_COS = 8, 0.05, 0.9
SVGF_PASSES, SVGF_SIGMA_LUMINANCE, SVGF_SIGMA_DEPTH, SVGF_NORMAL_POWER_LOG2 = 3, 2.0, 0.02, 7
TYR_TAA_RESET, TYR_TAA_BILINEAR = 1, 2
# tyr_taa's defaults (host/taa.cpp; DESIGN.md "Temporal anti-aliasing", profiles/taa_bench_c3.json)
TAA_ALPHA, TAA_GAMMA = 0.2, 1.5
# Renderer.allocate_samples' defaults (DESIGN.md "Adaptive sampling", profiles/adaptive_bench_c3.json): every pixel keeps one
# sample (the AOV / motion rays stay sample 0), and no pixel takes more than this many
ADAPTIVE_MIN_SPP, ADAPTIVE_MAX_SPP = 1, 256
TYR_DIST_GATHER, TYR_DIST_REDUCE = 0, 1
TYR_DIST_ID_BYTES = 128
KERNEL_NAMES = ("primary", "extend", "shade", "connect", "resolve")

c_f, c_u32, c_u64, c_i32, P = C.c_float, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p


class TyrError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: status {status} ({status_string(status)})")


class Config(C.Structure):
    _fields_ = [
        ("width", c_u32),
        ("height", c_u32),
        ("queue_size", c_u32),
        ("device", c_i32),
        ("rank", c_u32),
        ("nranks", c_u32),
        ("flags", c_u32),
        ("stream", P),
    ]


class CameraC(C.Structure):
    _fields_ = [("position", c_f * 3), ("direction", c_f * 3), ("up", c_f * 3), ("focalDistance", c_f), ("lensRadius", c_f)]


class Counters(C.Structure):
    _fields_ = [
        ("primary_ray_cnt", c_u32),
        ("start_position", c_u32),
        ("shadow_ray_cnt", c_u32),
        ("n_live", c_u32),
        ("frame", c_u32),
        ("device_error", c_u32),
        ("budget_remaining", c_u64),
        ("total_extend_rays", c_u64),
        ("total_shadow_rays", c_u64),
        ("total_primary_rays", c_u64),
        ("nodes_extend", c_u64),
        ("tris_extend", c_u64),
        ("nodes_connect", c_u64),
        ("tris_connect", c_u64),
        ("n_survive", c_u64),
        ("n_shadow_visible", c_u64),
        ("rays_in_tree_extend", c_u64),
        ("rays_in_tree_connect", c_u64),
        ("debug", c_u64 * 16),
    ]

    def asdict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "debug"}
        d["debug"] = [int(x) for x in self.debug]
        return d


class SceneInfo(C.Structure):
    _fields_ = [("n_prims", c_u32), ("n_pair_nodes", c_u32), ("n_quad_nodes", c_u32), ("n_staged_nodes", c_u32), ("n_lights", c_u32), ("max_quad_nodes", c_u32), ("max_prim_offset", c_u32),
                ("quad_max_stack", c_u32), ("device_bytes", c_u64), ("upload_layout_s", C.c_double), ("upload_copy_s", C.c_double), ("layout_on_device", c_u32), ("reserved_", c_u32)]


class LayoutStats(C.Structure):
    _fields_ = [("n_pair_nodes", c_u32), ("n_quad_nodes", c_u32), ("n_staged_nodes", c_u32), ("quad_max_stack", c_u32), ("root_ref", c_u32), ("quad_root_ref", c_u32),
                ("hash_pairs", c_u64), ("hash_quads", c_u64), ("hash_tris", c_u64), ("seconds", C.c_double)]


class AovOut(C.Structure):
    """tyr_aov_out: device pointers of the AOV buffers, NULL to skip one"""

    _fields_ = [("albedo", P), ("normal", P), ("depth", P), ("prim", P), ("geom", P)]


class NearestOut(C.Structure):
    """tyr_nearest_out: device pointers of tyr_query_nearest's outputs; uv, region, point may be NULL"""

    _fields_ = [("dist2", P), ("prim", P), ("uv", P), ("region", P), ("point", P)]


class NearestKOut(C.Structure):
    """tyr_nearest_k_out: device pointers of tyr_query_nearest_k's outputs; count, uv, region, point may be NULL"""

    _fields_ = [("dist2", P), ("prim", P), ("count", P), ("uv", P), ("region", P), ("point", P)]


class SweepOut(C.Structure):
    """tyr_sweep_out: device pointers of tyr_query_sweep's outputs; region, point, center, normal may be NULL"""

    _fields_ = [("t", P), ("prim", P), ("region", P), ("point", P), ("center", P), ("normal", P)]


class SweepCapsuleOut(C.Structure):
    """tyr_sweep_capsule_out: device pointers of tyr_query_sweep_capsule's outputs; s, feature, region, point, center, normal may be NULL"""

    _fields_ = [("t", P), ("prim", P), ("s", P), ("feature", P), ("region", P), ("point", P), ("center", P), ("normal", P)]


class BoxOut(C.Structure):
    """tyr_box_out: device pointers of tyr_query_box's outputs; prim may be NULL when max_prims is 0"""

    _fields_ = [("count", P), ("prim", P)]


class TriOut(C.Structure):
    """tyr_tri_out: device pointers of tyr_query_tri's outputs; prim may be NULL when max_prims is 0"""

    _fields_ = [("count", P), ("prim", P)]


class SegmentOut(C.Structure):
    """tyr_segment_out: device pointers of tyr_query_segment's outputs; s, feature, region, on_segment, on_triangle may be NULL"""

    _fields_ = [("dist2", P), ("prim", P), ("s", P), ("feature", P), ("region", P), ("on_segment", P), ("on_triangle", P)]


class TriDistanceOut(C.Structure):
    """tyr_tri_distance_out: device pointers of tyr_query_tri_distance's outputs; feature, region, on_query, on_triangle may be NULL"""

    _fields_ = [("dist2", P), ("prim", P), ("feature", P), ("region", P), ("on_query", P), ("on_triangle", P)]


class SignedOut(C.Structure):
    """tyr_signed_out: device pointers of tyr_query_signed's outputs; prim, point, gradient, w may be NULL"""

    _fields_ = [("sd", P), ("prim", P), ("point", P), ("gradient", P), ("w", P)]


class SdfGrid(C.Structure):
    """tyr_sdf_grid: the voxel grid of tyr_bake_sdf"""

    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", c_u32 * 3), ("band", C.c_float), ("accuracy", C.c_float)]


class SdfOut(C.Structure):
    """tyr_sdf_out: device pointers of tyr_bake_sdf's outputs; prim, stats may be NULL"""

    _fields_ = [("sd", P), ("prim", P), ("stats", P)]


class HitsOut(C.Structure):
    """tyr_hits_out: device pointers of tyr_query_hits's outputs; uv, side, back_count may be NULL"""

    _fields_ = [("count", P), ("t", P), ("prim", P), ("uv", P), ("side", P), ("back_count", P)]


class OcclusionOut(C.Structure):
    """tyr_occlusion_out: device pointers of tyr_query_occlusion's outputs; mask, bent, origin, direction may be NULL"""

    _fields_ = [("visible", P), ("mask", P), ("bent", P), ("origin", P), ("direction", P)]


class AovChainOut(C.Structure):
    """tyr_aov_chain_out: device pointers of what tyr_render_aov_chain adds, NULL to skip one"""

    _fields_ = [("chain", P), ("end_prim", P), ("end_geom", P), ("length0", P), ("depth_first", P)]


class DenoiseIn(C.Structure):
    """tyr_denoise_in: device pointers of the frame (NULL: the ctx's blit buffer) and its guides"""

    _fields_ = [("accum", P), ("albedo", P), ("normal", P), ("depth", P)]


class DenoiseParams(C.Structure):
    _fields_ = [("passes", c_u32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("normal_power_log2", c_u32), ("flags", c_u32)]


class MotionIn(C.Structure):
    """tyr_motion_in: device ids from render_aov, the previous camera (host record), the previous triangle records (device, or NULL)"""

    _fields_ = [("prim", P), ("geom", P), ("prev_camera", P), ("prev_prims", P)]


class MotionOut(C.Structure):
    _fields_ = [("motion", P), ("prev_depth", P)]


class MotionChainIn(C.Structure):
    """tyr_motion_chain_in: render_aov(max_chain=...)'s chain and length0 (device)"""

    _fields_ = [("chain", P), ("length0", P)]


class TemporalIn(C.Structure):
    """tyr_temporal_in: device pointers of the frame (NULL: the ctx's blit buffer), its guides and its motion"""

    _fields_ = [("accum", P), ("albedo", P), ("normal", P), ("depth", P), ("motion", P), ("prev_depth", P)]


class TemporalParams(C.Structure):
    _fields_ = [("max_history", c_u32), ("depth_tolerance", C.c_float), ("normal_cos", C.c_float), ("flags", c_u32)]


class SvgfIn(C.Structure):
    """tyr_svgf_in: the inputs of tyr_temporal_in"""

    _fields_ = [("accum", P), ("albedo", P), ("normal", P), ("depth", P), ("motion", P), ("prev_depth", P)]


class SvgfParams(C.Structure):
    _fields_ = [("max_history", c_u32), ("depth_tolerance", C.c_float), ("normal_cos", C.c_float), ("passes", c_u32), ("sigma_luminance", C.c_float),
                ("sigma_depth", C.c_float), ("normal_power_log2", c_u32), ("flags", c_u32)]


class TaaIn(C.Structure):
    """tyr_taa_in: a resolved frame, render_aov's depth, render_motion's motion and prev_depth"""

    _fields_ = [("color", P), ("depth", P), ("motion", P), ("prev_depth", P)]


class TaaParams(C.Structure):
    _fields_ = [("alpha", C.c_float), ("gamma", C.c_float), ("flags", c_u32)]


class AllocateParams(C.Structure):
    _fields_ = [("total", c_u64), ("min_spp", c_u32), ("max_spp", c_u32)]


class PrimaryWindowInfo(C.Structure):
    _fields_ = [("x0", c_u32), ("x1", c_u32), ("y0", c_u32), ("y1", c_u32), ("local_y0", c_u32), ("local_y1", c_u32), ("whole_frame", c_u32), ("strays", c_u32), ("splits", c_u32)]


class Timings(C.Structure):
    _fields_ = [("ms", C.c_double * 5), ("launches", c_u64 * 5)]


# every symbol include/tyr_c.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "tyr_status_string": (C.c_char_p, [C.c_int]),
    "tyr_abi_version": (C.c_int, []),
    "tyr_create": (C.c_int, [C.POINTER(P), C.POINTER(Config)]),
    "tyr_destroy": (C.c_int, [P]),
    "tyr_scene_upload": (C.c_int, [P, P, c_i32, P, c_i32]),
    "tyr_set_spheres": (C.c_int, [P, P]),
    "tyr_set_triangle_emission": (C.c_int, [P, P]),
    "tyr_set_triangle_palette": (C.c_int, [P, P, P]),
    "tyr_set_camera": (C.c_int, [P, C.POINTER(CameraC)]),
    "tyr_set_sun_position": (C.c_int, [P, c_f, c_f]),
    "tyr_set_blit_buffer": (C.c_int, [P, P]),
    "tyr_get_blit_buffer": (P, [P]),
    "tyr_launch_kernels": (C.c_int, [P]),
    "tyr_set_budget": (C.c_int, [P, c_u64]),
    "tyr_set_frame": (C.c_int, [P, c_u32]),
    "tyr_get_counters": (C.c_int, [P, C.POINTER(Counters)]),
    "tyr_render": (C.c_int, [P, c_u32, c_u32, C.POINTER(c_u32)]),
    "tyr_resolve": (C.c_int, [P, P]),
    "tyr_reset_accum": (C.c_int, [P]),
    "tyr_read_accum": (C.c_int, [P, P]),
    "tyr_stage_begin": (C.c_int, [P]),
    "tyr_stage_primary": (C.c_int, [P]),
    "tyr_stage_extend": (C.c_int, [P]),
    "tyr_stage_shade": (C.c_int, [P]),
    "tyr_stage_connect": (C.c_int, [P]),
    "tyr_stage_end": (C.c_int, [P]),
    "tyr_sync": (C.c_int, [P]),
    "tyr_queue_export": (C.c_int, [P, C.c_int, P, c_u32]),
    "tyr_queue_import": (C.c_int, [P, P, c_u32]),
    "tyr_queue_rank_check": (C.c_int, [P, C.c_int, P, P]),
    "tyr_shadow_export": (C.c_int, [P, P, c_u32]),
    "tyr_shadow_import": (C.c_int, [P, P, c_u32]),
    "tyr_get_scene_info": (C.c_int, [P, C.POINTER(SceneInfo)]),
    "tyr_layout_probe": (C.c_int, [P, c_i32, P, c_i32, c_i32, C.POINTER(LayoutStats)]),
    "tyr_scene_hash": (C.c_int, [P, C.POINTER(LayoutStats)]),
    "tyr_vecmath_probe": (C.c_int, [c_i32, c_i32, P, P, P, c_u32, P]),
    "tyr_sunsky_probe": (C.c_int, [c_i32, C.c_float, C.c_float, c_i32, P, c_u32, P]),
    "tyr_sun_setup": (C.c_int, [C.c_float, C.c_float, P]),
    "tyr_camera_handle_input": (C.c_int, [P, P, C.c_double]),
    "tyr_get_timings": (C.c_int, [P, C.POINTER(Timings), C.c_int]),
    "tyr_primary_window": (C.c_int, [P, C.POINTER(PrimaryWindowInfo)]),
    "tyr_primary_window_probe": (C.c_int, [C.POINTER(CameraC), c_u32, c_u32, c_u32, c_u32, C.POINTER(c_f), C.POINTER(c_f), C.c_int, C.POINTER(PrimaryWindowInfo)]),
    "tyr_set_tuning": (C.c_int, [P, C.c_int, C.c_int]),
    "tyr_bvh_build": (C.c_int, [P, c_i32, P, P, c_i32]),
    "tyr_bvh_build_device": (C.c_int, [c_i32, P, c_i32, P, P, P]),
    "tyr_scene_build_upload": (C.c_int, [P, P, c_i32, P, P, P, P]),
    "tyr_triangle_bboxes": (C.c_int, [P, c_i32, P]),
    "tyr_set_build_threads": (C.c_int, [c_i32]),
    "tyr_camera_update": (C.c_int, [C.c_double, C.c_double, C.POINTER(c_f)]),
    "tyr_load_ply": (C.c_int, [C.c_char_p, C.POINTER(P)]),
    "tyr_free": (None, [P]),
    "tyr_write_ppm": (C.c_int, [C.c_char_p, P, c_u32, c_u32]),
    "tyr_write_pfm": (C.c_int, [C.c_char_p, P, c_u32, c_u32]),
    "tyr_write_png": (C.c_int, [C.c_char_p, P, c_u32, c_u32]),
    "tyr_default_spheres": (C.c_int, [P]),
    "tyr_dist_unique_id": (C.c_int, [P]),
    "tyr_dist_create": (C.c_int, [C.POINTER(P), P, P, c_i32, c_i32]),
    "tyr_dist_destroy": (C.c_int, [P]),
    "tyr_dist_combine": (C.c_int, [P, c_i32, c_i32, P]),
    "tyr_dist_wait": (C.c_int, [P]),
    "tyr_dist_info": (C.c_int, [P, C.POINTER(c_i32), C.POINTER(c_i32)]),
    "tyr_dist_owned_rows": (C.c_int, [c_u32, c_u32, c_u32, C.POINTER(c_u32), C.POINTER(c_u32)]),
    "tyr_dist_row_owner": (C.c_int, [c_u32, c_u32, C.POINTER(c_u32), C.POINTER(c_u32)]),
    "tyr_dist_pack_rows": (C.c_int, [P, P, c_u32, c_u32, c_u32, c_u32, P]),
    "tyr_dist_scatter_rows": (C.c_int, [P, P, c_u32, c_u32, c_u32, P]),
    "tyr_query_closest": (C.c_int, [P, c_u32, P, P, P, c_u32, P, P, P, P, P]),
    "tyr_query_any": (C.c_int, [P, c_u32, P, P, P, c_u32, P, P]),
    "tyr_query_error": (C.c_int, [P, C.POINTER(c_u32), C.c_int]),
    "tyr_query_nearest": (C.c_int, [P, c_u32, P, P, c_u32, P, P]),
    "tyr_query_nearest_k": (C.c_int, [P, c_u32, P, P, c_u32, c_u32, P, P]),
    "tyr_query_sweep": (C.c_int, [P, c_u32, P, P, P, P, c_u32, P, P]),
    "tyr_query_sweep_capsule": (C.c_int, [P, c_u32, P, P, P, P, P, c_u32, P, P]),
    "tyr_query_box": (C.c_int, [P, c_u32, P, P, c_u32, c_u32, P, P]),
    "tyr_query_tri": (C.c_int, [P, c_u32, P, P, P, c_u32, c_u32, P, P]),
    "tyr_query_segment": (C.c_int, [P, c_u32, P, P, P, c_u32, P, P]),
    "tyr_query_tri_distance": (C.c_int, [P, c_u32, P, P, P, P, c_u32, P, P]),
    "tyr_query_hits": (C.c_int, [P, c_u32, P, P, P, c_u32, c_u32, P, P]),
    "tyr_query_occlusion": (C.c_int, [P, c_u32, P, P, P, c_u32, C.c_float, c_u32, c_u32, P, P]),
    "tyr_query_winding": (C.c_int, [P, c_u32, P, C.c_float, P, P, P]),
    "tyr_query_signed": (C.c_int, [P, c_u32, P, P, C.c_float, c_u32, P, P]),
    "tyr_bake_sdf": (C.c_int, [P, P, c_u32, P, P]),
    "tyr_scene_moments": (C.c_int, [P, c_i32, c_i32, P]),
    "tyr_scene_refit": (C.c_int, [P, P, P, c_i32, c_u32, P, P]),
    "tyr_render_aov": (C.c_int, [P, c_u32, P, P]),
    "tyr_render_aov_chain": (C.c_int, [P, c_u32, c_u32, P, P, P]),
    "tyr_denoise": (C.c_int, [P, P, P, P, P]),
    "tyr_render_motion": (C.c_int, [P, P, P, P]),
    "tyr_render_motion_chain": (C.c_int, [P, P, P, P, P]),
    "tyr_temporal": (C.c_int, [P, P, P, P, P, P]),
    "tyr_svgf": (C.c_int, [P, P, P, P, P, P]),
    "tyr_set_sample_map": (C.c_int, [P, P, P, C.POINTER(c_u64)]),
    "tyr_render_adaptive": (C.c_int, [P, P, P, c_u32, C.POINTER(c_u32)]),
    "tyr_allocate_samples": (C.c_int, [P, P, P, P, C.POINTER(c_u64), P]),
    "tyr_taa": (C.c_int, [P, P, P, P, P]),
}

_libs: dict = {}


def lib() -> C.CDLL:
    """Load order matters when PyTorch shares the process: its wheels carry their own HIP runtime in the global symbol
    scope.  Import torch BEFORE the first call of this function (then this library's HIP calls bind to that one runtime);
    the other order leaves two runtimes in the process and the one that initialises second reports no device."""
    path = LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `python __graft_entry__.py build` (there is no fallback path)")
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the header disagree
            fn.restype = res
            fn.argtypes = args
        _libs[path] = L
    return _libs[path]


def status_string(status: int) -> str:
    return lib().tyr_status_string(status).decode()


def _check(status: int, what: str):
    if status != 0:
        raise TyrError(status, what)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(P)


def _dptrs(*tensors):
    """the device pointers of torch tensors, None (a null pointer) for None"""
    return [None if t is None else t.data_ptr() for t in tensors]


# ---- host side of the hot path ---------------------------------------------------------------


def triangle_bboxes(tris: np.ndarray) -> np.ndarray:
    """Scene.cpp:22-33"""
    t = np.ascontiguousarray(tris)
    out = np.zeros(t.shape[0], dtype=scenes.BBOX_DTYPE)
    _check(lib().tyr_triangle_bboxes(_ptr(t), t.shape[0], _ptr(out)), "tyr_triangle_bboxes")
    return out


def bvh_build(tris: np.ndarray, bboxes: np.ndarray | None = None, algo: int = 2):
    """class BVH (bvh.cpp:3-25): returns (nodes[:nNodes], reordered triangles)"""
    prims = np.ascontiguousarray(tris.copy())
    n = prims.shape[0]
    bb = np.ascontiguousarray(bboxes) if bboxes is not None else triangle_bboxes(prims)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=scenes.NODE_DTYPE)
    nn = lib().tyr_bvh_build(_ptr(prims), n, _ptr(bb), _ptr(nodes), algo)
    if nn < 0:
        raise TyrError(nn, "tyr_bvh_build")
    return nodes[:nn].copy(), prims


def bvh_build_device(tris: np.ndarray, bboxes: np.ndarray | None = None, device: int = 0):
    """(nodes, prims, (device_seconds, copy_seconds)): tyr_bvh_build_device -- the SAH build on the GPU, the reference's bytes"""
    prims = np.array(tris, dtype=scenes.TRIANGLE_DTYPE, copy=True)
    bb = triangle_bboxes(prims) if bboxes is None else np.ascontiguousarray(bboxes)  # (tyr_triangle_bboxes: the same boxes bvh_build() takes)
    n = prims.shape[0]
    nodes = np.zeros(max(2 * n - 1, 1), dtype=scenes.NODE_DTYPE)
    sec = (C.c_double * 2)(0.0, 0.0)
    rc = lib().tyr_bvh_build_device(device, _ptr(prims), n, _ptr(bb), _ptr(nodes), sec)
    if rc < 0:
        raise TyrError(rc, "tyr_bvh_build_device")
    return nodes[:rc].copy(), prims, (sec[0], sec[1])


def layout_probe(nodes: np.ndarray, prims: np.ndarray, want_pairs: bool = True) -> dict:
    """the host half of tyr_scene_upload without a device: sizes, FNV-1a hashes of the device arrays, seconds (tyr_layout_probe)"""
    nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims)
    st = LayoutStats()
    _check(lib().tyr_layout_probe(_ptr(nodes), nodes.shape[0], _ptr(prims), prims.shape[0], int(want_pairs), C.byref(st)), "tyr_layout_probe")
    return {k: getattr(st, k) for k, _ in st._fields_}


def load_ply(path: str) -> np.ndarray:
    """Scene::Load's import half for a PLY file: TRIANGLE_DTYPE array (Scene.cpp:3-47)"""
    out = P()
    n = lib().tyr_load_ply(os.fsencode(path), C.byref(out))
    if n < 0:
        raise TyrError(n, f"tyr_load_ply({path})")
    try:
        if n == 0:
            return np.zeros(0, dtype=scenes.TRIANGLE_DTYPE)
        buf = (C.c_char * (40 * n)).from_address(out.value)
        return np.frombuffer(buf, dtype=scenes.TRIANGLE_DTYPE, count=n).copy()
    finally:
        lib().tyr_free(out)


def write_image(path: str, rgba: np.ndarray, width: int, height: int):
    """PPM (tonemapped 8-bit) or PFM (float) by extension"""
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    low = path.lower()
    fn = lib().tyr_write_pfm if low.endswith(".pfm") else lib().tyr_write_png if low.endswith(".png") else lib().tyr_write_ppm
    _check(fn(os.fsencode(path), _ptr(a), width, height), "tyr_write_image")


def set_build_threads(threads: int):
    _check(lib().tyr_set_build_threads(threads), "tyr_set_build_threads")


def camera_update(horizontal_angle: float, vertical_angle: float) -> np.ndarray:
    """Camera::update (camera.cpp:46-52)"""
    out = (c_f * 3)()
    _check(lib().tyr_camera_update(horizontal_angle, vertical_angle, out), "tyr_camera_update")
    return np.array(out[:], dtype=np.float32)


def default_spheres() -> np.ndarray:
    s = np.zeros(7, dtype=scenes.SPHERE_DTYPE)
    _check(lib().tyr_default_spheres(_ptr(s)), "tyr_default_spheres")
    return s


# ---- the renderer ------------------------------------------------------------------------------


class Renderer:
    """one tyr_ctx"""

    def __init__(self, width, height, queue_size, device=0, rank=0, nranks=1, flags=0, stream=None, blit_buffer=None):
        self.L = lib()
        self.W, self.H, self.N = width, height, queue_size
        self.device = device
        self._side = None  # query_* on a stream without a handle of its own (the default stream): see _on_stream
        self._n_nodes = 0  # length of the node array of the scene uploaded last (refit(want_nodes=True))
        cfg = Config(width, height, queue_size, device, rank, nranks, flags, stream)
        h = P()
        _check(self.L.tyr_create(C.byref(h), C.byref(cfg)), "tyr_create")
        self.h = h
        self._dists = []
        _check(self.L.tyr_set_blit_buffer(self.h, blit_buffer), "tyr_set_blit_buffer")

    def close(self):
        for d in list(getattr(self, "_dists", [])):
            d.close()
        if getattr(self, "h", None):
            self.L.tyr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, nodes: np.ndarray, prims: np.ndarray):
        nodes = np.ascontiguousarray(nodes)
        prims = np.ascontiguousarray(prims)
        _check(self.L.tyr_scene_upload(self.h, _ptr(nodes), nodes.shape[0], _ptr(prims), prims.shape[0]), "tyr_scene_upload")
        self._n_nodes = nodes.shape[0] if prims.shape[0] else 0

    def set_spheres(self, spheres: np.ndarray | None):
        if spheres is None:
            _check(self.L.tyr_set_spheres(self.h, None), "tyr_set_spheres")
            return
        s = np.ascontiguousarray(spheres)
        _check(self.L.tyr_set_spheres(self.h, _ptr(s)), "tyr_set_spheres")

    def set_camera(self, cam):
        f3 = lambda x: (c_f * 3)(*[float(v) for v in x])  # noqa: E731
        c = CameraC(f3(cam.position), f3(cam.direction), f3(cam.up), cam.focalDistance, cam.lensRadius)
        _check(self.L.tyr_set_camera(self.h, C.byref(c)), "tyr_set_camera")

    def set_sun_position(self, x, y):
        _check(self.L.tyr_set_sun_position(self.h, x, y), "tyr_set_sun_position")

    def load_scene(self, scene, nodes, prims):
        self.upload(nodes, prims)
        self.set_spheres(scene.spheres)
        self.set_camera(scene.camera)
        self.set_sun_position(*scene.sun_position)
        self.set_triangle_emission(getattr(scene, "triangle_emission", (3.0, 3.0, 3.0)))
        if getattr(scene, "palette_color", None) is not None:
            self.set_triangle_palette(scene.palette_color, scene.palette_emission)

    def set_triangle_palette(self, color, emission=None):
        col = np.ascontiguousarray(color, dtype=np.float32).reshape(256, 3)
        em = None if emission is None else np.ascontiguousarray(emission, dtype=np.float32).reshape(256, 3)
        _check(self.L.tyr_set_triangle_palette(self.h, _ptr(col), None if em is None else _ptr(em)), "tyr_set_triangle_palette")

    def set_triangle_emission(self, rgb):
        _check(self.L.tyr_set_triangle_emission(self.h, (C.c_float * 3)(*[float(v) for v in rgb])), "tyr_set_triangle_emission")

    def set_budget(self, n):
        _check(self.L.tyr_set_budget(self.h, n), "tyr_set_budget")

    def set_frame(self, frame=1):
        """restart the frame counter every seed is built from (kernel.cu:667): the next render repeats the one that began at `frame`"""
        _check(self.L.tyr_set_frame(self.h, frame), "tyr_set_frame")

    def launch_kernels(self):
        _check(self.L.tyr_launch_kernels(self.h), "tyr_launch_kernels")

    def render(self, spp, max_iterations=0xFFFFFFFF) -> int:
        it = c_u32(0)
        _check(self.L.tyr_render(self.h, spp, max_iterations, C.byref(it)), "tyr_render")
        return it.value

    def stage(self, name):
        _check(getattr(self.L, "tyr_stage_" + name)(self.h), "tyr_stage_" + name)

    def counters(self) -> dict:
        k = Counters()
        _check(self.L.tyr_get_counters(self.h, C.byref(k)), "tyr_get_counters")
        return k.asdict()

    def primary_window(self) -> dict:
        """The camera window of the current camera and scene (tyr_primary_window): x0, x1, y0, y1, local_y0, local_y1, whole_frame, strays, splits."""
        w = PrimaryWindowInfo()
        _check(self.L.tyr_primary_window(self.h, C.byref(w)), "tyr_primary_window")
        return {k: int(getattr(w, k)) for k, _ in w._fields_}

    def timings(self, reset=False) -> dict:
        t = Timings()
        _check(self.L.tyr_get_timings(self.h, C.byref(t), int(reset)), "tyr_get_timings")
        return {n: {"ms": t.ms[i], "launches": int(t.launches[i])} for i, n in enumerate(KERNEL_NAMES)}

    TUNING_KEYS = {"refill_min_idle": 1, "waves_per_simd": 2, "min_traversing": 4, "ticket_chunk": 5, "static_share": 8, "staged_nodes": 9, "profile_mask": 11, "merge_trace": 12, "static_interleave": 13, "run_ahead": 14, "wide_drain": 15, "fold_spheres": 19, "retire_sky": 20, "resolve_shadows": 21, "wide_block_min_items": 22, "fold_prologue": 23, "layout_on_device": 24, "scan_in_trace": 25, "kernel_snapshot": 26, "stage_timing": 27, "shade_dense": 32,
                   "primary_overlap": 28, "overlap_trace_blocks": 29, "overlap_min_new": 30, "window_inset": 31}

    def set_tuning(self, **knobs):
        for name, v in knobs.items():
            if v is not None:
                _check(self.L.tyr_set_tuning(self.h, self.TUNING_KEYS[name], int(v)), "tyr_set_tuning")

    def reset_accum(self):
        _check(self.L.tyr_reset_accum(self.h), "tyr_reset_accum")

    def blit_buffer(self) -> np.ndarray:
        out = np.zeros((self.H * self.W, 4), dtype=np.float32)
        _check(self.L.tyr_read_accum(self.h, _ptr(out)), "tyr_read_accum")
        return out

    def resolve_into(self, device_ptr):
        _check(self.L.tyr_resolve(self.h, device_ptr), "tyr_resolve")

    def queue_rank_check(self, which=1):
        """(records, mismatches): the device's rank tables against the order ray_queue() presents (tyr_queue_rank_check)"""
        n, bad = c_u32(0), c_u32(0)
        _check(self.L.tyr_queue_rank_check(self.h, which, C.byref(n), C.byref(bad)), "tyr_queue_rank_check")
        return n.value, bad.value

    def ray_queue(self, which=0, count=None) -> np.ndarray:
        n = self.N if count is None else count
        out = np.zeros(n, dtype=scenes.RAY_DTYPE)
        _check(self.L.tyr_queue_export(self.h, which, _ptr(out), n), "tyr_queue_export")
        return out

    def shadow_queue(self, count=None) -> np.ndarray:
        n = self.N if count is None else count
        out = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
        _check(self.L.tyr_shadow_export(self.h, _ptr(out), n), "tyr_shadow_export")
        return out

    def import_shadow_queue(self, rays: np.ndarray):
        r = np.ascontiguousarray(rays)
        _check(self.L.tyr_shadow_import(self.h, _ptr(r), r.shape[0]), "tyr_shadow_import")

    def scene_hash(self) -> dict:
        """sizes and FNV-1a hashes of the scene arrays this ctx holds in HBM, read back (tyr_scene_hash): layout_probe()'s figures"""
        st = LayoutStats()
        _check(self.L.tyr_scene_hash(self.h, C.byref(st)), "tyr_scene_hash")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def build_upload(self, tris: np.ndarray, bboxes: np.ndarray | None = None, want_nodes: bool = True):
        """(nodes or None, prims, (build_s, layout_s, copy_s)): tyr_scene_build_upload -- the tree built and laid out on this ctx's device"""
        prims = np.array(tris, dtype=scenes.TRIANGLE_DTYPE, copy=True)
        bb = triangle_bboxes(prims) if bboxes is None else np.ascontiguousarray(bboxes)
        n = prims.shape[0]
        nodes = np.zeros(max(2 * n - 1, 1), dtype=scenes.NODE_DTYPE) if want_nodes else None
        sec = (C.c_double * 3)(0.0, 0.0, 0.0)
        nn = c_i32(0)
        _check(self.L.tyr_scene_build_upload(self.h, _ptr(prims), n, _ptr(bb), None if nodes is None else _ptr(nodes), C.byref(nn), sec), "tyr_scene_build_upload")
        self._n_nodes = nn.value
        return (None if nodes is None else nodes[: nn.value].copy()), prims, (sec[0], sec[1], sec[2])

    def scene_info(self) -> dict:
        s = SceneInfo()
        _check(self.L.tyr_get_scene_info(self.h, C.byref(s)), "tyr_get_scene_info")
        return {k: (float(getattr(s, k)) if k.endswith("_s") else int(getattr(s, k))) for k, _ in s._fields_}

    def import_work_queue(self, rays: np.ndarray, n_survivors: int):
        r = np.ascontiguousarray(rays)
        _check(self.L.tyr_queue_import(self.h, _ptr(r), n_survivors), "tyr_queue_import")

    # ---- ray queries on the uploaded scene (tyr_query_closest / tyr_query_any) ----
    def _query_take(self, a, what, shape):
        """a caller's float32 CUDA tensor as it is (a numpy array is copied to the ctx's device first)"""
        import torch

        dev = torch.device("cuda", self.device)
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{what}: a torch tensor or a numpy array")
        if a.dtype != torch.float32 or a.device != dev or not a.is_contiguous() or tuple(a.shape) != shape:
            raise ValueError(f"{what}: a contiguous float32 tensor of shape {shape} on {dev}, not {tuple(a.shape)} {a.dtype} on {a.device}")
        return a

    def _query_inputs(self, *inputs, optional=()):
        """a query's inputs, each (name, value, trailing shape): (n, tensors, staged).  n is the leading dimension of the first
        input, which is (N, 3) -- or -1, a length no tensor has, so that another shape fails in _query_take; every value goes
        through _query_take with the shape (n, *trailing), but an `optional` one that is None stays None; staged: some value
        was not a tensor, so its copy was made on torch's current stream."""
        import torch

        staged = not all(isinstance(a, torch.Tensor) for _, a, _ in inputs if a is not None)
        what, first, tail = inputs[0]
        first = first if isinstance(first, torch.Tensor) else np.asarray(first)
        n = first.shape[0] if first.ndim == 2 else -1
        inputs = ((what, first, tail),) + inputs[1:]
        return n, [None if a is None and what in optional else self._query_take(a, what, (n, *tail)) for what, a, tail in inputs], staged

    def _query_rays(self, origins, directions, tmax):
        """the caller's (N, 3) float32 CUDA tensors as they are (numpy arrays are copied to the ctx's device first)"""
        return self._query_inputs(("origins", origins, (3,)), ("directions", directions, (3,)), ("tmax", tmax, ()), optional=("tmax",))

    def _query_outputs(self, n, *specs):
        """a query's outputs: one uninitialised (n, *shape) tensor on the ctx's device per (shape, dtype), None for a spec of None"""
        import torch

        dev = torch.device("cuda", self.device)
        return [None if s is None else torch.empty((n, *s[0]), dtype=s[1], device=dev) for s in specs]

    def _query_call(self, name, stream, staged, *args):
        """the C call `name`(ctx, *args, stream handle) on `stream` (see _on_stream), then the queries' device error bits"""
        fn = getattr(self.L, name)
        self._on_stream(stream, lambda h: fn(self.h, *args, h), staged, name)
        self._query_finish()

    def _on_stream(self, stream, launch, staged, what="tyr_query"):
        """launch(handle) on `stream` (default: torch's current stream).  The default stream has no handle of its own (0 means
        the ctx's stream to the library): the work then goes to a side stream ordered after it and before what follows on it."""
        import torch

        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if staged and s != cur:
            s.wait_stream(cur)  # the copies of numpy inputs were made on the current stream
        if s.cuda_stream != 0:
            _check(launch(s.cuda_stream), what)
            return
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        self._side.wait_stream(s)
        _check(launch(self._side.cuda_stream), what)
        s.wait_stream(self._side)

    def refit(self, prims, bboxes=None, stream=None, want_nodes=False):
        """tyr_scene_refit: new triangle records, in the uploaded (build) order, for the scene this ctx holds -- the tree keeps its
        shape, its boxes follow the reference's rule.  prims: a TRIANGLE_DTYPE numpy array (host path), or a contiguous torch
        tensor on this ctx's device holding the 40-byte records (e.g. (n, 10) float32, or (n, 40) uint8), read on `stream`
        (default: torch's current stream).  bboxes: None (computed from the records), or BBOX_DTYPE numpy / (n, 6) float32
        tensor alike.  Returns the refitted node array with want_nodes=True, else None.  Raises TyrError as the C call fails."""
        nodes = np.zeros(self._n_nodes, dtype=scenes.NODE_DTYPE) if want_nodes else None
        out = None if nodes is None else _ptr(nodes)
        try:
            import torch
        except ImportError:
            torch = None
        if torch is not None and isinstance(prims, torch.Tensor):
            dev = torch.device("cuda", self.device)
            for a, what, size in ((prims, "prims", 40), (bboxes, "bboxes", 24)):
                if a is None:
                    continue
                if not isinstance(a, torch.Tensor) or a.device != dev or not a.is_contiguous() or a.numel() * a.element_size() % size:
                    raise ValueError(f"{what}: a contiguous tensor of {size}-byte records on {dev}")
            n = prims.numel() * prims.element_size() // 40
            if bboxes is not None and bboxes.numel() * bboxes.element_size() != 24 * n:
                raise ValueError("bboxes: one 24-byte box per triangle")
            pp, bp = _dptrs(prims, bboxes)
            self._on_stream(stream, lambda h: self.L.tyr_scene_refit(self.h, pp, bp, n, TYR_REFIT_DEVICE, h, out), False, "tyr_scene_refit")
        else:
            p = np.ascontiguousarray(prims, dtype=scenes.TRIANGLE_DTYPE)
            bb = None if bboxes is None else np.ascontiguousarray(bboxes, dtype=scenes.BBOX_DTYPE)
            if bb is not None and bb.shape != p.shape:
                raise ValueError("bboxes: one box per triangle")
            _check(self.L.tyr_scene_refit(self.h, _ptr(p), None if bb is None else _ptr(bb), p.shape[0], 0, None, out), "tyr_scene_refit")
        return nodes

    def query_error(self, reset=True) -> int:
        """tyr_query_error: the device-side error bits of this ctx's queries (1: traversal stack overflow); waits for them"""
        bits = c_u32()
        _check(self.L.tyr_query_error(self.h, C.byref(bits), 1 if reset else 0), "tyr_query_error")
        return bits.value

    def _query_finish(self):
        bits = self.query_error(reset=True)
        if bits:
            raise TyrError(TYR_ERR_DEVICE, f"tyr_query: device error bits {bits:#x}")

    def query_closest(self, origins, directions, tmax=None, spheres=False, stream=None):
        """closest hit of every ray against the uploaded scene (CachedBVH::intersect with ray.distance = tmax, bvh.h:118-161;
        with spheres=True intersect_scene, kernel.cu:125-140).  Returns torch tensors (t, prim, geom, uv): a miss keeps
        t = tmax with prim = geom = -1 and uv = (0, 0); geom 0 = sphere (prim = its index), 1 = triangle (prim = build order)."""
        import torch

        n, ins, staged = self._query_rays(origins, directions, tmax)
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), ((), torch.int32), ((2,), torch.float32))
        self._query_call("tyr_query_closest", stream, staged, n, *_dptrs(*ins), TYR_QUERY_SPHERES if spheres else 0, *_dptrs(*outs))
        return tuple(outs)

    def query_any(self, origins, directions, tmax=None, spheres=False, stream=None):
        """is anything hit within tmax (CachedBVH::intersectSimple, bvh.h:213-256; with spheres=True intersect_scene_simple,
        kernel.cu:163-174)?  Returns a bool torch tensor."""
        import torch

        n, ins, staged = self._query_rays(origins, directions, tmax)
        (occ,) = self._query_outputs(n, ((), torch.bool))
        self._query_call("tyr_query_any", stream, staged, n, *_dptrs(*ins), TYR_QUERY_SPHERES if spheres else 0, occ.data_ptr())
        return occ

    def query_nearest(self, points, max_dist=None, stream=None):
        """tyr_query_nearest: for every point the nearest triangle of the uploaded scene (include/tyr_c.h "Closest-point queries").
        points: (N, 3) float32, max_dist: (N,) or None -- torch tensors on this ctx's device, taken as they are, or numpy arrays.
        Returns torch tensors (dist2, prim, uv, region, point): without a triangle nearer than max_dist, dist2 = max_dist^2 (+inf for
        an invalid point or max_dist), prim = -1, uv = (0, 0), region = 0 and point = the query point."""
        import torch

        n, ins, staged = self._query_inputs(("points", points, (3,)), ("max_dist", max_dist, ()), optional=("max_dist",))
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), ((2,), torch.float32), ((), torch.uint8), ((3,), torch.float32))
        out = NearestOut(*_dptrs(*outs))
        self._query_call("tyr_query_nearest", stream, staged, n, *_dptrs(*ins), 0, C.byref(out))
        return tuple(outs)

    def query_sweep(self, origins, directions, radius, tmax=None, normal=False, stream=None):
        """tyr_query_sweep: for every sphere of radius `radius` whose centre moves from `origins` along `directions`, the first
        contact with the uploaded scene (include/tyr_c.h "Swept-sphere queries").  origins, directions: (N, 3) float32, radius: a
        number or (N,), tmax: (N,) or None (1: the whole displacement) -- torch tensors on this ctx's device, taken as they are,
        or numpy arrays.  Returns torch tensors (t, prim, region, point, center), and normal behind them with normal=True: without
        a contact t = tmax, prim = -1 and center = point = the end of the path; an invalid sweep has t = +inf."""
        import torch

        n, (o, d, tm), staged = self._query_rays(origins, directions, tmax)
        if isinstance(radius, (int, float, np.floating, np.integer)):
            r = torch.full((max(n, 0),), float(radius), dtype=torch.float32, device=o.device)
            staged = True  # filled on torch's current stream: `stream` has to wait for it like for a copied numpy input
        else:
            staged = staged or not isinstance(radius, torch.Tensor)
            r = self._query_take(radius, "radius", (n,))
        vec = ((3,), torch.float32)
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), ((), torch.uint8), vec, vec, vec if normal else None)
        out = SweepOut(*_dptrs(*outs))
        self._query_call("tyr_query_sweep", stream, staged, n, *_dptrs(o, d, r, tm), 0, C.byref(out))
        return tuple(outs) if normal else tuple(outs[:5])

    def query_sweep_capsule(self, p, q, directions, radius, tmax=None, normal=False, stream=None):
        """tyr_query_sweep_capsule: for every capsule of radius `radius` around the axis p -> q whose ends both move along
        `directions`, the first contact with the uploaded scene (include/tyr_c.h "Swept-capsule queries").  p, q, directions:
        (N, 3) float32, radius: a number or (N,), tmax: (N,) or None (1: the whole displacement) -- torch tensors on this ctx's
        device, taken as they are, or numpy arrays.  Returns torch tensors (t, prim, s, feature, region, point, center), and normal
        behind them with normal=True: s is where on the axis the contact is (0 at p, 1 at q), center that point of the moved axis;
        without a contact t = tmax, prim = -1 and center = point = the end of p's path; an invalid capsule has t = +inf."""
        import torch

        n, (a, b, d, tm), staged = self._query_inputs(("p", p, (3,)), ("q", q, (3,)), ("directions", directions, (3,)), ("tmax", tmax, ()), optional=("tmax",))
        if isinstance(radius, (int, float, np.floating, np.integer)):
            r = torch.full((max(n, 0),), float(radius), dtype=torch.float32, device=a.device)
            staged = True  # filled on torch's current stream: `stream` has to wait for it like for a copied numpy input
        else:
            staged = staged or not isinstance(radius, torch.Tensor)
            r = self._query_take(radius, "radius", (n,))
        vec, byte = ((3,), torch.float32), ((), torch.uint8)
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), ((), torch.float32), byte, byte, vec, vec, vec if normal else None)
        out = SweepCapsuleOut(*_dptrs(*outs))
        self._query_call("tyr_query_sweep_capsule", stream, staged, n, *_dptrs(a, b, d, r, tm), 0, C.byref(out))
        return tuple(outs) if normal else tuple(outs[:7])

    def query_segment(self, p, q, max_dist=None, stream=None):
        """tyr_query_segment: for every segment p -> q the triangle of the uploaded scene that comes nearest to it (include/tyr_c.h
        "Closest-segment queries").  p, q: (N, 3) float32, max_dist: a number, (N,) or None -- torch tensors on this ctx's device,
        taken as they are, or numpy arrays.  Returns torch tensors (dist2, prim, s, feature, region, on_segment, on_triangle):
        without a triangle nearer than max_dist, dist2 = max_dist^2 (+inf for an invalid segment or max_dist), prim = -1, s = 0,
        feature = region = 0 and both points = p.  A capsule of radius r at rest touches the scene where prim >= 0 with max_dist = r."""
        import torch

        if isinstance(max_dist, (int, float, np.floating, np.integer)):
            n, (a, b), staged = self._query_inputs(("p", p, (3,)), ("q", q, (3,)))
            md = torch.full((max(n, 0),), float(max_dist), dtype=torch.float32, device=a.device)
            staged = True  # filled on torch's current stream: `stream` has to wait for it like for a copied numpy input
        else:
            n, (a, b, md), staged = self._query_inputs(("p", p, (3,)), ("q", q, (3,)), ("max_dist", max_dist, ()), optional=("max_dist",))
        vec = ((3,), torch.float32)
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), ((), torch.float32), ((), torch.uint8), ((), torch.uint8), vec, vec)
        out = SegmentOut(*_dptrs(*outs))
        self._query_call("tyr_query_segment", stream, staged, n, *_dptrs(a, b, md), 0, C.byref(out))
        return tuple(outs)

    def query_tri_distance(self, a, b, c, max_dist=None, skip_shared=False, feature=False, region=False, points=False, stream=None):
        """tyr_query_tri_distance: for every triangle (a, b, c) the triangle of the uploaded scene that comes nearest to it
        (include/tyr_c.h "Closest-triangle queries").  a, b, c: (N, 3) float32, max_dist: a number, (N,) or None -- torch tensors on
        this ctx's device, taken as they are, or numpy arrays.  skip_shared: a scene triangle with a corner equal to one of the
        query's is no candidate (the mesh's own triangles as queries: self-proximity).  Returns torch tensors (dist2, prim), and
        behind them those asked for, in this order: feature, region, on_query and on_triangle (points=True: both).  Without a
        triangle nearer than max_dist, dist2 = max_dist^2 (+inf for an invalid query or max_dist), prim = -1, feature = region = 0
        and both points = a."""
        import torch

        ins = (("a", a, (3,)), ("b", b, (3,)), ("c", c, (3,)))
        if isinstance(max_dist, (int, float, np.floating, np.integer)):
            n, (ta, tb, tc), staged = self._query_inputs(*ins)
            md = torch.full((max(n, 0),), float(max_dist), dtype=torch.float32, device=ta.device)
            staged = True  # filled on torch's current stream: `stream` has to wait for it like for a copied numpy input
        else:
            n, (ta, tb, tc, md), staged = self._query_inputs(*ins, ("max_dist", max_dist, ()), optional=("max_dist",))
        vec, byte = ((3,), torch.float32), ((), torch.uint8)
        outs = self._query_outputs(n, ((), torch.float32), ((), torch.int32), byte if feature else None, byte if region else None, vec if points else None, vec if points else None)
        out = TriDistanceOut(*_dptrs(*outs))
        self._query_call("tyr_query_tri_distance", stream, staged, n, *_dptrs(ta, tb, tc, md), TYR_QUERY_TRI_SKIP_SHARED if skip_shared else 0, C.byref(out))
        return tuple(x for x in outs if x is not None)

    def query_box(self, lo, hi, max_prims=0, any=False, stream=None):
        """tyr_query_box: for every axis-aligned box [lo, hi] the triangles of the uploaded scene it touches (include/tyr_c.h
        "Box-overlap queries"; touching counts).  lo, hi: (N, 3) float32 -- torch tensors on this ctx's device, taken as they are,
        or numpy arrays.  Returns count, (N,) int32 (the library's uint32): every triangle the box touches, not capped by
        max_prims; with max_prims > 0 (count, prim), prim (N, max_prims) int32 the lowest build-order indices of them, ascending,
        unused entries -1; with any=True (max_prims must be 0) a bool tensor, count > 0, from a walk that stops at the first
        triangle.  An invalid box (a NaN or infinite component, lo > hi on an axis) touches nothing."""
        import contextlib

        import torch

        k = int(max_prims)
        if not 0 <= k <= TYR_QUERY_BOX_MAX:
            raise ValueError(f"max_prims: 0 .. {TYR_QUERY_BOX_MAX}")
        if any and k:
            raise ValueError("any=True answers without indices: max_prims must be 0")
        n, ins, staged = self._query_inputs(("lo", lo, (3,)), ("hi", hi, (3,)))
        cnt, prim = self._query_outputs(n, ((), torch.int32), ((k,), torch.int32) if k else None)
        out = BoxOut(*_dptrs(cnt, prim))
        self._query_call("tyr_query_box", stream, staged, n, *_dptrs(*ins), k, TYR_QUERY_BOX_ANY if any else 0, C.byref(out))
        if any:
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                return cnt != 0
        return (cnt, prim) if k else cnt

    def query_tri(self, a, b, c, max_prims=0, any=False, skip_shared=False, stream=None):
        """tyr_query_tri: for every triangle with the corners a, b, c the triangles of the uploaded scene it touches (include/tyr_c.h
        "Triangle-overlap queries"; touching counts).  a, b, c: (N, 3) float32 -- torch tensors on this ctx's device, taken as they
        are, or numpy arrays.  Returns what query_box returns: count, (N,) int32 (the library's uint32), not capped by max_prims;
        with max_prims > 0 (count, prim), prim (N, max_prims) int32 the lowest build-order indices of them, ascending, unused
        entries -1; with any=True (max_prims must be 0) a bool tensor, count > 0, from a walk that stops at the first triangle.
        skip_shared=True: a scene triangle with a corner equal to one of the query's is not reported (self-intersection checks
        with the mesh's own triangles).  A query with a NaN or infinite component touches nothing."""
        import contextlib

        import torch

        k = int(max_prims)
        if not 0 <= k <= TYR_QUERY_TRI_MAX:
            raise ValueError(f"max_prims: 0 .. {TYR_QUERY_TRI_MAX}")
        if any and k:
            raise ValueError("any=True answers without indices: max_prims must be 0")
        n, ins, staged = self._query_inputs(("a", a, (3,)), ("b", b, (3,)), ("c", c, (3,)))
        cnt, prim = self._query_outputs(n, ((), torch.int32), ((k,), torch.int32) if k else None)
        out = TriOut(*_dptrs(cnt, prim))
        flags = (TYR_QUERY_TRI_ANY if any else 0) | (TYR_QUERY_TRI_SKIP_SHARED if skip_shared else 0)
        self._query_call("tyr_query_tri", stream, staged, n, *_dptrs(*ins), k, flags, C.byref(out))
        if any:
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                return cnt != 0
        return (cnt, prim) if k else cnt

    def query_nearest_k(self, points, k, max_dist=None, count=False, stream=None):
        """tyr_query_nearest_k: for every point the k nearest triangles of the uploaded scene inside max_dist (include/tyr_c.h
        "k-nearest queries").  points: (N, 3) float32, max_dist: (N,) or None -- torch tensors on this ctx's device, taken as they
        are, or numpy arrays.  Returns torch tensors (dist2, prim, uv, region, point) of shapes (N, k), (N, k), (N, k, 2), (N, k),
        (N, k, 3): nearest first, of equal dist2 the lower build-order index first -- unused entries hold dist2 = max_dist^2 (+inf
        for an invalid point or max_dist), prim = -1, uv = (0, 0), region = 0 and point = the query point.  With count=True a
        sixth tensor (N,) int32 (the library's uint32): every triangle inside max_dist, not capped by k -- the search is then
        pruned by max_dist alone, so give one."""
        import torch

        if not 1 <= int(k) <= TYR_QUERY_NEAREST_K_MAX:
            raise ValueError(f"k: 1 .. {TYR_QUERY_NEAREST_K_MAX}")
        k = int(k)
        n, ins, staged = self._query_inputs(("points", points, (3,)), ("max_dist", max_dist, ()), optional=("max_dist",))
        dist2, prim, cnt, uv, region, point = self._query_outputs(
            n, ((k,), torch.float32), ((k,), torch.int32), ((), torch.int32) if count else None, ((k, 2), torch.float32), ((k,), torch.uint8), ((k, 3), torch.float32))
        out = NearestKOut(*_dptrs(dist2, prim, cnt, uv, region, point))
        self._query_call("tyr_query_nearest_k", stream, staged, n, *_dptrs(*ins), k, 0, C.byref(out))
        return (dist2, prim, uv, region, point, cnt) if count else (dist2, prim, uv, region, point)

    def query_hits(self, origins, directions, tmax=None, max_hits=4, two_sided=False, stream=None):
        """tyr_query_hits: every surface a ray goes through within (1e-3, tmax - 1e-3) (include/tyr_c.h "Multi-hit queries").
        origins, directions: (N, 3) float32, tmax: (N,) or None (VERY_FAR) -- torch tensors on this ctx's device, taken as they are,
        or numpy arrays.  Returns torch tensors (count, t, prim, uv, side, back_count): count (N,) int32 (the
        library's uint32), the number of hits in range (not capped by max_hits); t, prim, side (N, max_hits) and uv (N, max_hits, 2) the nearest
        max_hits of them, nearest first, of equal t the lower build-order index first -- unused entries hold t = tmax, prim = -1,
        uv = (0, 0), side = 0; back_count (N,) the hits met from behind (two_sided=True; side 1).  Inside a closed mesh: count odd
        with two_sided=True."""
        import torch

        if not 1 <= int(max_hits) <= TYR_QUERY_HITS_MAX:
            raise ValueError(f"max_hits: 1 .. {TYR_QUERY_HITS_MAX}")
        k = int(max_hits)
        n, ins, staged = self._query_rays(origins, directions, tmax)
        outs = self._query_outputs(n, ((), torch.int32), ((k,), torch.float32), ((k,), torch.int32), ((k, 2), torch.float32), ((k,), torch.uint8), ((), torch.int32))
        out = HitsOut(*_dptrs(*outs))
        self._query_call("tyr_query_hits", stream, staged, n, *_dptrs(*ins), k, TYR_QUERY_TWO_SIDED if two_sided else 0, C.byref(out))
        return tuple(outs)

    def query_occlusion(self, points, normals, samples=64, max_dist=None, bias=1e-3, seed=0, spheres=False, mask=False, bent=False, rays=False, stream=None):
        """tyr_query_occlusion: for every point, `samples` cosine-weighted any-hit rays over the hemisphere of its normal, made on
        the device (include/tyr_c.h "Occlusion queries").  points, normals: (N, 3) float32, max_dist: (N,) or None (VERY_FAR) --
        torch tensors on this ctx's device, taken as they are, or numpy arrays.  Returns torch tensors (visible, mask, bent, origin,
        direction), None for what was not asked for: visible (N,) int32 (the library's uint32), the samples nothing blocks -- AO =
        visible / samples; mask (N, (samples + 31) // 32) int32 (uint32 words), bit s % 32 of word s // 32 set for a visible
        sample; bent (N, 3), the sum of the visible samples' directions in sample order (bent=True implies the mask); with
        rays=True origin (N, 3) and direction (N, samples, 3), every sample's ray.  An invalid point (a NaN, infinite or zero
        normal, a NaN point) has visible = 0."""
        import torch

        if not 1 <= int(samples) <= TYR_QUERY_OCCLUSION_MAX_SAMPLES:
            raise ValueError(f"samples: 1 .. {TYR_QUERY_OCCLUSION_MAX_SAMPLES}")
        S = int(samples)
        n, ins, staged = self._query_inputs(("points", points, (3,)), ("normals", normals, (3,)), ("max_dist", max_dist, ()), optional=("max_dist",))
        outs = self._query_outputs(
            n,
            ((), torch.int32),
            (((S + 31) // 32,), torch.int32) if (mask or bent) else None,
            ((3,), torch.float32) if bent else None,
            ((3,), torch.float32) if rays else None,
            ((S, 3), torch.float32) if rays else None,
        )
        out = OcclusionOut(*_dptrs(*outs))
        self._query_call("tyr_query_occlusion", stream, staged, n, *_dptrs(*ins), S, float(bias), int(seed) & 0xFFFFFFFF, TYR_QUERY_SPHERES if spheres else 0, C.byref(out))
        return tuple(outs)

    def query_winding(self, points, accuracy=2.0, terms=False, stream=None):
        """tyr_query_winding: the generalised winding number of the uploaded triangles at every point (include/tyr_c.h "Winding
        numbers"; the ctx needs TYR_FLAG_WINDING) -- 1 inside a closed outward-facing mesh, 0 outside, 0.5 on it, so `w > 0.5` is
        the inside test.  points: (N, 3) float32, a torch tensor on this ctx's device, taken as it is, or a numpy array; accuracy:
        how many box reaches away a node counts as far (math.inf: the exact sum).  Returns the torch tensor w (N,) float32, or with
        terms=True (w, terms) with terms (N, 2) int32 (the library's uint32): the dipoles and triangles summed for the point."""
        import torch

        n, (p,), staged = self._query_inputs(("points", points, (3,)))
        w, t = self._query_outputs(n, ((), torch.float32), ((2,), torch.int32) if terms else None)
        self._query_call("tyr_query_winding", stream, staged, n, p.data_ptr(), float(accuracy), *_dptrs(w, t))
        return (w, t) if terms else w

    def query_signed(self, points, max_dist=None, accuracy=2.0, gradient=False, stream=None):
        """tyr_query_signed: the signed distance of every point to the uploaded triangles (include/tyr_c.h "Signed-distance queries";
        the ctx needs TYR_FLAG_WINDING) -- tyr_query_nearest's distance with the sign of tyr_query_winding's inside test, negative
        inside.  points: (N, 3) float32, max_dist: (N,) or None -- torch tensors on this ctx's device, taken as they are, or numpy
        arrays; accuracy: query_winding's.  Returns torch tensors (sd, prim, point, w), and gradient (N, 3) behind them with
        gradient=True: the unit direction in which sd grows.  Without a triangle nearer than max_dist, sd = +-max_dist, prim = -1
        and point = the query point; an invalid point or max_dist has sd = w = NaN."""
        import torch

        n, ins, staged = self._query_inputs(("points", points, (3,)), ("max_dist", max_dist, ()), optional=("max_dist",))
        vec = ((3,), torch.float32)
        sd, prim, point, grad, w = self._query_outputs(n, ((), torch.float32), ((), torch.int32), vec, vec if gradient else None, ((), torch.float32))
        out = SignedOut(*_dptrs(sd, prim, point, grad, w))
        self._query_call("tyr_query_signed", stream, staged, n, *_dptrs(*ins), float(accuracy), 0, C.byref(out))
        return (sd, prim, point, w, grad) if gradient else (sd, prim, point, w)

    def bake_sdf(self, origin, cell, dims, band, accuracy=2.0, prim=False, stats=False, stream=None):
        """tyr_bake_sdf: a narrow-band signed-distance grid of the uploaded triangles (include/tyr_c.h "Signed-distance queries"; the
        ctx needs TYR_FLAG_WINDING).  origin: the corner of voxel (0, 0, 0); cell: a voxel's edge; dims: (nx, ny, nz); band:
        distances are answered up to it, +-band beyond.  The voxel centres are made on the device.  Returns the torch tensor sd
        (nz, ny, nx) float32; with prim=True the nearest triangle per voxel (the same shape, int32, -1 = none inside band) behind
        it; with stats=True (near bricks, far bricks) as an int32 tensor of 2 (the library's uint32) behind that."""
        import torch

        nx, ny, nz = (int(d) for d in dims)
        grid = SdfGrid((C.c_float * 3)(*(float(o) for o in origin)), float(cell), (c_u32 * 3)(nx, ny, nz), float(band), float(accuracy))
        dev = torch.device("cuda", self.device)
        ok = min(nx, ny, nz) >= 1 and nx * ny * nz < 2**31
        shape = (nz, ny, nx) if ok else (0, 0, 0)  # (a refused grid: the library says so, nothing is written)
        sd = torch.empty(shape, dtype=torch.float32, device=dev)
        pr = torch.empty(shape, dtype=torch.int32, device=dev) if prim else None
        st = torch.empty(2, dtype=torch.int32, device=dev) if stats else None
        out = SdfOut(*_dptrs(sd, pr, st))
        self._query_call("tyr_bake_sdf", stream, False, C.byref(grid), 0, C.byref(out))
        return sd if not (prim or stats) else tuple(x for x in (sd, pr, st) if x is not None)

    def scene_moments(self, first=0, count=None) -> np.ndarray:
        """tyr_scene_moments: (count, 8) float64 -- p xyz, N xyz, r2, S of nodes first .. first + count - 1 of the moment tree this
        ctx holds (count=None: up to the last node of the scene uploaded through this Renderer)"""
        if count is None:
            count = max(self._n_nodes - int(first), 0)
        out = np.zeros((int(count), 8), dtype=np.float64)
        _check(self.L.tyr_scene_moments(self.h, int(first), int(count), _ptr(out) if count else None), "tyr_scene_moments")
        return out

    def render_aov(self, spp, albedo=True, normal=True, depth=True, ids=True, stream=None, max_chain=None) -> dict:
        """tyr_render_aov: first-hit guide buffers of the current camera at the current frame counter, spp camera rays per pixel
        (the rays of a render's first wavefront from an empty queue).  Returns a dict of torch tensors on this ctx's device:
        "albedo", "normal" (H, W, 3) float32, "depth" (H, W) float32 (VERY_FAR where no sample hit), "prim", "geom" (H, W) int32
        (sample 0's identity: geom 0 sphere, 1 triangle, -1 miss) -- those asked for.  Runs on `stream` (default: torch's current
        stream) and returns once it is done.  A sharded ctx fills its own rows; the others are zero.
        max_chain (0 .. AOV_CHAIN_MAX; None: the call above) takes tyr_render_aov_chain instead: albedo, normal and depth are
        those of the surface each sample's specular chain ends on, after at most max_chain mirror / glass bounces; prim, geom
        stay the first hit; and the dict gains "chain", "end_prim", "end_geom" (H, W) int32, "length0" and "depth_first" (H, W)
        float32 (include/tyr_c.h "Specular-chain guides")."""
        import torch

        dev = torch.device("cuda", self.device)
        res = {}
        if albedo:
            res["albedo"] = torch.zeros((self.H, self.W, 3), dtype=torch.float32, device=dev)
        if normal:
            res["normal"] = torch.zeros((self.H, self.W, 3), dtype=torch.float32, device=dev)
        if depth:
            res["depth"] = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
        if ids:
            res["prim"] = torch.zeros((self.H, self.W), dtype=torch.int32, device=dev)
            res["geom"] = torch.zeros((self.H, self.W), dtype=torch.int32, device=dev)
        out = AovOut(*(res[k].data_ptr() if k in res else None for k in ("albedo", "normal", "depth", "prim", "geom")))
        if max_chain is None:
            self._query_call("tyr_render_aov", stream, True, spp, C.byref(out))
        else:
            for k in ("chain", "end_prim", "end_geom"):
                res[k] = torch.zeros((self.H, self.W), dtype=torch.int32, device=dev)
            for k in ("length0", "depth_first"):
                res[k] = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
            ext = AovChainOut(*(res[k].data_ptr() for k in ("chain", "end_prim", "end_geom", "length0", "depth_first")))
            self._query_call("tyr_render_aov_chain", stream, True, spp, max_chain, C.byref(out), C.byref(ext))
        return res

    def denoise(self, albedo, normal, depth, accum=None, passes=DENOISE_PASSES, sigma_color=DENOISE_SIGMA_COLOR, sigma_depth=DENOISE_SIGMA_DEPTH,
                normal_power_log2=DENOISE_NORMAL_POWER_LOG2, resolve=False, stream=None):
        """tyr_denoise: the edge-avoiding a-trous filter of a frame guided by render_aov's buffers.  albedo, normal (H, W, 3),
        depth (H, W) and accum (H, W, 4; None: this ctx's blit buffer) are contiguous float32 tensors on this ctx's device.
        Returns an (H, W, 4) float32 tensor: the filtered frame in the blit buffer's layout with one sample per pixel, or
        with resolve=True tone-mapped as resolve_into writes it.  Runs on `stream` (default: torch's current stream) and
        returns without waiting for it."""
        din = DenoiseIn(*self._frame_inputs(accum=accum, albedo=albedo, normal=normal, depth=depth))
        prm = DenoiseParams(passes, sigma_color, sigma_depth, normal_power_log2, TYR_DENOISE_RESOLVE if resolve else 0)
        (out,) = self._frame_outputs(4)
        self._frame_call("tyr_denoise", stream, C.byref(din), C.byref(prm), out)
        return out

    def _frame_tensors(self, ins):
        import torch

        dev = torch.device("cuda", self.device)
        for what, (t, dtype, size) in ins.items():
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or t.numel() != size:
                raise ValueError(f"{what}: a contiguous {dtype} tensor of {size} values on {dev}")
        return dev

    # values per pixel of the frame passes' float32 planes, by argument name; the optional ones may be None
    _FRAME_PLANES = {"albedo": 3, "normal": 3, "depth": 1, "prev_depth": 1, "motion": 2, "accum": 4, "color": 4, "out": 4}
    _FRAME_OPTIONAL = ("accum", "out")

    def _frame_inputs(self, **ins):
        """a frame pass's planes by argument name, checked (_frame_tensors): their addresses in the order given, None for an
        optional one that is None"""
        import torch

        n = self.H * self.W
        self._frame_tensors({k: (t, torch.float32, self._FRAME_PLANES[k] * n) for k, t in ins.items() if t is not None or k not in self._FRAME_OPTIONAL})
        return [None if t is None else t.data_ptr() for t in ins.values()]

    def _frame_outputs(self, *planes, dtype=None, zero=False):
        """a frame pass's outputs: one (H, W, k) tensor on the ctx's device per k -- (H, W) for 0, None for None -- float32
        unless `dtype` says otherwise, uninitialised unless `zero`"""
        import torch

        make = torch.zeros if zero else torch.empty
        dev = torch.device("cuda", self.device)
        return [None if k is None else make((self.H, self.W, k) if k else (self.H, self.W), dtype=dtype or torch.float32, device=dev) for k in planes]

    def _frame_call(self, name, stream, *args):
        """the C call `name`(ctx, *args, stream handle) on `stream` (see _on_stream).  A tensor among args is an output: its address
        is passed, and when a stream was given it is recorded there -- it was written there: the allocator must not hand its
        memory out before that stream is done."""
        import torch

        fn = getattr(self.L, name)
        outs = [a for a in args if isinstance(a, torch.Tensor)]
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        self._on_stream(stream, lambda h: fn(self.h, *args, h), True, name)
        if stream is not None:
            for t in outs:
                t.record_stream(stream)

    def render_motion(self, prim, geom, prev_camera, prev_prims=None, stream=None, chain=None, length0=None) -> dict:
        """tyr_render_motion: per pixel the motion to the previous frame and the depth expected there, from render_aov's sample-0
        ids (prim, geom: (H, W) int32 tensors on this ctx's device) at the current camera and frame.  prev_camera: the previous
        frame's camera (fields as set_camera takes them).  prev_prims: None (the geometry did not move), or the records held
        before the last refit in the uploaded order -- a contiguous tensor of 40-byte records on this device, or a TRIANGLE_DTYPE
        numpy array (copied over on the current stream).  Returns a dict of torch tensors: "motion" (H, W, 2), "prev_depth"
        (H, W).  Runs on `stream` (default: torch's current stream) and returns once it is enqueued.  A sharded ctx fills its own
        rows; the others are zero.  chain, length0 (both or neither; (H, W) int32 / float32 from render_aov(max_chain=...)):
        tyr_render_motion_chain -- where a pixel's chain has bounces, the motion of the virtual image point seen through them."""
        import torch

        n = self.H * self.W
        dev = self._frame_tensors({"prim": (prim, torch.int32, n), "geom": (geom, torch.int32, n)})
        if (chain is None) != (length0 is None):
            raise ValueError("chain and length0 go together")
        if chain is not None:
            self._frame_tensors({"chain": (chain, torch.int32, n), "length0": (length0, torch.float32, n)})
        f3 = lambda x: (c_f * 3)(*[float(v) for v in x])  # noqa: E731
        cam = CameraC(f3(prev_camera.position), f3(prev_camera.direction), f3(prev_camera.up), prev_camera.focalDistance, prev_camera.lensRadius)
        pp = None
        if prev_prims is not None:
            if not isinstance(prev_prims, torch.Tensor):
                a = np.ascontiguousarray(prev_prims, dtype=scenes.TRIANGLE_DTYPE)
                prev_prims = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
            if prev_prims.device != dev or not prev_prims.is_contiguous() or prev_prims.numel() * prev_prims.element_size() % 40:
                raise ValueError(f"prev_prims: a contiguous tensor of 40-byte records on {dev}")
            pp = prev_prims.data_ptr()
        res = {"motion": torch.zeros((self.H, self.W, 2), dtype=torch.float32, device=dev), "prev_depth": torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)}
        mi = MotionIn(prim.data_ptr(), geom.data_ptr(), C.cast(C.pointer(cam), P), pp)
        mo = MotionOut(res["motion"].data_ptr(), res["prev_depth"].data_ptr())
        if chain is None:
            self._on_stream(stream, lambda h: self.L.tyr_render_motion(self.h, C.byref(mi), C.byref(mo), h), True)
        else:
            via = MotionChainIn(chain.data_ptr(), length0.data_ptr())
            self._on_stream(stream, lambda h: self.L.tyr_render_motion_chain(self.h, C.byref(mi), C.byref(via), C.byref(mo), h), True)
        if stream is not None:
            for t in res.values():
                t.record_stream(stream)
            if pp is not None:
                prev_prims.record_stream(stream)
            if chain is not None:
                chain.record_stream(stream), length0.record_stream(stream)
        return res

    def temporal(self, albedo, normal, depth, motion, prev_depth, accum=None, max_history=TEMPORAL_MAX_HISTORY, depth_tolerance=TEMPORAL_DEPTH_TOLERANCE,
                 normal_cos=TEMPORAL_NORMAL_COS, reset=False, want_history_len=False, stream=None):
        """tyr_temporal: blend this frame into the ctx's reprojected history.  albedo, normal (H, W, 3), depth (H, W) from
        render_aov, motion (H, W, 2), prev_depth (H, W) from render_motion, accum (H, W, 4; None: this ctx's blit buffer):
        contiguous float32 tensors on this ctx's device.  Returns the (H, W, 4) float32 frame in the blit buffer's layout with one
        sample per pixel (denoise's accum), and with want_history_len=True also the (H, W) history lengths.  reset=True discards
        the history first.  Runs on `stream` (default: torch's current stream) and returns without waiting for it."""
        tin = TemporalIn(*self._frame_inputs(accum=accum, albedo=albedo, normal=normal, depth=depth, motion=motion, prev_depth=prev_depth))
        prm = TemporalParams(max_history, depth_tolerance, normal_cos, TYR_TEMPORAL_RESET if reset else 0)
        out, hl = self._frame_outputs(4, 0 if want_history_len else None)
        self._frame_call("tyr_temporal", stream, C.byref(tin), C.byref(prm), out, hl)
        return (out, hl) if want_history_len else out

    def svgf(self, albedo, normal, depth, motion, prev_depth, accum=None, max_history=SVGF_MAX_HISTORY, depth_tolerance=SVGF_DEPTH_TOLERANCE,
             normal_cos=SVGF_NORMAL_COS, passes=SVGF_PASSES, sigma_luminance=SVGF_SIGMA_LUMINANCE, sigma_depth=SVGF_SIGMA_DEPTH,
             normal_power_log2=SVGF_NORMAL_POWER_LOG2, reset=False, resolve=False, want_variance=False, stream=None):
        """tyr_svgf: variance-guided spatiotemporal filtering of this frame against the ctx's own SVGF history.  The inputs are
        temporal's: albedo, normal (H, W, 3), depth (H, W) from render_aov, motion (H, W, 2), prev_depth (H, W) from
        render_motion, accum (H, W, 4; None: this ctx's blit buffer), contiguous float32 tensors on this ctx's device.  Returns
        the (H, W, 4) float32 filtered frame in the blit buffer's layout with one sample per pixel (with resolve=True tone-mapped
        as resolve_into writes it), and with want_variance=True also the (H, W) variance estimate.  reset=True discards the
        history first.  Runs on `stream` (default: torch's current stream) and returns without waiting for it."""
        sin = SvgfIn(*self._frame_inputs(accum=accum, albedo=albedo, normal=normal, depth=depth, motion=motion, prev_depth=prev_depth))
        flags = (TYR_SVGF_RESET if reset else 0) | (TYR_SVGF_RESOLVE if resolve else 0)
        prm = SvgfParams(max_history, depth_tolerance, normal_cos, passes, sigma_luminance, sigma_depth, normal_power_log2, flags)
        out, var = self._frame_outputs(4, 0 if want_variance else None)
        self._frame_call("tyr_svgf", stream, C.byref(sin), C.byref(prm), out, var)
        return (out, var) if want_variance else out

    def taa(self, color, depth, motion, prev_depth, alpha=TAA_ALPHA, gamma=TAA_GAMMA, bilinear=False, reset=False, out=None, stream=None):
        """tyr_taa: temporal anti-aliasing of a resolved frame against the ctx's own history of its outputs.  color (H, W, 4): a
        resolved frame (resolve_into's, or denoise's / svgf's with resolve=True); depth (H, W) from render_aov; motion
        (H, W, 2), prev_depth (H, W) from render_motion: contiguous float32 tensors on this ctx's device.  Returns the (H, W, 4)
        float32 frame: `out` when given (it may be `color` itself: in place), else a new tensor.  bilinear=True samples the
        history with four taps instead of the 4 x 4 Catmull-Rom kernel; reset=True discards the history first.  Runs on
        `stream` (default: torch's current stream) and returns without waiting for it."""
        tin = TaaIn(*self._frame_inputs(color=color, depth=depth, motion=motion, prev_depth=prev_depth, out=out)[:4])
        prm = TaaParams(alpha, gamma, (TYR_TAA_RESET if reset else 0) | (TYR_TAA_BILINEAR if bilinear else 0))
        if out is None:
            (out,) = self._frame_outputs(4)
        self._frame_call("tyr_taa", stream, C.byref(tin), C.byref(prm), out)
        return out

    # ---- adaptive sampling (include/tyr_c.h "Adaptive sampling") ----

    def _frame_map(self, a, dtype, what):
        """a (H, W) map as a contiguous tensor of `dtype` on this ctx's device: torch tensors of that dtype are taken as they are,
        numpy arrays are copied over on the current stream"""
        import torch

        dev = torch.device("cuda", self.device)
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32 if dtype == torch.int32 else np.float32, copy=False))).to(dev)
        if a.dtype != dtype or a.device != dev or not a.is_contiguous() or a.numel() != self.H * self.W:
            raise ValueError(f"{what}: a contiguous ({self.H}, {self.W}) {dtype} tensor on {dev}")
        return a

    def set_sample_map(self, spp_map, stream=None) -> int:
        """tyr_set_sample_map: build the ticket list of an (H, W) int32 sample map (torch tensor on this ctx's device, or numpy)
        and enter mapped mode (budget = the map's sum T over this ctx's rows).  The map is read after the work on `stream`
        (default: torch's current stream).  Returns T."""
        import torch

        m = self._frame_map(spp_map, torch.int32, "spp_map")
        total = c_u64(0)
        self._on_stream(stream, lambda h: self.L.tyr_set_sample_map(self.h, m.data_ptr(), h, C.byref(total)), True, "tyr_set_sample_map")
        return total.value

    def render_adaptive(self, spp_map, max_iterations=0xFFFFFFFF, stream=None) -> int:
        """tyr_render_adaptive: set_sample_map(spp_map), then render's loop on that budget.  Returns the iterations."""
        import torch

        m = self._frame_map(spp_map, torch.int32, "spp_map")
        it = c_u32(0)
        self._on_stream(stream, lambda h: self.L.tyr_render_adaptive(self.h, m.data_ptr(), h, max_iterations, C.byref(it)), True, "tyr_render_adaptive")
        return it.value

    def allocate_samples(self, error, total, min_spp=ADAPTIVE_MIN_SPP, max_spp=ADAPTIVE_MAX_SPP, stream=None):
        """tyr_allocate_samples: an (H, W) float32 error estimate (torch tensor on this ctx's device, or numpy) -> (sample map, its
        sum): an (H, W) int32 tensor (a sharded ctx writes its own rows; the others are 0) and the sum over this ctx's rows.
        The map spends exactly max(total, min_spp * P) samples unless some pixel reaches max_spp."""
        import torch

        e = self._frame_map(error, torch.float32, "error")
        prm = AllocateParams(int(total), int(min_spp), int(max_spp))
        (out,) = self._frame_outputs(0, dtype=torch.int32, zero=True)
        got = c_u64(0)
        self._frame_call("tyr_allocate_samples", stream, e.data_ptr(), C.byref(prm), out, C.byref(got))
        return out, got.value


def vecmath_probe(op: int, a: np.ndarray, b: np.ndarray, c: np.ndarray, device: int = 0) -> np.ndarray:
    """hip/vecmath.hpp function `op` on the device over float3 arrays (op codes: oracle/ref_harness.cpp ref_glm)"""
    a, b, c = (np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3) for x in (a, b, c))
    out = np.zeros_like(a)
    _check(lib().tyr_vecmath_probe(device, op, _ptr(a), _ptr(b), _ptr(c), a.shape[0], _ptr(out)), "tyr_vecmath_probe")
    return out


def contract_probe(op: int, a: np.ndarray, b: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """tyr_vecmath_probe's own ops (32-52: hip/detmath.hpp, the samplers and the winding numbers' binary64 building blocks,
    listed at contract_probe in hip/frame.hip) over
    (n, 3) arrays of 32-bit words -- float32, or uint32 where the op reads seeds -- into (n, 3) uint32 words"""
    a, b = (np.ascontiguousarray(x).reshape(-1, 3) for x in (a, a if b is None else b))
    assert all(x.dtype in (np.float32, np.uint32) for x in (a, b)) and a.shape == b.shape and 32 <= op <= 52
    out = np.zeros(a.shape, dtype=np.uint32)
    _check(lib().tyr_vecmath_probe(device, op, _ptr(a), _ptr(b), _ptr(a), a.shape[0], _ptr(out)), "tyr_vecmath_probe")
    return out


# ---- multi-GPU combine (RCCL behind the C ABI) --------------------------------------------------


class InputState(C.Structure):
    """tyr_input_state: what Camera::handle_input reads from the GLFW window (camera.cpp:3-44)"""

    _fields_ = [("key_w", C.c_uint8), ("key_s", C.c_uint8), ("key_a", C.c_uint8), ("key_d", C.c_uint8), ("key_space", C.c_uint8), ("key_left_control", C.c_uint8), ("key_left_shift", C.c_uint8),
                ("key_left_alt", C.c_uint8), ("cursor_x", C.c_double), ("cursor_y", C.c_double), ("window_w", c_i32), ("window_h", c_i32)]


class CameraPose(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("up", C.c_float * 3), ("horizontal_angle", C.c_double), ("vertical_angle", C.c_double)]


def camera_handle_input(pose: "CameraPose", state: "InputState", delta: float):
    _check(lib().tyr_camera_handle_input(C.byref(pose), C.byref(state), float(delta)), "tyr_camera_handle_input")


SUN_PARAM_FIELDS = (("sunDirection", 3), ("sunAngularDiameterCos", 1), ("sunE", 1), ("rayleighAtX", 3), ("mieAtX", 3), ("totalLightAtX", 3), ("mixFactor", 1), ("coneDir", 3), ("coneO1", 3), ("coneO2", 3), ("coneExtent", 1))


def sun_setup(sun_x: float, sun_y: float) -> dict:
    """the library's per-sun-change constants (host code; no GPU needed)"""
    out = np.zeros(25, dtype=np.float32)
    _check(lib().tyr_sun_setup(sun_x, sun_y, _ptr(out)), "tyr_sun_setup")
    res, k = {}, 0
    for name, n in SUN_PARAM_FIELDS:
        res[name] = out[k : k + n].copy() if n > 1 else out[k]
        k += n
    return res


def sunsky_probe(which: int, sun_position, dirs: np.ndarray, device: int = 0) -> np.ndarray:
    """sun / sky / sunsky (which 0 / 1 / 2) of the device code over float3 directions"""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(d)
    _check(lib().tyr_sunsky_probe(device, float(sun_position[0]), float(sun_position[1]), which, _ptr(d), d.shape[0], _ptr(out)), "tyr_sunsky_probe")
    return out


def cone_probe(sun_position, seed: int, n: int, device: int = 0):
    """n sun-cone samples of the device code along one xorshift stream; returns (samples[n][3], seed after)"""
    inp = np.array([seed], dtype=np.uint32).view(np.float32)
    out = np.zeros(3 * n + 1, dtype=np.float32)
    _check(lib().tyr_sunsky_probe(device, float(sun_position[0]), float(sun_position[1]), 3, _ptr(inp), n, _ptr(out)), "tyr_sunsky_probe")
    return out[: 3 * n].reshape(n, 3).copy(), int(out[3 * n : 3 * n + 1].view(np.uint32)[0])


def primary_window_probe(cam, width: int, height: int, root_min, root_max, rank: int = 0, nranks: int = 1, inset: int = 0) -> dict:
    """The camera window (tyr_primary_window_probe) of any camera, frame, sharding and root box; no ctx, no device."""
    f3 = lambda x: (c_f * 3)(*[float(v) for v in x])  # noqa: E731
    c = CameraC(f3(cam.position), f3(cam.direction), f3(cam.up), cam.focalDistance, cam.lensRadius)
    w = PrimaryWindowInfo()
    _check(lib().tyr_primary_window_probe(C.byref(c), width, height, rank, nranks, f3(root_min), f3(root_max), inset, C.byref(w)), "tyr_primary_window_probe")
    return {k: int(getattr(w, k)) for k, _ in w._fields_}


def dist_unique_id() -> bytes:
    """ncclGetUniqueId through the library: 128 opaque bytes that rank 0 hands to the other ranks"""
    buf = (C.c_char * TYR_DIST_ID_BYTES)()
    _check(lib().tyr_dist_unique_id(buf), "tyr_dist_unique_id")
    return bytes(buf)


def dist_owned_rows(height: int, rank: int, nranks: int):
    first, n = c_u32(0), c_u32(0)
    _check(lib().tyr_dist_owned_rows(height, rank, nranks, C.byref(first), C.byref(n)), "tyr_dist_owned_rows")
    return first.value, n.value


def dist_row_owner(y: int, nranks: int):
    r, yl = c_u32(0), c_u32(0)
    _check(lib().tyr_dist_row_owner(y, nranks, C.byref(r), C.byref(yl)), "tyr_dist_row_owner")
    return r.value, yl.value


class Dist:
    """one tyr_dist: the RCCL communicator of a Renderer (same rank / nranks as its pixel shard)"""

    def __init__(self, renderer: "Renderer", unique_id: bytes, rank: int, nranks: int):
        assert len(unique_id) == TYR_DIST_ID_BYTES
        self.L = renderer.L
        self.r = renderer  # keeps the ctx alive
        h = P()
        _check(self.L.tyr_dist_create(C.byref(h), renderer.h, unique_id, rank, nranks), "tyr_dist_create")
        self.h = h
        renderer._dists.append(self)  # Renderer.close() closes its communicators first (a combine reads the ctx)

    def combine(self, frame_out_device_ptr, mode=TYR_DIST_GATHER, root=0):
        _check(self.L.tyr_dist_combine(self.h, mode, root, frame_out_device_ptr), "tyr_dist_combine")

    def info(self) -> dict:
        n, r = c_i32(-1), c_i32(-1)
        _check(self.L.tyr_dist_info(self.h, C.byref(n), C.byref(r)), "tyr_dist_info")
        return {"comm_ranks": int(n.value), "rank": int(r.value)}

    def wait(self):
        _check(self.L.tyr_dist_wait(self.h), "tyr_dist_wait")

    def close(self):
        if getattr(self, "h", None):
            self.L.tyr_dist_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
