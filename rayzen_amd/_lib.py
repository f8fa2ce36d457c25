"""ctypes loaders for the in-tree shared libraries.

There is no CPU fallback for rendering: if librayzen_hip.so is missing or has
no GPU to talk to, the calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.environ.get("RAYZEN_HIP_SO") or os.path.join(_HERE, "lib", "librayzen_hip.so")   # override: A/B builds
HOST_SO = os.path.join(_HERE, "lib", "librayzen_host.so")

# the symbols include/rayzen_hip.h declares
HIP_SYMBOLS = (
    "rz_create", "rz_destroy", "rz_last_error", "rz_upload", "rz_update", "rz_update_transforms", "rz_build_blas", "rz_build_geometry", "rz_read_binding",
    "rz_set_frame", "rz_set_stream",
    "rz_bind_accum", "rz_render", "rz_render_counted", "rz_sync", "rz_clear_accum", "rz_read_accum",
    "rz_resolve_rgba8", "rz_present", "rz_last_render_ms", "rz_render_history_ms", "rz_last_kernel_name", "rz_accum_device_ptr", "rz_version", "rz_sizeof",
    "rz_debug_fail_alloc", "rz_debug_read_layout", "rz_debug_last_plan", "rz_source_hash", "rz_stream_handle", "rz_device_count",
    "rz_group_rccl_version", "rz_group_unique_id", "rz_group_create", "rz_group_create_rank", "rz_group_destroy",
    "rz_group_last_error", "rz_group_size", "rz_group_local_count", "rz_group_rank", "rz_group_ctx", "rz_group_upload",
    "rz_group_update", "rz_group_set_frame", "rz_group_render", "rz_group_reduce", "rz_group_sync", "rz_group_read_frame",
    "rz_group_frame_device_ptr", "rz_group_last_reduce_ms", "rz_group_transport", "rz_group_set_transport", "rz_abi_version", "rz_debug_poke_backstop", "rz_math_flavour",
    "rz_trace_rays", "rz_shadow_rays", "rz_render_editor", "rz_denoise", "rz_present_denoised", "rz_refit_geometry",
    "rz_denoise_temporal", "rz_present_temporal", "rz_temporal_reset", "rz_debug_read_temporal",
    "rz_display", "rz_present_display", "rz_display_reset", "rz_display_state",
    "rz_skin_create", "rz_skin_pose", "rz_skin_destroy", "rz_skin_last_kernel_ms",
    "rz_geometry_quality", "rz_rebuild_geometry",
    "rz_upscale", "rz_present_upscaled", "rz_upscale_seethrough", "rz_present_upscaled_seethrough",
    "rz_antialias", "rz_present_antialiased", "rz_antialias_seethrough", "rz_present_antialiased_seethrough",
    "rz_render_cost", "rz_cost_view", "rz_present_cost",
    "rz_coverage", "rz_outline",
    "rz_ambient_occlusion", "rz_ao_directions",
    "rz_render_adaptive", "rz_adaptive_plan",
    "rz_draw_lines",
    "rz_bloom", "rz_present_bloomed",
)
ABI_VERSION = 5         # RZ_ABI_VERSION of the include/rayzen_hip.h this file mirrors
# the symbols include/rayzen_host.h declares
HOST_SYMBOLS = (
    "rzh_load_obj", "rzh_build_blas", "rzh_build_tlas", "rzh_world_bounds", "rzh_scene_create",
    "rzh_scene_destroy", "rzh_scene_add_mesh", "rzh_scene_add_object", "rzh_scene_set_transform",
    "rzh_scene_build", "rzh_scene_set_blas_builder", "rzh_scene_update_dynamic", "rzh_scene_buffer", "rzh_scene_depths",
    "rzh_scene_save_cache", "rzh_scene_load_cache", "rzh_scene_build_cached",
    "rzh_camera_matrices", "rzh_mat_translate", "rzh_mat_scale", "rzh_mat_rotate", "rzh_mat_inverse",
    "rzh_make_cube", "rzh_make_blob", "rzh_version", "rzh_refit_blas", "rzh_scene_refit_mesh", "rzh_skin_triangles",
    "rzh_blas_sah_cost", "rzh_scene_rebuild_mesh",
)


class FrameParams(C.Structure):
    """rz_frame_params of include/rayzen_hip.h."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("inv_view", C.c_float * 16), ("inv_proj", C.c_float * 16),
                ("view", C.c_float * 16), ("proj", C.c_float * 16),
                ("cam_pos", C.c_float * 3),
                ("num_lights", C.c_int32), ("bounce_budget", C.c_int32),
                ("spp", C.c_int32), ("sample_base", C.c_int32),
                ("tile_rank", C.c_int32), ("tile_nranks", C.c_int32)]


COUNTER_FIELDS = ("samples", "traversals", "tlas_nodes", "tlas_leaf_indices", "instances",
                  "blas_nodes", "triangles", "materials", "light_fetches", "pixels",
                  "scatters", "diffuse_scatters", "hemi_draws", "lit_lights", "triangles_past_u")


class PresentParams(C.Structure):
    """rz_present_params of include/rayzen_hip.h."""
    _fields_ = [("fps", C.c_float), ("show_fps", C.c_int32), ("show_lights", C.c_int32), ("show_bvh", C.c_int32),
                ("bvh_mode", C.c_int32), ("selected_blas", C.c_int32), ("selected_tri", C.c_int32)]


class BvhNode(C.Structure):
    """rz_bvh_node of include/rayzen_hip.h."""
    _fields_ = [("boundsMin", C.c_float * 3), ("leftFirst", C.c_int32), ("boundsMax", C.c_float * 3), ("count", C.c_int32)]


class MeshBuild(C.Structure):
    """rz_mesh_build of include/rayzen_hip.h."""
    _fields_ = [("first_triangle", C.c_size_t), ("n_triangles", C.c_size_t), ("node_offset", C.c_int32),
                ("index_offset", C.c_int32), ("n_nodes", C.c_int32), ("depth", C.c_int32), ("root", BvhNode)]


class LaunchPlan(C.Structure):
    """rz_launch_plan of include/rayzen_hip.h."""
    _fields_ = [("groups", C.c_int64), ("grid", C.c_int64), ("per_claim", C.c_int32), ("claim_units", C.c_int32),
                ("batches_per_pixel", C.c_int32), ("pixels_per_wave", C.c_int32), ("lds_stack_entries", C.c_int32),
                ("overflow_entries", C.c_int32), ("transparent", C.c_int32), ("scratch_mib", C.c_int32)]


class Ray(C.Structure):
    """rz_ray of include/rayzen_hip.h (32 B)."""
    _fields_ = [("origin", C.c_float * 3), ("max_dist", C.c_float), ("dir", C.c_float * 3), ("reserved", C.c_uint32)]


class Hit(C.Structure):
    """rz_hit of include/rayzen_hip.h (48 B)."""
    _fields_ = [("t", C.c_float), ("point", C.c_float * 3), ("normal", C.c_float * 3), ("material", C.c_int32),
                ("instance", C.c_int32), ("triangle", C.c_int32), ("prim", C.c_int32), ("reserved", C.c_int32)]


class Visibility(C.Structure):
    """rz_visibility of include/rayzen_hip.h (8 B)."""
    _fields_ = [("visibility", C.c_float), ("lit", C.c_int32)]


RAYS_HOST, RAYS_INCOHERENT = 1, 2       # RZ_RAYS_HOST, RZ_RAYS_INCOHERENT


class EditorParams(C.Structure):
    """rz_editor_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("ambient", C.c_float * 3), ("pad0", C.c_float), ("clear", C.c_float * 4)]


EDITOR_HOST, EDITOR_INCOHERENT = 1, 2   # RZ_EDITOR_HOST, RZ_EDITOR_INCOHERENT


class DenoiseParams(C.Structure):
    """rz_denoise_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("demodulate", C.c_int32), ("reserved", C.c_int32 * 3)]


DENOISE_HOST = 1                        # RZ_DENOISE_HOST


class TemporalParams(C.Structure):
    """rz_temporal_params of include/rayzen_hip.h (64 B)."""
    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_int32), ("normal_cos", C.c_float),
                ("plane_tol", C.c_float), ("iterations", C.c_int32), ("sigma_l", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_plane", C.c_float), ("demodulate", C.c_int32), ("reserved", C.c_int32 * 6)]


TEMPORAL_DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9, plane_tol=2.0, iterations=5, sigma_l=0.5,
                         sigma_normal=128.0, sigma_plane=1.0, demodulate=1)
TEMPORAL_HOST, TEMPORAL_KEEP = 1, 4     # RZ_TEMPORAL_HOST, RZ_TEMPORAL_KEEP
REFIT_HOST = 1                          # RZ_REFIT_HOST


class DisplayParams(C.Structure):
    """rz_display_params of include/rayzen_hip.h (64 B)."""
    _fields_ = [("exposure_mode", C.c_int32), ("exposure", C.c_float), ("key", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float), ("low_permille", C.c_int32), ("high_permille", C.c_int32),
                ("curve", C.c_int32), ("white", C.c_float), ("transfer", C.c_int32), ("reserved", C.c_int32 * 5)]


class DisplayInfo(C.Structure):
    """rz_display_info of include/rayzen_hip.h (536 B)."""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("log2_mean", C.c_float), ("counted", C.c_uint32),
                ("below", C.c_uint32), ("above", C.c_uint32), ("histogram", C.c_uint32 * 128)]


DISPLAY_HOST, DISPLAY_KEEP = 1, 4       # RZ_DISPLAY_HOST, RZ_DISPLAY_KEEP
DISPLAY_CURVES = {"clamp": 0, "reinhard": 1, "aces": 2}
DISPLAY_TRANSFERS = {"linear": 0, "srgb": 1}
DISPLAY_SOURCES = {"accum": 0, "denoise": 1, "temporal": 2}


class UpscaleParams(C.Structure):
    """rz_upscale_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("factor", C.c_int32), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("demodulate", C.c_int32),
                ("reserved", C.c_int32 * 4)]


UPSCALE_DEFAULTS = dict(factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=1)
UPSCALE_HOST = 1                        # RZ_UPSCALE_HOST
SIZEOF_UPSCALE_PARAMS = 21              # its rz_sizeof index


class SeethroughParams(C.Structure):
    """rz_seethrough_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("max_depth", C.c_int32), ("reserved", C.c_int32 * 7)]


class Chain(C.Structure):
    """rz_chain of include/rayzen_hip.h (16 B)."""
    _fields_ = [("throughput", C.c_float * 3), ("word", C.c_int32)]


# rz_chain as a numpy record: word = k | (m_first + 1) << 8, 0 for a primary miss
CHAIN_DTYPE = np.dtype([("throughput", np.float32, (3,)), ("word", np.int32)])
SEETHROUGH_DEFAULTS = dict(max_depth=8)
SEETHROUGH_MAX_DEPTH = 8
SIZEOF_SEETHROUGH_PARAMS, SIZEOF_CHAIN = 23, 24     # their rz_sizeof indices


class AntialiasParams(C.Structure):
    """rz_antialias_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("factor", C.c_int32), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("demodulate", C.c_int32),
                ("edge_normal", C.c_float), ("edge_plane", C.c_float), ("reserved", C.c_int32 * 2)]


ANTIALIAS_DEFAULTS = dict(factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=1, edge_normal=0.9, edge_plane=1.0)
ANTIALIAS_HOST = 1                      # RZ_ANTIALIAS_HOST
SIZEOF_ANTIALIAS_PARAMS = 26            # its rz_sizeof index


class PixelCost(C.Structure):
    """rz_pixel_cost of include/rayzen_hip.h (32 B)."""
    _fields_ = [(n, C.c_uint32) for n in ("traversals", "tlas_nodes", "tlas_leaf_indices", "instances", "blas_nodes", "triangles",
                                          "materials", "light_fetches")]


class CostParams(C.Structure):
    """rz_cost_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("spp", C.c_int32), ("reserved", C.c_int32 * 7)]


class CostViewParams(C.Structure):
    """rz_cost_view_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("metric", C.c_int32), ("curve", C.c_int32), ("scale", C.c_float), ("reserved", C.c_int32 * 5)]


class CostStats(C.Structure):
    """rz_cost_stats of include/rayzen_hip.h (32 B)."""
    _fields_ = [("max_value", C.c_uint64), ("sum_value", C.c_uint64), ("max_x", C.c_int32), ("max_y", C.c_int32),
                ("scale_used", C.c_float), ("reserved", C.c_int32)]


# rz_pixel_cost as a numpy record
PIXEL_COST_DTYPE = np.dtype([(n, np.uint32) for n, _ in PixelCost._fields_])
COST_DEFAULTS = dict(spp=0)
COST_VIEW_DEFAULTS = dict(metric=0, curve=0, scale=0.0)
COST_METRICS = {"bytes": 0, "nodes": 1, "triangles": 2, "traversals": 3, "instances": 4}
COST_CURVES = {"linear": 0, "log": 1}
COST_HOST = 1                           # RZ_COST_HOST
SIZEOF_PIXEL_COST, SIZEOF_COST_PARAMS, SIZEOF_COST_VIEW_PARAMS, SIZEOF_COST_STATS = 28, 29, 30, 31    # their rz_sizeof indices


class CoverageParams(C.Structure):
    """rz_coverage_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("reserved", C.c_int32 * 4)]


class InstanceCoverage(C.Structure):
    """rz_instance_coverage of include/rayzen_hip.h (32 B)."""
    _fields_ = [("pixels", C.c_uint32), ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_max", C.c_int32), ("y_max", C.c_int32),
                ("t_min", C.c_float), ("t_max", C.c_float), ("reserved", C.c_uint32)]


class OutlineParams(C.Structure):
    """rz_outline_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("color", C.c_float * 3), ("alpha", C.c_float),
                ("reserved", C.c_int32)]


# rz_instance_coverage as a numpy record
INSTANCE_COVERAGE_DTYPE = np.dtype([("pixels", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"), ("y_max", "<i4"),
                                    ("t_min", "<f4"), ("t_max", "<f4"), ("reserved", "<u4")])
COVERAGE_HOST = OUTLINE_HOST = 1        # RZ_COVERAGE_HOST, RZ_OUTLINE_HOST
SIZEOF_COVERAGE_PARAMS, SIZEOF_INSTANCE_COVERAGE, SIZEOF_OUTLINE_PARAMS = 33, 34, 35      # their rz_sizeof indices


class AoParams(C.Structure):
    """rz_ao_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("samples", C.c_int32), ("radius", C.c_float), ("smooth", C.c_int32), ("strength", C.c_float),
                ("normal_cos", C.c_float), ("plane_tol", C.c_float), ("reserved", C.c_int32 * 2)]


AO_HOST = 1                             # RZ_AO_HOST
AO_DIRECTIONS = 256                     # points of rz_ao_directions' table
SIZEOF_AO_PARAMS = 37                   # its rz_sizeof index (36 is unassigned)


class AdaptiveParams(C.Structure):
    """rz_adaptive_params of include/rayzen_hip.h (32 B); a zero field = its default."""
    _fields_ = [("batch_spp", C.c_int32), ("min_batches", C.c_int32), ("max_batches", C.c_int32), ("threshold", C.c_float),
                ("luminance_floor", C.c_float), ("merge_gap", C.c_int32), ("max_runs", C.c_int32), ("flags", C.c_uint32)]


ADAPTIVE_MAX_BATCHES = 64               # RZ_ADAPTIVE_MAX_BATCHES


class AdaptiveInfo(C.Structure):
    """rz_adaptive_info of include/rayzen_hip.h (800 B)."""
    _fields_ = [("batches", C.c_int32), ("n_tiles", C.c_int32), ("samples_traced", C.c_uint64), ("samples_uniform", C.c_uint64),
                ("render_ms", C.c_float), ("meter_ms", C.c_float), ("tiles_active", C.c_int32 * ADAPTIVE_MAX_BATCHES),
                ("tiles_rendered", C.c_int32 * ADAPTIVE_MAX_BATCHES), ("runs", C.c_int32 * ADAPTIVE_MAX_BATCHES)]


TILE_RUN_DTYPE = np.dtype([("first", np.int32), ("len", np.int32)])     # rz_tile_run (8 B)
ADAPTIVE_HOST = 1                       # RZ_ADAPTIVE_HOST
ADAPTIVE_DEFAULTS = dict(batch_spp=8, min_batches=4, max_batches=8, threshold=0.02, luminance_floor=0.01, merge_gap=8, max_runs=1)
SIZEOF_ADAPTIVE_PARAMS, SIZEOF_ADAPTIVE_INFO, SIZEOF_TILE_RUN = 38, 39, 40      # their rz_sizeof indices


class LinesParams(C.Structure):
    """rz_lines_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("width", C.c_float), ("near_w", C.c_float), ("depth_bias", C.c_float), ("hidden_alpha", C.c_float),
                ("smooth", C.c_int32), ("reserved", C.c_int32 * 3)]


# rz_line as a numpy record: color = bytes r, g, b, alpha in memory order; instance < 0 = world space
LINE_DTYPE = np.dtype([("a", "<f4", 3), ("color", "u1", 4), ("b", "<f4", 3), ("instance", "<i4")])
LINES_DEFAULTS = dict(width=1.5, near_w=0.01, depth_bias=2.0 ** -8, hidden_alpha=0.0, smooth=0)
LINES_HOST = 1                          # RZ_LINES_HOST
LINES_MAX = 1 << 20                     # lines per call
SIZEOF_LINE, SIZEOF_LINES_PARAMS = 42, 43       # their rz_sizeof indices (41 is unassigned)


class BloomParams(C.Structure):
    """rz_bloom_params of include/rayzen_hip.h (32 B)."""
    _fields_ = [("threshold", C.c_float), ("knee", C.c_float), ("limit", C.c_float), ("intensity", C.c_float),
                ("spread", C.c_float), ("levels", C.c_int32), ("reserved", C.c_int32 * 2)]


BLOOM_DEFAULTS = dict(threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6)
BLOOM_HOST = 1                          # RZ_BLOOM_HOST
BLOOM_MAX_LEVELS = 8
SIZEOF_BLOOM_PARAMS = 45                # its rz_sizeof index (44 is unassigned)


class SkinTriangle(C.Structure):
    """rz_skin_triangle of include/rayzen_hip.h (64 B)."""
    _fields_ = [("bones", C.c_uint32 * 3), ("pad", C.c_uint32), ("weights", (C.c_float * 4) * 3)]


class MorphTriangle(C.Structure):
    """rz_morph_triangle of include/rayzen_hip.h (48 B)."""
    _fields_ = [("d", (C.c_float * 4) * 3)]


SKIN_DEVICE_ARGS = 1                    # RZ_SKIN_DEVICE_ARGS
SIZEOF_SKIN_TRIANGLE, SIZEOF_MORPH_TRIANGLE = 17, 18    # their rz_sizeof indices


class MeshQuality(C.Structure):
    """rz_mesh_quality of include/rayzen_hip.h (64 B)."""
    _fields_ = [("node_offset", C.c_int32), ("index_offset", C.c_int32), ("tri_offset", C.c_int32), ("node_offset_before", C.c_int32),
                ("n_triangles", C.c_int32), ("n_nodes", C.c_int32), ("depth", C.c_int32), ("flags", C.c_uint32),
                ("sah_cost", C.c_double), ("sah_cost_built", C.c_double), ("sah_cost_before", C.c_double), ("reserved", C.c_double)]


QUALITY_REBUILT = 1                     # RZ_QUALITY_REBUILT
SIZEOF_MESH_QUALITY = 20                # its rz_sizeof index


class Counters(C.Structure):
    """rz_counters of include/rayzen_hip.h."""
    _fields_ = [(n, C.c_uint64) for n in COUNTER_FIELDS]


_hip = None
_host = None


def hip():
    """librayzen_hip.so with prototypes set.  Raises if it has not been built."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise RuntimeError(f"{HIP_SO} is missing: run `python -m rayzen_amd.build` (needs hipcc). "
                               "There is no CPU fallback for the render path.")
        L = C.CDLL(HIP_SO)
        vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
        L.rz_create.restype, L.rz_create.argtypes = vp, [i, C.c_uint]
        L.rz_destroy.restype, L.rz_destroy.argtypes = None, [vp]
        L.rz_last_error.restype, L.rz_last_error.argtypes = C.c_char_p, [vp]
        L.rz_upload.restype, L.rz_upload.argtypes = i, [vp, i, vp, sz]
        L.rz_update.restype, L.rz_update.argtypes = i, [vp, i, sz, vp, sz]
        L.rz_update_transforms.restype, L.rz_update_transforms.argtypes = i, [vp, vp, sz]
        L.rz_read_binding.restype, L.rz_read_binding.argtypes = i, [vp, i, vp, sz, C.POINTER(sz)]
        L.rz_build_blas.restype, L.rz_build_blas.argtypes = i, [vp, vp, sz, vp, sz, vp, C.POINTER(sz), C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.rz_build_geometry.restype, L.rz_build_geometry.argtypes = i, [vp, vp, sz, C.POINTER(MeshBuild), sz]
        L.rz_set_frame.restype, L.rz_set_frame.argtypes = i, [vp, C.POINTER(FrameParams)]
        L.rz_set_stream.restype, L.rz_set_stream.argtypes = i, [vp, vp]
        L.rz_bind_accum.restype, L.rz_bind_accum.argtypes = i, [vp, vp, sz]
        L.rz_render.restype, L.rz_render.argtypes = i, [vp]
        L.rz_render_counted.restype, L.rz_render_counted.argtypes = i, [vp, C.POINTER(Counters)]
        L.rz_sync.restype, L.rz_sync.argtypes = i, [vp]
        L.rz_clear_accum.restype, L.rz_clear_accum.argtypes = i, [vp]
        L.rz_read_accum.restype, L.rz_read_accum.argtypes = i, [vp, vp, sz]
        L.rz_resolve_rgba8.restype, L.rz_resolve_rgba8.argtypes = i, [vp, vp, sz]
        L.rz_present.restype, L.rz_present.argtypes = i, [vp, C.POINTER(PresentParams), vp, sz, vp, sz]
        L.rz_last_render_ms.restype, L.rz_last_render_ms.argtypes = i, [vp, C.POINTER(C.c_float), C.POINTER(i)]
        L.rz_render_history_ms.restype, L.rz_render_history_ms.argtypes = i, [vp, C.POINTER(C.c_float), i]
        L.rz_last_kernel_name.restype, L.rz_last_kernel_name.argtypes = C.c_char_p, [vp]
        L.rz_accum_device_ptr.restype, L.rz_accum_device_ptr.argtypes = vp, [vp]
        L.rz_version.restype, L.rz_version.argtypes = C.c_char_p, []
        L.rz_sizeof.restype, L.rz_sizeof.argtypes = sz, [i]
        L.rz_debug_fail_alloc.restype, L.rz_debug_fail_alloc.argtypes = i, [vp, i]
        L.rz_debug_read_layout.restype, L.rz_debug_read_layout.argtypes = i, [vp, i, vp, sz, C.POINTER(sz)]
        L.rz_debug_last_plan.restype, L.rz_debug_last_plan.argtypes = i, [vp, C.POINTER(LaunchPlan)]
        L.rz_source_hash.restype, L.rz_source_hash.argtypes = C.c_char_p, []
        L.rz_stream_handle.restype, L.rz_stream_handle.argtypes = vp, [vp]
        L.rz_device_count.restype, L.rz_device_count.argtypes = i, []
        L.rz_group_rccl_version.restype, L.rz_group_rccl_version.argtypes = i, [C.POINTER(i)]
        L.rz_group_unique_id.restype, L.rz_group_unique_id.argtypes = i, [vp]
        L.rz_group_create.restype, L.rz_group_create.argtypes = vp, [i, C.POINTER(i), C.c_uint]
        L.rz_group_create_rank.restype, L.rz_group_create_rank.argtypes = vp, [i, i, i, vp, C.c_uint]
        L.rz_group_destroy.restype, L.rz_group_destroy.argtypes = None, [vp]
        L.rz_group_last_error.restype, L.rz_group_last_error.argtypes = C.c_char_p, [vp]
        L.rz_group_size.restype, L.rz_group_size.argtypes = i, [vp]
        L.rz_group_local_count.restype, L.rz_group_local_count.argtypes = i, [vp]
        L.rz_group_rank.restype, L.rz_group_rank.argtypes = i, [vp, i]
        L.rz_group_ctx.restype, L.rz_group_ctx.argtypes = vp, [vp, i]
        L.rz_group_upload.restype, L.rz_group_upload.argtypes = i, [vp, i, vp, sz]
        L.rz_group_update.restype, L.rz_group_update.argtypes = i, [vp, i, sz, vp, sz]
        L.rz_group_set_frame.restype, L.rz_group_set_frame.argtypes = i, [vp, C.POINTER(FrameParams)]
        L.rz_group_render.restype, L.rz_group_render.argtypes = i, [vp]
        L.rz_group_reduce.restype, L.rz_group_reduce.argtypes = i, [vp, i]
        L.rz_group_sync.restype, L.rz_group_sync.argtypes = i, [vp]
        L.rz_group_read_frame.restype, L.rz_group_read_frame.argtypes = i, [vp, vp, sz]
        L.rz_group_frame_device_ptr.restype, L.rz_group_frame_device_ptr.argtypes = vp, [vp]
        # (each in a try of its own: an A/B library built from an older revision (RAYZEN_HIP_SO) may lack any ONE of them, and
        #  everything else must still work -- ADVICE r4)
        for name, res, args in (("rz_group_last_reduce_ms", i, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
                                ("rz_group_transport", C.c_char_p, [vp]),
                                ("rz_group_set_transport", i, [vp, C.c_char_p]),
                                ("rz_abi_version", i, []), ("rz_debug_poke_backstop", i, [vp, C.c_uint]), ("rz_math_flavour", i, []),
                                ("rz_trace_rays", i, [vp, vp, vp, sz, C.c_uint]), ("rz_shadow_rays", i, [vp, vp, vp, sz, C.c_uint]),
                                ("rz_render_editor", i, [vp, C.POINTER(FrameParams), vp, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_denoise", i, [vp, vp, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_denoised", i, [vp, C.POINTER(PresentParams), vp, vp, sz, vp, sz]),
                                ("rz_refit_geometry", i, [vp, vp, sz, sz, C.c_uint]),
                                ("rz_denoise_temporal", i, [vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_temporal", i, [vp, C.POINTER(PresentParams), vp, vp, sz, vp, sz]),
                                ("rz_temporal_reset", i, [vp]),
                                ("rz_debug_read_temporal", i, [vp, i, vp, sz, C.POINTER(sz)]),
                                ("rz_display", i, [vp, vp, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_display", i, [vp, C.POINTER(PresentParams), vp, i, vp, vp, sz, vp, sz]),
                                ("rz_display_reset", i, [vp]),
                                ("rz_display_state", i, [vp, C.POINTER(DisplayInfo)]),
                                ("rz_skin_create", i, [vp, sz, sz, vp, vp, i, vp, i, C.POINTER(i)]),
                                ("rz_skin_pose", i, [vp, i, vp, vp, C.c_uint]),
                                ("rz_skin_destroy", i, [vp, i]),
                                ("rz_skin_last_kernel_ms", i, [vp, C.POINTER(C.c_float)]),
                                ("rz_geometry_quality", i, [vp, vp, sz, C.POINTER(sz)]),
                                ("rz_rebuild_geometry", i, [vp, C.c_double, vp, sz, C.POINTER(sz), C.c_uint]),
                                ("rz_upscale", i, [vp, vp, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_upscaled", i, [vp, C.POINTER(PresentParams), vp, vp, i, vp, vp, sz, vp, sz]),
                                ("rz_upscale_seethrough", i, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_upscaled_seethrough", i, [vp, C.POINTER(PresentParams), vp, vp, vp, i, vp, vp, sz, vp, sz]),
                                ("rz_antialias", i, [vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_antialiased", i, [vp, C.POINTER(PresentParams), vp, vp, i, vp, vp, sz, vp, sz]),
                                ("rz_antialias_seethrough", i, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_antialiased_seethrough", i, [vp, C.POINTER(PresentParams), vp, vp, vp, i, vp, vp, sz, vp, sz]),
                                ("rz_render_cost", i, [vp, vp, vp, sz, C.POINTER(Counters), C.c_uint]),
                                ("rz_cost_view", i, [vp, vp, vp, sz, vp, sz, vp, C.c_uint]),
                                ("rz_present_cost", i, [vp, C.POINTER(PresentParams), vp, vp, sz, vp, sz]),
                                ("rz_coverage", i, [vp, C.POINTER(FrameParams), vp, vp, sz, vp, sz, C.c_uint]),
                                ("rz_outline", i, [vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_ambient_occlusion", i, [vp, C.POINTER(FrameParams), vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_ao_directions", i, [vp, sz]),
                                ("rz_render_adaptive", i, [vp, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveInfo), vp, sz, vp, sz]),
                                ("rz_adaptive_plan", i, [vp, vp, sz, i, i, vp, sz, C.POINTER(sz)]),
                                ("rz_draw_lines", i, [vp, C.POINTER(FrameParams), vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_bloom", i, [vp, vp, vp, sz, vp, sz, vp, sz, C.c_uint]),
                                ("rz_present_bloomed", i, [vp, C.POINTER(PresentParams), vp, vp, i, vp, vp, sz, vp, sz])):
            try:
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
            except AttributeError:
                if not os.environ.get("RAYZEN_HIP_SO"):
                    raise
        # the structs this file mirrors are the ones of ABI revision ABI_VERSION (include/rayzen_hip.h: RZ_ABI_VERSION)
        if hasattr(L, "rz_abi_version") and L.rz_abi_version() != ABI_VERSION and not os.environ.get("RAYZEN_HIP_SO"):
            raise RuntimeError(f"{HIP_SO} speaks ABI revision {L.rz_abi_version()}, this binding {ABI_VERSION}: rebuild (python -m rayzen_amd.build)")
        _hip = L
    return _hip


def host():
    """librayzen_host.so with prototypes set."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_SO):
            raise RuntimeError(f"{HOST_SO} is missing: run `python -m rayzen_amd.build`")
        L = C.CDLL(HOST_SO)
        vp, i, sz, f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
        L.rzh_load_obj.restype, L.rzh_load_obj.argtypes = i, [C.c_char_p, i, vp, i]
        L.rzh_build_blas.restype, L.rzh_build_blas.argtypes = i, [vp, i, vp, vp, C.POINTER(i)]
        L.rzh_build_tlas.restype, L.rzh_build_tlas.argtypes = i, [vp, i, vp, vp, C.POINTER(i)]
        L.rzh_refit_blas.restype, L.rzh_refit_blas.argtypes = i, [vp, i, vp, i, vp]
        L.rzh_scene_refit_mesh.restype, L.rzh_scene_refit_mesh.argtypes = i, [vp, i, vp, i]
        L.rzh_blas_sah_cost.restype, L.rzh_blas_sah_cost.argtypes = C.c_double, [vp, i]
        L.rzh_scene_rebuild_mesh.restype, L.rzh_scene_rebuild_mesh.argtypes = i, [vp, i]
        L.rzh_skin_triangles.restype, L.rzh_skin_triangles.argtypes = i, [vp, vp, i, vp, i, vp, vp, i, vp]
        L.rzh_world_bounds.restype, L.rzh_world_bounds.argtypes = None, [vp, vp, vp, vp]
        L.rzh_scene_create.restype, L.rzh_scene_create.argtypes = vp, []
        L.rzh_scene_destroy.restype, L.rzh_scene_destroy.argtypes = None, [vp]
        L.rzh_scene_add_mesh.restype, L.rzh_scene_add_mesh.argtypes = i, [vp, vp, i]
        L.rzh_scene_add_object.restype, L.rzh_scene_add_object.argtypes = i, [vp, i, vp]
        L.rzh_scene_set_transform.restype, L.rzh_scene_set_transform.argtypes = i, [vp, i, vp]
        L.rzh_scene_build.restype, L.rzh_scene_build.argtypes = i, [vp, i]
        L.rzh_scene_set_blas_builder.restype, L.rzh_scene_set_blas_builder.argtypes = i, [vp, vp, vp]
        L.rzh_scene_update_dynamic.restype, L.rzh_scene_update_dynamic.argtypes = i, [vp]
        L.rzh_scene_buffer.restype, L.rzh_scene_buffer.argtypes = vp, [vp, i, C.POINTER(sz)]
        L.rzh_scene_save_cache.restype, L.rzh_scene_save_cache.argtypes = i, [vp, C.c_char_p]
        L.rzh_scene_load_cache.restype, L.rzh_scene_load_cache.argtypes = i, [vp, C.c_char_p]
        L.rzh_scene_build_cached.restype, L.rzh_scene_build_cached.argtypes = i, [vp, C.c_char_p, i, C.POINTER(i * 5)]
        L.rzh_scene_depths.restype, L.rzh_scene_depths.argtypes = None, [vp, C.POINTER(i), C.POINTER(i)]
        L.rzh_camera_matrices.restype = None
        L.rzh_camera_matrices.argtypes = [vp, vp, vp, f, f, f, f, vp, vp, vp, vp]
        for n in ("rzh_mat_translate", "rzh_mat_scale"):
            getattr(L, n).restype, getattr(L, n).argtypes = None, [vp, vp, vp]
        L.rzh_mat_rotate.restype, L.rzh_mat_rotate.argtypes = None, [vp, f, vp, vp]
        L.rzh_mat_inverse.restype, L.rzh_mat_inverse.argtypes = None, [vp, vp]
        L.rzh_make_cube.restype, L.rzh_make_cube.argtypes = i, [i, vp, i]
        L.rzh_make_blob.restype, L.rzh_make_blob.argtypes = i, [i, f, C.c_uint, i, vp, i]
        L.rzh_version.restype, L.rzh_version.argtypes = C.c_char_p, []
        _host = L
    return _host
