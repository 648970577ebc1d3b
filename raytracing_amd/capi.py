"""ctypes binding of the C-ABI in include/rt_hip.h (raytracing_amd/librt_hip.so).

Python here is plumbing for tests and bench.py; the product is the shared
library.  There is NO fallback: if the library is missing or no GPU is present
the constructors raise."""
import ctypes as C
import os
import numpy as np
from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librt_hip.so")
_lib = None


class RtError(RuntimeError):
    """Mirrors the reference's CLException (src/utils/cl_exception.hpp:109-123)."""


class rt_stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("samples", C.c_uint64),
                ("last_active", C.c_uint32 * 64), ("last_shadow", C.c_uint32 * 64),
                ("samples_in_flight", C.c_uint32), ("samples_in_flight_limit", C.c_uint32), ("path_state_bytes", C.c_uint64),
                ("stack_spills", C.c_uint32), ("slow_rays", C.c_uint32), ("chunk_pixels", C.c_uint32), ("pipelines", C.c_uint32),
                ("log_inline_entries", C.c_uint32), ("log_fallbacks", C.c_uint32), ("frame_kernel_samples", C.c_uint32), ("samples_ahead", C.c_uint32), ("samples_from_banks", C.c_uint64),
                ("fused_raygen_launches", C.c_uint64)]


class rt_profile(C.Structure):
    _fields_ = [("ms_raygen", C.c_double), ("ms_trace_closest", C.c_double), ("ms_shade", C.c_double),
                ("ms_trace_shadow", C.c_double), ("n_raygen", C.c_uint32), ("n_trace_closest", C.c_uint32),
                ("n_shade", C.c_uint32), ("n_trace_shadow", C.c_uint32)]


class rt_scene_desc(C.Structure):
    _fields_ = [("triangles", C.c_void_p), ("num_triangles", C.c_uint32),
                ("nodes", C.c_void_p), ("num_nodes", C.c_uint32),
                ("materials", C.c_void_p), ("num_materials", C.c_uint32),
                ("textures", C.c_void_p), ("num_textures", C.c_uint32),
                ("texture_data", C.c_void_p), ("num_texture_data", C.c_uint32),
                ("lights", C.c_void_p), ("num_lights", C.c_uint32),
                ("emissive_indices", C.c_void_p), ("num_emissive", C.c_uint32),
                ("env_rgba", C.c_void_p), ("env_width", C.c_uint32), ("env_height", C.c_uint32),
                ("material_texture_indices", C.c_void_p), ("flags", C.c_uint32)]


SCENE_EMISSIVE_NEE = 1


class rt_frame_desc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tile_rank", C.c_uint32),
                ("tile_count", C.c_uint32), ("band_height", C.c_uint32)]


class rt_filter_desc(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


FILTER_DEMODULATE = 1
FILTER_DEFAULT = dict(iterations=2, flags=FILTER_DEMODULATE, sigma_color=8.0, sigma_normal=0.05, sigma_depth=0.1)   # RT_FILTER_DESC_DEFAULT


def filter_desc(desc=None, **kw):
    """an rt_filter_desc from None (the header's defaults), a dict, keywords or an rt_filter_desc"""
    if isinstance(desc, rt_filter_desc):
        return desc
    v = dict(FILTER_DEFAULT)
    v.update(desc or {})
    v.update(kw)
    return rt_filter_desc(v["iterations"], v["flags"], v["sigma_color"], v["sigma_normal"], v["sigma_depth"])


class rt_temporal_filter_desc(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("alpha_color", C.c_float), ("alpha_moments", C.c_float),
                ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


# RT_TEMPORAL_FILTER_DESC_DEFAULT
TEMPORAL_FILTER_DEFAULT = dict(iterations=5, flags=FILTER_DEMODULATE, alpha_color=0.2, alpha_moments=0.2, sigma_luminance=2.0, sigma_normal=0.05,
                               sigma_depth=0.1)


def temporal_filter_desc(desc=None, **kw):
    """an rt_temporal_filter_desc from None (the header's defaults), a dict, keywords or an rt_temporal_filter_desc"""
    if isinstance(desc, rt_temporal_filter_desc):
        return desc
    v = dict(TEMPORAL_FILTER_DEFAULT)
    v.update(desc or {})
    v.update(kw)
    return rt_temporal_filter_desc(*(v[k] for k, _ in rt_temporal_filter_desc._fields_))


EXPORTS = [
    "rt_ctx_create", "rt_ctx_destroy", "rt_finish", "rt_last_error", "rt_ctx_device_info", "rt_ctx_stream",
    "rt_ctx_set_option", "rt_upload_blue_noise_tables", "rt_host_register", "rt_host_unregister",
    "rt_buffer_create", "rt_buffer_destroy", "rt_buffer_write", "rt_buffer_read", "rt_buffer_copy",
    "rt_buffer_device_ptr", "rt_buffer_size", "rt_scene_upload", "rt_frame_create", "rt_frame_destroy",
    "rt_frame_local_rows", "rt_frame_global_row", "rt_set_option", "rt_set_camera", "rt_reset",
    "rt_generate_rays", "rt_intersect", "rt_shade_miss", "rt_clear_outgoing_counter", "rt_clear_shadow_counter",
    "rt_shade", "rt_intersect_shadow", "rt_accumulate_direct", "rt_advance_sample", "rt_integrate",
    "rt_frame_reserve_samples",
    "rt_compute_aovs", "rt_denoise", "rt_copy_history",
    "rt_frame_resolve", "rt_frame_present", "rt_frame_present_wait", "rt_frame_read_radiance", "rt_frame_radiance_device_ptr", "rt_frame_sample_count",
    "rt_frame_get_stats", "rt_frame_get_profile", "rt_frame_copy_radiance", "rt_frame_debug_read_queue", "rt_frame_debug_read_hits", "rt_debug_eval",
    "rt_debug_wide_bvh", "rt_frame_debug_timeline", "rt_frame_debug_frame_rows", "rt_debug_own_bvh", "rt_debug_wide_bvh_metric", "rt_scene_tree_report", "rt_debug_choose_tree", "rt_debug_adapt_fold", "rt_debug_fold_abandon", "rt_debug_adapt_shadow_side", "rt_debug_rotate_tree", "rt_debug_fold_view_left", "rt_debug_device_fold", "rt_debug_wide_bvh_weights", "rt_debug_pair_layout", "rt_debug_check_folds", "rt_debug_device_tree", "rt_debug_count_box_passes", "rt_scene_export_folds", "rt_scene_import_folds",
    "rt_group_create", "rt_group_unique_id", "rt_group_join", "rt_group_size", "rt_group_local_count", "rt_group_local_rank", "rt_group_comm_count",
    "rt_group_gather_radiance", "rt_group_destroy", "rt_group_last_error", "rt_group_denoise", "rt_group_create_local",
    "rt_group_create_unchecked",
    "rt_frame_filter", "rt_frame_read_guides", "rt_debug_filter",
    "rt_frame_filter_temporal", "rt_frame_filter_history_reset", "rt_frame_read_filter_history", "rt_debug_filter_temporal",
    "rt_scene_refit", "rt_scene_refit_buffer", "rt_debug_refit",
    "rt_scene_set_objects", "rt_scene_pose", "rt_debug_pose",
    "rt_scene_set_skin", "rt_scene_skin", "rt_debug_skin",
    "rt_scene_set_morph", "rt_scene_morph", "rt_scene_morph_skin", "rt_debug_morph", "rt_debug_morph_skin",
    "rt_frame_read_guide_motion", "rt_debug_guide_motion", "rt_debug_filter_temporal_motion",
    "rt_scene_trace", "rt_scene_trace_buffer", "rt_frame_pick", "rt_debug_query_surface",
    "rt_scene_bake", "rt_scene_bake_buffer", "rt_debug_bake_rays", "rt_debug_bake_reduce",
    "rt_scene_light_bake", "rt_scene_light_bake_buffer", "rt_scene_atlas_bake_light", "rt_debug_light_bake_rays", "rt_debug_light_bake_reduce",
    "rt_scene_atlas", "rt_scene_atlas_buffer", "rt_scene_atlas_surfaces", "rt_scene_atlas_surfaces_buffer", "rt_scene_atlas_bake", "rt_debug_atlas",
    "rt_scene_nearest", "rt_scene_nearest_buffer", "rt_debug_nearest", "rt_debug_nearest_walk",
    "rt_scene_trace_all", "rt_scene_trace_all_buffer", "rt_frame_pick_all", "rt_debug_trace_all",
    "rt_scene_within", "rt_scene_within_buffer", "rt_debug_within", "rt_debug_within_walk",
    "rt_scene_overlap", "rt_scene_overlap_buffer", "rt_debug_overlap", "rt_debug_overlap_walk",
    "rt_scene_select", "rt_scene_select_buffer", "rt_debug_select", "rt_frame_pick_rect", "rt_debug_rect_region",
    "rt_scene_cross", "rt_scene_cross_buffer", "rt_scene_cross_self", "rt_scene_cross_self_buffer",
    "rt_debug_cross", "rt_debug_cross_walk", "rt_debug_cross_self",
    "rt_scene_separation", "rt_scene_separation_buffer", "rt_scene_separation_self", "rt_scene_separation_self_buffer",
    "rt_debug_separation", "rt_debug_separation_walk", "rt_debug_separation_self",
]

OPT_MAX_BOUNCES, OPT_WHITE_FURNACE, OPT_SAMPLER, OPT_AOV, OPT_DENOISER, OPT_DROP_LAST, OPT_PROFILE, OPT_TRACE_VARIANT, OPT_TRACE_WAVES, OPT_SAMPLES_IN_FLIGHT, OPT_SELECT_FORM_BOX, OPT_PACKET_BOUNCES, OPT_TRACE_TUNE, OPT_DEBUG_ALLOC_LIMIT, OPT_PATH_STATE_LIMIT_MB, OPT_PIPELINES, OPT_SHADE_PARTITION, OPT_OVERLAP_SHADOW, OPT_SMALL_LAUNCH_PATHS, OPT_COMPACT_LOG, OPT_DEBUG_LOG_POOL_DIV, OPT_TRACE_TAIL_LANES, OPT_TRACE_TAIL_PATHS, OPT_CHUNK_REFILL, OPT_STAGE_PIPES, OPT_FRAME_KERNEL, OPT_SAMPLES_AHEAD, OPT_FUSED_RAYGEN = range(28)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError("librt_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(LIB_PATH)
    vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
    sig = {
        "rt_ctx_create": (i32, [i32, C.POINTER(vp)]), "rt_ctx_destroy": (i32, [vp]), "rt_finish": (i32, [vp]),
        "rt_last_error": (C.c_char_p, [vp]),
        "rt_ctx_device_info": (i32, [vp, C.c_char_p, sz, C.POINTER(i32), C.POINTER(sz)]),
        "rt_ctx_stream": (vp, [vp]), "rt_ctx_set_option": (i32, [vp, i32, u32]),
        "rt_upload_blue_noise_tables": (i32, [vp, vp, vp, vp]),
        "rt_host_register": (i32, [vp, vp, sz]), "rt_host_unregister": (i32, [vp, vp]),
        "rt_buffer_create": (i32, [vp, sz, vp, C.POINTER(vp)]), "rt_buffer_destroy": (i32, [vp]),
        "rt_buffer_write": (i32, [vp, sz, vp, sz]), "rt_buffer_read": (i32, [vp, sz, vp, sz]),
        "rt_buffer_copy": (i32, [vp, vp, sz, sz, sz]), "rt_buffer_device_ptr": (vp, [vp]),
        "rt_buffer_size": (sz, [vp]),
        "rt_scene_upload": (i32, [vp, C.POINTER(rt_scene_desc)]),
        "rt_frame_create": (i32, [vp, C.POINTER(rt_frame_desc), C.POINTER(vp)]), "rt_frame_destroy": (i32, [vp]),
        "rt_frame_local_rows": (u32, [vp]), "rt_frame_global_row": (u32, [vp, u32]),
        "rt_set_option": (i32, [vp, i32, u32]), "rt_set_camera": (i32, [vp, vp]),
        "rt_reset": (i32, [vp]), "rt_generate_rays": (i32, [vp]), "rt_intersect": (i32, [vp, u32]),
        "rt_shade_miss": (i32, [vp, u32]), "rt_clear_outgoing_counter": (i32, [vp, u32]),
        "rt_clear_shadow_counter": (i32, [vp]), "rt_shade": (i32, [vp, u32]),
        "rt_intersect_shadow": (i32, [vp, u32]), "rt_accumulate_direct": (i32, [vp]),
        "rt_advance_sample": (i32, [vp]), "rt_integrate": (i32, [vp, u32]),
        "rt_frame_reserve_samples": (i32, [vp, u32, C.POINTER(C.c_uint32)]),
        "rt_compute_aovs": (i32, [vp]), "rt_denoise": (i32, [vp]), "rt_copy_history": (i32, [vp]),
        "rt_frame_resolve": (i32, [vp, vp]), "rt_frame_present": (i32, [vp, vp]), "rt_frame_present_wait": (i32, [vp]),
        "rt_frame_read_radiance": (i32, [vp, vp]),
        "rt_frame_radiance_device_ptr": (vp, [vp]), "rt_frame_sample_count": (u32, [vp]),
        "rt_frame_get_stats": (i32, [vp, C.POINTER(rt_stats)]),
        "rt_frame_get_profile": (i32, [vp, C.POINTER(rt_profile)]),
        "rt_frame_copy_radiance": (i32, [vp, vp]),
        "rt_frame_debug_read_queue": (i32, [vp, i32, u32, vp, vp, vp, u32, C.POINTER(u32)]),
        "rt_frame_debug_read_hits": (i32, [vp, vp, u32]),
        "rt_debug_eval": (i32, [vp, i32, vp, vp, vp, u32]),
        "rt_debug_wide_bvh": (i32, [vp, u32, i32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        "rt_frame_debug_timeline": (i32, [vp, i32, vp]),
        "rt_frame_debug_frame_rows": (i32, [vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        "rt_scene_tree_report": (C.c_char_p, [vp]),
        "rt_debug_choose_tree": (i32, [C.POINTER(rt_scene_desc), i32, u32, vp, u32, C.POINTER(u32), C.POINTER(u32), C.c_char_p, sz]),
        "rt_debug_own_bvh": (i32, [vp, u32, C.c_double, vp, u32, vp, u32, C.POINTER(u32)]),
        "rt_debug_wide_bvh_metric": (i32, [vp, u32, C.c_double, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        "rt_debug_fold_view_left": (i32, [vp, vp, C.c_double]),
        "rt_debug_device_fold": (i32, [vp, vp, u32, C.c_double, vp, u32, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_double)]),
        "rt_debug_wide_bvh_weights": (i32, [vp, u32, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        "rt_debug_pair_layout": (i32, [vp, u32, vp, vp, u32]),
        "rt_debug_check_folds": (i32, [vp, u32, vp, u32, u32]),
        "rt_debug_device_tree": (i32, [vp, vp, u32, C.c_double, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(u32), u32, vp, C.c_double]),
        "rt_debug_count_box_passes": (i32, [vp, vp, u32, vp, vp, u32, vp, C.POINTER(C.c_ulonglong)]),
        "rt_scene_export_folds": (i32, [vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "rt_scene_import_folds": (i32, [vp, vp, u32, u32, vp, u32, u32]),
        "rt_debug_rotate_tree": (i32, [vp, u32, vp, vp, u32, i32, vp, C.POINTER(C.c_double), C.POINTER(u32), i32, C.c_double]),
        "rt_debug_adapt_shadow_side": (i32, [vp, u32, vp, vp, u32, u32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32), vp, C.POINTER(C.c_double), C.POINTER(u32), vp, u32, C.POINTER(u32)]),
        "rt_debug_fold_abandon": (C.c_double, [vp, u32, vp, vp, u32, u32, u32, C.POINTER(i32)]),
        "rt_debug_adapt_fold": (i32, [vp, u32, vp, vp, u32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(i32)]),
        "rt_group_create": (i32, [i32, C.POINTER(i32), C.POINTER(vp)]), "rt_group_create_unchecked": (i32, [i32, C.POINTER(i32), C.POINTER(vp)]),
        "rt_group_unique_id": (i32, [vp, sz]),
        "rt_group_join": (i32, [i32, i32, vp, i32, C.POINTER(vp)]), "rt_group_size": (i32, [vp]),
        "rt_group_local_count": (i32, [vp]), "rt_group_local_rank": (i32, [vp, i32]),
        "rt_group_comm_count": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
        "rt_group_gather_radiance": (i32, [vp, C.POINTER(vp), i32, vp, C.POINTER(vp)]), "rt_group_destroy": (i32, [vp]),
        "rt_group_last_error": (C.c_char_p, [vp]),
        "rt_group_denoise": (i32, [vp, C.POINTER(vp), i32, vp, vp]), "rt_group_create_local": (i32, [i32, i32, C.POINTER(vp)]),
        "rt_frame_filter": (i32, [vp, C.POINTER(rt_filter_desc), vp]),
        "rt_frame_read_guides": (i32, [vp, vp, vp, vp, C.POINTER(u32)]),
        "rt_debug_filter": (i32, [vp, u32, u32, vp, vp, vp, vp, C.POINTER(rt_filter_desc), vp]),
        "rt_frame_filter_temporal": (i32, [vp, C.POINTER(rt_temporal_filter_desc), vp]),
        "rt_frame_filter_history_reset": (i32, [vp]),
        "rt_frame_read_filter_history": (i32, [vp, vp, vp]),
        "rt_debug_filter_temporal": (i32, [vp, u32, u32, vp, vp] + [vp] * 8 + [C.POINTER(rt_temporal_filter_desc), vp, vp, vp]),
        "rt_scene_refit": (i32, [vp, vp, u32]), "rt_scene_refit_buffer": (i32, [vp, vp]),
        "rt_debug_refit": (i32, [vp, vp, u32, vp, u32, vp, u32, u32, vp, vp]),
        "rt_scene_set_objects": (i32, [vp, vp, u32, u32]), "rt_scene_pose": (i32, [vp, vp, u32]),
        "rt_debug_pose": (i32, [vp, vp, vp, u32, vp, u32, vp]),
        "rt_scene_set_skin": (i32, [vp, vp, u32, u32]), "rt_scene_skin": (i32, [vp, vp, u32]),
        "rt_debug_skin": (i32, [vp, vp, vp, u32, vp, u32, vp]),
        "rt_scene_set_morph": (i32, [vp, vp, vp, u32, u32]), "rt_scene_morph": (i32, [vp, vp, u32]), "rt_scene_morph_skin": (i32, [vp, vp, u32, vp, u32]),
        "rt_debug_morph": (i32, [vp, vp, vp, vp, u32, u32, vp, vp]), "rt_debug_morph_skin": (i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp]),
        "rt_frame_read_guide_motion": (i32, [vp, vp, vp]),
        "rt_debug_guide_motion": (i32, [vp, u32, vp, vp, u32, vp, vp]),
        "rt_debug_filter_temporal_motion": (i32, [vp, u32, u32, vp, vp] + [vp] * 10 + [C.POINTER(rt_temporal_filter_desc), vp, vp, vp]),
        "rt_scene_trace": (i32, [vp, vp, u32, u32, vp, vp, vp]), "rt_scene_trace_buffer": (i32, [vp, vp, u32, u32, vp, vp, vp]),
        "rt_frame_pick": (i32, [vp, u32, u32, vp, vp, vp]),
        "rt_debug_query_surface": (i32, [vp, vp, u32, vp, vp, vp, u32, vp]),
        "rt_scene_bake": (i32, [vp, vp, u32, C.POINTER(rt_bake_desc), vp]), "rt_scene_bake_buffer": (i32, [vp, vp, u32, C.POINTER(rt_bake_desc), vp]),
        "rt_debug_bake_rays": (i32, [vp, vp, u32, u32, C.POINTER(rt_bake_desc), vp]),
        "rt_debug_bake_reduce": (i32, [vp, vp, u32, u32, vp]),
        "rt_scene_light_bake": (i32, [vp, vp, u32, C.POINTER(rt_light_bake_desc), vp]), "rt_scene_light_bake_buffer": (i32, [vp, vp, u32, C.POINTER(rt_light_bake_desc), vp]),
        "rt_scene_atlas_bake_light": (i32, [vp, C.POINTER(rt_atlas_desc), vp, C.POINTER(rt_light_bake_desc), vp, vp, vp]),
        "rt_debug_light_bake_rays": (i32, [vp, vp, u32, u32, C.POINTER(rt_light_bake_desc), vp, u32, vp]),
        "rt_debug_light_bake_reduce": (i32, [vp, u32, u32, C.POINTER(rt_light_bake_desc), vp, u32, vp, u32, u32, vp, vp]),
        "rt_scene_atlas": (i32, [vp, C.POINTER(rt_atlas_desc), vp, vp, vp]), "rt_scene_atlas_buffer": (i32, [vp, C.POINTER(rt_atlas_desc), vp, vp, vp]),
        "rt_scene_atlas_surfaces": (i32, [vp, vp, u32, vp]), "rt_scene_atlas_surfaces_buffer": (i32, [vp, vp, u32, vp]),
        "rt_scene_atlas_bake": (i32, [vp, C.POINTER(rt_atlas_desc), vp, C.POINTER(rt_bake_desc), vp, vp, vp]),
        "rt_debug_atlas": (i32, [vp, vp, u32, vp, vp, C.POINTER(rt_atlas_desc), vp, vp]),
        "rt_scene_nearest": (i32, [vp, vp, u32, vp, vp]), "rt_scene_nearest_buffer": (i32, [vp, vp, u32, vp, vp]),
        "rt_debug_nearest": (i32, [vp, vp, u32, vp, u32, vp]),
        "rt_debug_nearest_walk": (i32, [vp, u32, vp, u32, i32, vp, u32, vp, vp]),
        "rt_scene_trace_all": (i32, [vp, vp, u32, u32, vp, vp, vp]), "rt_scene_trace_all_buffer": (i32, [vp, vp, u32, u32, vp, vp, vp]),
        "rt_frame_pick_all": (i32, [vp, u32, u32, u32, vp, vp, vp, vp]),
        "rt_debug_trace_all": (i32, [vp, vp, u32, vp, u32, vp, u32, u32, vp, vp]),
        "rt_scene_within": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]), "rt_scene_within_buffer": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]),
        "rt_debug_within": (i32, [vp, vp, u32, vp, u32, u32, u32, vp, vp]),
        "rt_debug_within_walk": (i32, [vp, u32, vp, u32, i32, vp, u32, u32, u32, vp, vp, vp]),
        "rt_scene_overlap": (i32, [vp, vp, u32, u32, vp, vp]), "rt_scene_overlap_buffer": (i32, [vp, vp, u32, u32, vp, vp]),
        "rt_debug_overlap": (i32, [vp, vp, u32, vp, u32, u32, vp, vp]),
        "rt_debug_overlap_walk": (i32, [vp, u32, vp, u32, i32, vp, u32, u32, vp, vp, vp]),
        "rt_scene_select": (i32, [vp, vp, u32, vp, vp, vp, vp]), "rt_scene_select_buffer": (i32, [vp, vp, u32, vp, vp, vp, vp]),
        "rt_debug_select": (i32, [vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp]),
        "rt_frame_pick_rect": (i32, [vp, u32, u32, u32, u32, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
        "rt_debug_rect_region": (i32, [vp, u32, u32, u32, u32, u32, u32, C.c_float, C.c_float, vp]),
        "rt_scene_cross": (i32, [vp, vp, u32, u32, u32, vp, vp]), "rt_scene_cross_buffer": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "rt_scene_cross_self": (i32, [vp, u32, u32, u32, u32, vp, vp]), "rt_scene_cross_self_buffer": (i32, [vp, u32, u32, u32, u32, vp, vp]),
        "rt_debug_cross": (i32, [vp, vp, u32, vp, u32, u32, u32, vp, vp]),
        "rt_debug_cross_walk": (i32, [vp, u32, vp, u32, i32, vp, u32, u32, u32, vp, vp, vp]),
        "rt_debug_cross_self": (i32, [vp, vp, u32, vp, u32, u32, u32, u32, vp, vp]),
        "rt_scene_separation": (i32, [vp, vp, u32, C.c_float, u32, vp]), "rt_scene_separation_buffer": (i32, [vp, vp, u32, C.c_float, u32, vp]),
        "rt_scene_separation_self": (i32, [vp, u32, u32, C.c_float, u32, vp]), "rt_scene_separation_self_buffer": (i32, [vp, u32, u32, C.c_float, u32, vp]),
        "rt_debug_separation": (i32, [vp, vp, u32, vp, u32, C.c_float, vp]),
        "rt_debug_separation_walk": (i32, [vp, u32, vp, u32, i32, vp, u32, C.c_float, vp, vp]),
        "rt_debug_separation_self": (i32, [vp, vp, u32, vp, u32, u32, C.c_float, u32, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check(lib, ctx, rc):
    if rc != 0:
        msg = lib.rt_last_error(ctx)
        raise RtError(msg.decode() if msg else "unknown error")


def debug_filter(ctx, hdr, albedo, normal, depth, desc=None):
    """rt_debug_filter: the spatial filter over caller arrays (hdr, albedo, normal: float32[h, w, 4]; depth: float32[h, w]) on ctx's GPU,
    or the host restatement when ctx is None.  Returns the filtered HDR image float32[h, w, 4]."""
    lib = load()
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w = hdr.shape[:2]
    alb, nrm = (np.ascontiguousarray(a, np.float32) for a in (albedo, normal))
    dep = np.ascontiguousarray(depth, np.float32)
    if alb.shape != hdr.shape or nrm.shape != hdr.shape or dep.shape != (h, w) or hdr.shape != (h, w, 4):
        raise ValueError("debug_filter: hdr, albedo, normal must be [h, w, 4], depth [h, w]")
    out = np.zeros_like(hdr)
    handle = ctx.handle if ctx is not None else None
    d = filter_desc(desc)
    if lib.rt_debug_filter(handle, w, h, hdr.ctypes.data, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data, C.byref(d), out.ctypes.data):
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_filter_temporal(ctx, cam, prev_cam, hdr, albedo, normal, depth, prev_normal, prev_depth, hist_color, hist_moments, desc=None):
    """rt_debug_filter_temporal: one call of the temporal filter over caller arrays (hdr, albedo, normal, prev_normal, hist_color, hist_moments:
    float32[h, w, 4]; depth, prev_depth: float32[h, w]; cam, prev_cam: types.camera, prev_cam None = a standing camera) on ctx's GPU, or the
    host restatement when ctx is None.  Returns (HDR image, colour history, moments history (mu1, mu2, L, 0)), each float32[h, w, 4]."""
    return _debug_filter_temporal(ctx, cam, prev_cam, hdr, albedo, normal, depth, prev_normal, prev_depth, hist_color, hist_moments, None, None, desc, False)


def debug_filter_temporal_motion(ctx, cam, prev_cam, hdr, albedo, normal, depth, prev_normal, prev_depth, hist_color, hist_moments, prev_position,
                                 prev_pose_normal, desc=None):
    """rt_debug_filter_temporal_motion: debug_filter_temporal with the motion images of moved geometry (prev_position float32[h, w, 4] = (where the
    pixel's first hit was at the previous call, 1), w 0 = no motion known; prev_pose_normal = (its unit normal there, 0)).  Either None: exactly
    debug_filter_temporal.  With both the history is reprojected even under a standing camera."""
    return _debug_filter_temporal(ctx, cam, prev_cam, hdr, albedo, normal, depth, prev_normal, prev_depth, hist_color, hist_moments, prev_position,
                                  prev_pose_normal, desc, True)


def debug_guide_motion(ctx, hits, prev_triangles):
    """rt_debug_guide_motion: per pixel of hits (float32[..., 4] = u, v, the primitive index's bits, unused; an index >= len(prev_triangles) = no hit)
    where the hit was in the pose prev_triangles (types.triangle) and its unit normal there: (float32[..., 4] = (X', 1), float32[..., 4] = (n', 0)),
    zeros without a hit.  ctx None = the host restatement, else the kernel on ctx's GPU."""
    lib = load()
    hits = np.ascontiguousarray(hits, np.float32)
    tris = np.ascontiguousarray(prev_triangles)
    if hits.shape[-1] != 4 or tris.dtype != T.triangle:
        raise ValueError("debug_guide_motion: hits must be [..., 4] float32, prev_triangles types.triangle")
    pos, nrm = np.zeros_like(hits), np.zeros_like(hits)
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_guide_motion(handle, hits.size // 4, hits.ctypes.data, tris.ctypes.data if len(tris) else None, len(tris), pos.ctypes.data,
                                 nrm.ctypes.data):
        raise RtError(lib.rt_last_error(handle).decode())
    return pos, nrm


def _debug_filter_temporal(ctx, cam, prev_cam, hdr, albedo, normal, depth, prev_normal, prev_depth, hist_color, hist_moments, prev_position,
                           prev_pose_normal, desc, motion_entry):
    lib = load()
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w = hdr.shape[:2]
    four = [np.ascontiguousarray(a, np.float32) for a in (albedo, normal, prev_normal, hist_color, hist_moments)]
    dep, pdep = (np.ascontiguousarray(a, np.float32) for a in (depth, prev_depth))
    if hdr.shape != (h, w, 4) or any(a.shape != hdr.shape for a in four) or dep.shape != (h, w) or pdep.shape != (h, w):
        raise ValueError("debug_filter_temporal: images must be [h, w, 4], depths [h, w]")
    alb, nrm, pnrm, hc, hm = four
    cam = np.ascontiguousarray(cam)
    pc = np.ascontiguousarray(prev_cam) if prev_cam is not None else None
    out, hc_out, hm_out = np.zeros_like(hdr), np.zeros_like(hdr), np.zeros_like(hdr)
    handle = ctx.handle if ctx is not None else None
    d = temporal_filter_desc(desc)
    head = (handle, w, h, cam.ctypes.data, pc.ctypes.data if pc is not None else None, hdr.ctypes.data, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data,
            pnrm.ctypes.data, pdep.ctypes.data, hc.ctypes.data, hm.ctypes.data)
    tail = (C.byref(d), out.ctypes.data, hc_out.ctypes.data, hm_out.ctypes.data)
    if motion_entry:
        pp, pn = (np.ascontiguousarray(a, np.float32) if a is not None else None for a in (prev_position, prev_pose_normal))
        if any(a is not None and a.shape != hdr.shape for a in (pp, pn)):
            raise ValueError("debug_filter_temporal_motion: the motion images must be [h, w, 4]")
        rc = lib.rt_debug_filter_temporal_motion(*head, pp.ctypes.data if pp is not None else None, pn.ctypes.data if pn is not None else None, *tail)
    else:
        rc = lib.rt_debug_filter_temporal(*head, *tail)
    if rc:
        raise RtError(lib.rt_last_error(handle).decode())
    return out, hc_out, hm_out


def debug_refit(ctx, nodes, triangles, records=None, entry=0):
    """rt_debug_refit: `nodes` (reference layout) and any fold of it (`records`: the 64-byte records as a structured or uint8 array, `entry`) refitted to
    `triangles` (same count and order).  ctx None = the host restatement, else refit.hip's kernels on ctx's GPU.
    Returns (nodes, records, disqualified): disqualified = a record no longer qualifies for k_trace_w4 (its bytes are left as they were)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    out_nodes = np.zeros_like(nodes)
    n_rec = 0 if records is None else len(records)
    recs = out_recs = None
    if n_rec:
        recs = np.ascontiguousarray(records)
        if recs.dtype.itemsize * (recs.size // n_rec) != 64:
            raise RtError("debug_refit: records must be 64 bytes each")
        out_recs = np.zeros_like(recs)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_refit(handle, nodes.ctypes.data, len(nodes), tris.ctypes.data, len(tris), recs.ctypes.data if n_rec else None, n_rec, entry,
                            out_nodes.ctypes.data, out_recs.ctypes.data if n_rec else None)
    if rc not in (0, 2):
        raise RtError(lib.rt_last_error(handle).decode())
    return out_nodes, out_recs, rc == 2


def _matrices3x4(matrices, who):
    m = np.ascontiguousarray(matrices, np.float32)
    if m.ndim == 2 and m.shape[1] == 12:
        m = m.reshape(-1, 3, 4)
    if m.ndim != 3 or m.shape[1:] != (3, 4):
        raise RtError(who + ": matrices must be float32[num_objects, 3, 4]")
    return m


def debug_pose(ctx, rest, object_of_triangle, matrices, num_objects=None):
    """rt_debug_pose: `rest` (types.triangle) with triangle i posed by matrices[object_of_triangle[i]] (float32[num_objects, 3, 4], row-major, the translation in
    the fourth column).  ctx None = the host restatement, else pose.hip's kernel on ctx's GPU.  Returns the posed triangles."""
    lib = load()
    tris = np.ascontiguousarray(rest, T.triangle)
    ids = np.ascontiguousarray(object_of_triangle, np.uint32)
    if ids.shape != (len(tris),):
        raise RtError("debug_pose: one object index per triangle")
    m = _matrices3x4(matrices, "debug_pose")
    out = np.zeros_like(tris)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_pose(handle, tris.ctypes.data, ids.ctypes.data, len(tris), m.ctypes.data, len(m) if num_objects is None else num_objects, out.ctypes.data)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


SKIN_LDS_BONES, SKIN_MAX_BONES = 128, 65536     # skin_host.h: the largest palette k_skin_triangles stages in LDS (above it: gathered through L1 / L2); the most bones


def _influences(per_corner, num_triangles, who):
    """types.skin_influence[3 * num_triangles], from that or from [num_triangles, 3] of it"""
    f = np.ascontiguousarray(per_corner)
    if f.dtype != T.skin_influence:
        raise RtError(who + ": influences must be types.skin_influence records (types.influences packs bones and weights)")
    f = f.reshape(-1)
    if num_triangles is not None and len(f) != 3 * num_triangles:
        raise RtError(who + ": three influences per triangle")
    if len(f) % 3:
        raise RtError(who + ": three influences per triangle")
    return f


def debug_skin(ctx, rest, influences, matrices, num_bones=None):
    """rt_debug_skin: `rest` (types.triangle) with corner c of triangle i blended by influences[3 i + c] (types.skin_influence; types.influences packs them)
    from the palette `matrices` (float32[num_bones, 3, 4], rt_scene_pose's layout).  ctx None = the host restatement, else skin.hip's kernel on ctx's GPU.
    Returns the skinned triangles."""
    lib = load()
    tris = np.ascontiguousarray(rest, T.triangle)
    f = _influences(influences, len(tris), "debug_skin")
    m = _matrices3x4(matrices, "debug_skin")
    out = np.zeros_like(tris)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_skin(handle, tris.ctypes.data, f.ctypes.data, len(tris), m.ctypes.data, len(m) if num_bones is None else num_bones, out.ctypes.data)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


MORPH_LDS_TARGETS, MORPH_MAX_TARGETS = 1024, 65536     # morph_host.h: the most weights k_morph_triangles stages in LDS (above it: gathered through L1 / L2); the most targets


def _morph_table(deltas, offsets, who):
    """(types.morph_delta[total], uint32[targets + 1]), as types.morph_targets makes them; a flat array of at least one delta's room, so that its address is never NULL"""
    d = np.ascontiguousarray(deltas)
    if d.dtype != T.morph_delta:
        raise RtError(who + ": deltas must be types.morph_delta records (types.morph_targets packs them)")
    d = d.reshape(-1)
    o = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
    if len(o) < 2:
        raise RtError(who + ": offsets must have one entry per target and one more")
    if int(o.max()) > len(d):
        raise RtError(who + ": an offset lies past the deltas")
    if len(d) == 0:
        d = np.zeros(1, T.morph_delta)              # a set with no deltas at all is legal
    return d, o


def _weights(weights, who, num_targets=None):
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if len(w) == 0:
        raise RtError(who + ": no weights")
    if num_targets is not None and len(w) != num_targets:
        raise RtError(who + ": one weight per target")
    return w


def debug_morph(ctx, rest, deltas, offsets, weights):
    """rt_debug_morph: `rest` (types.triangle) morphed by the sparse targets (deltas, offsets: types.morph_targets) with one weight per target.  ctx None = the
    host restatement, else morph.hip's k_morph_triangles on ctx's GPU.  Returns the morphed triangles."""
    lib = load()
    tris = np.ascontiguousarray(rest, T.triangle)
    d, o = _morph_table(deltas, offsets, "debug_morph")
    w = _weights(weights, "debug_morph", len(o) - 1)
    out = np.zeros_like(tris)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_morph(handle, tris.ctypes.data, d.ctypes.data, o.ctypes.data, len(o) - 1, len(tris), w.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_morph_skin(ctx, rest, deltas, offsets, weights, influences, matrices):
    """rt_debug_morph_skin: debug_morph's result skinned by debug_skin's rule.  ctx None = the host composition of the two restatements, else
    k_morph_skin_triangles' one pass on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(rest, T.triangle)
    d, o = _morph_table(deltas, offsets, "debug_morph_skin")
    w = _weights(weights, "debug_morph_skin", len(o) - 1)
    f = _influences(influences, len(tris), "debug_morph_skin")
    m = _matrices3x4(matrices, "debug_morph_skin")
    out = np.zeros_like(tris)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_morph_skin(handle, tris.ctypes.data, d.ctypes.data, o.ctypes.data, len(o) - 1, len(tris), w.ctypes.data,
                                 f.ctypes.data, m.ctypes.data, len(m), out.ctypes.data)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


QUERY_CLOSEST, QUERY_ANY_HIT = 0, 1
INVALID_ID = 0xFFFFFFFF


def ray_records(rays):
    """the one rule for a query's rays: types.ray records as they are, or float32[n, 8] = origin.xyz, t_min, direction.xyz, t_max per row"""
    a = np.asarray(rays)
    if a.dtype == T.ray:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise RtError("rays must be types.ray records or float32[n, 8] (origin.xyz, t_min, direction.xyz, t_max)")
    return a.view(T.ray).reshape(-1)


ALL_HITS_MAX = 8          # RT_ALL_HITS_MAX
RAY_HITS_WALKED = 1       # rt_ray_hits.flags bit 0
RAY_HITS_EXIT_SHIFT = 8   # rt_ray_hits.flags bit 8 + j: stored hit j is an exit


def debug_trace_all(ctx, nodes, triangles, rays, max_hits=ALL_HITS_MAX):
    """rt_debug_trace_all: (types.ray_hits[n], types.hit[n, max_hits]) of `rays` (ray_records' rule) by brute force over the leaves of `nodes`
    (types.bvh_node) and `triangles` (types.triangle) -- no tree walk.  ctx None = the host (csrc/all_hits.h), else k_all_hits_brute on ctx's GPU."""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    r = ray_records(rays)
    out = np.zeros(len(r), T.ray_hits)
    hits = np.zeros((len(r), max_hits), T.hit)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_trace_all(handle, nd.ctypes.data if len(nd) else None, len(nd), tris.ctypes.data if len(tris) else None, len(tris),
                                r.ctypes.data if len(r) else None, len(r), max_hits, out.ctypes.data if len(r) else None,
                                hits.ctypes.data if hits.size else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out, hits


def debug_query_surface(ctx, triangles, rays, hits, object_of_triangle=None):
    """rt_debug_query_surface: the surface records (types.surface) of `hits` (types.hit) of `rays` over `triangles` (types.triangle); object_of_triangle
    None = object 0xFFFFFFFF.  ctx None = the host restatement (csrc/query.h), else k_query_surface on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    r = ray_records(rays)
    h = np.ascontiguousarray(hits, T.hit)
    if len(r) != len(h):
        raise RtError("debug_query_surface: one hit per ray")
    ids = None
    if object_of_triangle is not None:
        ids = np.ascontiguousarray(object_of_triangle, np.uint32)
        if ids.shape != (len(tris),):
            raise RtError("debug_query_surface: one object index per triangle")
    out = np.zeros(len(r), T.surface)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_query_surface(handle, tris.ctypes.data if len(tris) else None, len(tris), ids.ctypes.data if ids is not None else None,
                                    r.ctypes.data if len(r) else None, h.ctypes.data if len(h) else None, len(r), out.ctypes.data if len(r) else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


BAKE_FROM_SURFACES = 1
BAKE_BIAS_DEFAULT, BAKE_RADIUS_DEFAULT = 1e-3, 1.0


class rt_bake_desc(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("bias", C.c_float), ("radius", C.c_float)]


def bake_points(points, from_surfaces=False):
    """the one rule for a bake's points: float32[n, 8] = position.xyz, -, normal.xyz, - per row; from_surfaces: types.surface records"""
    a = np.asarray(points)
    if from_surfaces:
        if a.dtype != T.surface:
            raise RtError("points must be types.surface records (from_surfaces)")
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise RtError("points must be float32[n, 8] (position.xyz, -, normal.xyz, -)")
    return a


def bake_desc(samples, seed=0, bias=BAKE_BIAS_DEFAULT, radius=BAKE_RADIUS_DEFAULT, from_surfaces=False, flags=None):
    return rt_bake_desc(int(samples), int(seed) & 0xFFFFFFFF, (BAKE_FROM_SURFACES if from_surfaces else 0) if flags is None else flags, bias, radius)


def debug_bake_rays(ctx, points, samples, seed=0, bias=BAKE_BIAS_DEFAULT, radius=BAKE_RADIUS_DEFAULT, from_surfaces=False, first_index=0):
    """rt_debug_bake_rays: the rays a bake walks, types.ray[n, samples] (a skipped point's are zeros); the index of points[0] is first_index.
    ctx None = the host restatement (csrc/bake.h), else k_bake_rays on ctx's GPU."""
    lib = load()
    pts = bake_points(points, from_surfaces)
    d = bake_desc(samples, seed, bias, radius, from_surfaces)
    n = len(pts)
    out = np.zeros((n, max(int(samples), 0)), T.ray)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_bake_rays(handle, pts.ctypes.data if n else None, n, first_index, C.byref(d), out.ctypes.data if out.size else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_bake_reduce(rays, occluded, samples):
    """rt_debug_bake_reduce (host only): types.bake_result[n] of types.ray[n, samples] and their verdicts uint32[n, samples], in bake.h's order"""
    lib = load()
    r = np.ascontiguousarray(rays, T.ray).reshape(-1)
    o = np.ascontiguousarray(occluded, np.uint32).reshape(-1)
    if samples <= 0 or len(r) % samples or len(o) != len(r):
        raise RtError("debug_bake_reduce: n * samples rays and one verdict per ray")
    n = len(r) // samples
    out = np.zeros(n, T.bake_result)
    rc = lib.rt_debug_bake_reduce(r.ctypes.data if n else None, o.ctypes.data if n else None, n, samples, out.ctypes.data if n else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return out


LIGHT_BAKE_NO_SKY, LIGHT_BAKE_NO_LIGHTS = 2, 4
LIGHT_BAKE_SKY_DISTANCE_DEFAULT = 20000.0          # RT_MAX_RENDER_DIST


class rt_light_bake_desc(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("bias", C.c_float), ("sky_distance", C.c_float)]


def light_bake_desc(samples, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT, from_surfaces=False, sky=True, lights=True, flags=None):
    """rt_light_bake_desc; sky / lights False: RT_LIGHT_BAKE_NO_SKY / RT_LIGHT_BAKE_NO_LIGHTS; flags: the word itself"""
    if flags is None:
        flags = (BAKE_FROM_SURFACES if from_surfaces else 0) | (0 if sky else LIGHT_BAKE_NO_SKY) | (0 if lights else LIGHT_BAKE_NO_LIGHTS)
    return rt_light_bake_desc(int(samples), int(seed) & 0xFFFFFFFF, flags, bias, sky_distance)


def _lights(lights):
    return np.ascontiguousarray(lights if lights is not None else np.zeros(0, T.light), T.light).reshape(-1)


def debug_light_bake_rays(ctx, points, samples, lights=None, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT, from_surfaces=False,
                          sky=True, use_lights=True, first_index=0):
    """rt_debug_light_bake_rays: the rays a light bake walks, types.ray[n, samples + len(lights)] (zeros for an item without a ray and for a skipped point); the
    index of points[0] is first_index.  ctx None = the host restatement (csrc/light_bake.h), else k_light_bake_rays on ctx's GPU."""
    lib = load()
    pts = bake_points(points, from_surfaces)
    lg = _lights(lights)
    d = light_bake_desc(samples, seed, bias, sky_distance, from_surfaces, sky, use_lights)
    n = len(pts)
    out = np.zeros((n, max(int(samples), 0) + len(lg)), T.ray)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_light_bake_rays(handle, pts.ctypes.data if n else None, n, first_index, C.byref(d), lg.ctypes.data if len(lg) else None, len(lg),
                                      out.ctypes.data if out.size else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_light_bake_reduce(points, samples, occluded, lights=None, env=None, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT,
                            from_surfaces=False, sky=True, use_lights=True, first_index=0):
    """rt_debug_light_bake_reduce (host only): types.light_bake_result[n] of the points and the verdicts uint32[n, samples + len(lights)] of their items, in
    light_bake.h's order.  env: float32[h, w, 4], the environment image (None only with sky=False)."""
    lib = load()
    pts = bake_points(points, from_surfaces)
    lg = _lights(lights)
    n = len(pts)
    o = np.ascontiguousarray(occluded, np.uint32).reshape(-1)
    if samples <= 0 or len(o) != n * (int(samples) + len(lg)):
        raise RtError("debug_light_bake_reduce: one verdict per item (n * (samples + lights))")
    e = None
    if env is not None:
        e = np.ascontiguousarray(env, np.float32)
        if e.ndim != 3 or e.shape[2] != 4:
            raise RtError("debug_light_bake_reduce: env must be float32[h, w, 4]")
    d = light_bake_desc(samples, seed, bias, sky_distance, from_surfaces, sky, use_lights)
    out = np.zeros(n, T.light_bake_result)
    rc = lib.rt_debug_light_bake_reduce(pts.ctypes.data if n else None, n, first_index, C.byref(d), lg.ctypes.data if len(lg) else None, len(lg),
                                        e.ctypes.data if e is not None else None, e.shape[1] if e is not None else 0, e.shape[0] if e is not None else 0,
                                        o.ctypes.data if n else None, out.ctypes.data if n else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return out


TEXEL_COVERED, TEXEL_GUTTER = 1, 2
ATLAS_MAX_SIDE, ATLAS_MAX_TEXELS, ATLAS_MAX_GUTTER = 16384, 1 << 26, 4


class rt_atlas_desc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("gutter", C.c_uint32), ("object", C.c_uint32)]


def atlas_desc(width, height, gutter=0, object=None):
    """rt_atlas_desc; object None = every triangle"""
    return rt_atlas_desc(int(width), int(height), int(gutter), INVALID_ID if object is None else int(object))


def atlas_uv(uv, num_triangles):
    """the one rule for a second UV set: float32[num_triangles, 6] = u1 v1 u2 v2 u3 v3 per triangle in BVH order (or [num_triangles, 3, 2]); None: the triangles' own"""
    if uv is None:
        return None
    a = np.ascontiguousarray(uv, np.float32).reshape(-1)
    if a.size != 6 * num_triangles:
        raise RtError("uv must hold six floats per triangle (u1 v1 u2 v2 u3 v3)")
    return a


def _atlas_texels(d):
    # (sized only for a description the library will accept: it refuses the others before it writes)
    ok = 1 <= d.width <= ATLAS_MAX_SIDE and 1 <= d.height <= ATLAS_MAX_SIDE and d.width * d.height <= ATLAS_MAX_TEXELS
    return np.zeros(d.width * d.height if ok else 1, T.texel)


def debug_atlas(ctx, triangles, width, height, gutter=0, object=None, object_of_triangle=None, uv=None):
    """rt_debug_atlas: (types.texel[height * width], types.atlas_stats record) -- the cover of a width x height atlas by caller triangles, primitive_id = the
    index.  ctx None = the host restatement (csrc/atlas.h), else the kernels on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle).reshape(-1)
    ids = np.ascontiguousarray(object_of_triangle, np.uint32) if object_of_triangle is not None else None
    if ids is not None and len(ids) != len(tris):
        raise RtError("object_of_triangle must have one entry per triangle")
    u = atlas_uv(uv, len(tris))
    d = atlas_desc(width, height, gutter, object)
    texels, stats = _atlas_texels(d), np.zeros(1, T.atlas_stats)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_atlas(handle, tris.ctypes.data if len(tris) else None, len(tris), ids.ctypes.data if ids is not None else None,
                            u.ctypes.data if u is not None and u.size else None, C.byref(d), texels.ctypes.data, stats.ctypes.data)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return texels, stats[0]


def atlas_surfaces_host(triangles, texels, object_of_triangle=None):
    """what rt_scene_atlas_surfaces gives for `texels` on `triangles`, on the host: rt_debug_query_surface(NULL) of the hits (bc, primitive_id, t = 0) met by
    all-zero directions -- csrc/query.h's arithmetic; an uncovered record gives a miss record"""
    tx = np.ascontiguousarray(texels, T.texel).reshape(-1)
    hits = np.zeros(len(tx), T.hit)
    hits["bc"]["x"], hits["bc"]["y"], hits["primitive_id"] = tx["bc"][:, 0], tx["bc"][:, 1], tx["primitive_id"]
    return debug_query_surface(None, triangles, np.zeros(len(tx), T.ray), hits, object_of_triangle)


NEAREST_FOUND, NEAREST_BACK_SIDE, NEAREST_FEATURE_SHIFT = 1, 2, 2
NEAREST_FACE, NEAREST_EDGE, NEAREST_VERTEX = 0, 1, 2


def point_records(points):
    """the one rule for a nearest query's points: types.point records as they are, float32[n, 4] = position.xyz, max_distance per row, or float32[n, 3] =
    position.xyz with no limit (max_distance = +inf)"""
    a = np.asarray(points)
    if a.dtype == T.point:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim == 2 and a.shape[1] == 3:
        a = np.ascontiguousarray(np.concatenate([a, np.full((len(a), 1), np.inf, np.float32)], axis=1))
    if a.ndim != 2 or a.shape[1] != 4:
        raise RtError("points must be types.point records, float32[n, 4] (position.xyz, max_distance) or float32[n, 3] (no limit)")
    return a.view(T.point).reshape(-1)


def debug_nearest(ctx, triangles, points):
    """rt_debug_nearest: types.nearest[n], brute force over all `triangles` (types.triangle) for `points` (point_records' rule).  ctx None = the host
    (csrc/nearest.h), else k_nearest_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    pts = point_records(points)
    out = np.zeros(len(pts), T.nearest)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_nearest(handle, tris.ctypes.data if len(tris) else None, len(tris), pts.ctypes.data if len(pts) else None, len(pts),
                              out.ctypes.data if len(pts) else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_nearest_walk(nodes, triangles, points, wide=True, counts=False):
    """rt_debug_nearest_walk (host only): k_nearest's walk over the child-pair form of `nodes` (types.bvh_node; wide=False) or over build_wide_bvh's 4-wide
    records of them (wide=True): types.nearest[n], or (records, uint32[n] triangles tested per point) with counts=True"""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    pts = point_records(points)
    out = np.zeros(len(pts), T.nearest)
    tested = np.zeros(len(pts), np.uint32)
    rc = lib.rt_debug_nearest_walk(nd.ctypes.data if len(nd) else None, len(nd), tris.ctypes.data if len(tris) else None, len(tris), int(wide),
                                   pts.ctypes.data if len(pts) else None, len(pts), out.ctypes.data if len(pts) else None, tested.ctypes.data if len(pts) else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return (out, tested) if counts else out


WITHIN_MAX = 8              # RT_WITHIN_MAX
WITHIN_K_NEAREST = 1        # RT_WITHIN_K_NEAREST: list the max_near nearest members and look no further
POINT_HITS_SEARCHED = 1     # rt_point_hits.flags bit 0
POINT_HITS_K_NEAREST = 2    # rt_point_hits.flags bit 1


def debug_within(ctx, triangles, points, max_near=WITHIN_MAX, k_nearest=False):
    """rt_debug_within: (types.point_hits[n], types.nearest[n, max_near]) of `points` (point_records' rule; max_distance is the radius) by brute force
    over all `triangles` (types.triangle).  ctx None = the host (csrc/within.h), else k_within_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    pts = point_records(points)
    out = np.zeros(len(pts), T.point_hits)
    near = np.zeros((len(pts), max_near), T.nearest)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_within(handle, tris.ctypes.data if len(tris) else None, len(tris), pts.ctypes.data if len(pts) else None, len(pts), max_near,
                             WITHIN_K_NEAREST if k_nearest else 0, out.ctypes.data if len(pts) else None, near.ctypes.data if near.size else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out, near


def debug_within_walk(nodes, triangles, points, max_near=WITHIN_MAX, k_nearest=False, wide=True, counts=False):
    """rt_debug_within_walk (host only): k_within's walk over the child-pair form of `nodes` (types.bvh_node; wide=False) or over build_wide_bvh's 4-wide
    records of them (wide=True): (types.point_hits[n], types.nearest[n, max_near]), with uint32[n] triangles tested per point appended when counts=True"""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    pts = point_records(points)
    out = np.zeros(len(pts), T.point_hits)
    near = np.zeros((len(pts), max_near), T.nearest)
    tested = np.zeros(len(pts), np.uint32)
    rc = lib.rt_debug_within_walk(nd.ctypes.data if len(nd) else None, len(nd), tris.ctypes.data if len(tris) else None, len(tris), int(wide),
                                  pts.ctypes.data if len(pts) else None, len(pts), max_near, WITHIN_K_NEAREST if k_nearest else 0,
                                  out.ctypes.data if len(pts) else None, near.ctypes.data if near.size else None, tested.ctypes.data if len(pts) else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return (out, near, tested) if counts else (out, near)


REGION_MAX_PLANES = 8       # RT_REGION_MAX_PLANES
REGION_LIST_MAX = 8         # RT_REGION_LIST_MAX
REGION_HITS_SEARCHED = 1    # rt_region_hits.flags bit 0
REGION_MEMBER_INSIDE = 1    # rt_region_member.flags bit 0
REGION_MEMBER_CROSSING_SHIFT = 8   # rt_region_member.flags bit 8 + k: plane k has 1 or 2 corners outside
SELECT_MAX_REGIONS = 32     # RT_SELECT_MAX_REGIONS


def region_records(regions):
    """types.region[n], contiguous: an array of them, one scalar, or a list of scalars (types.box_region, types.oriented_box_region, types.planes_region)"""
    if isinstance(regions, np.ndarray) and regions.dtype == T.region:
        return np.ascontiguousarray(regions.reshape(-1))
    return np.ascontiguousarray(np.array(list(regions), T.region).reshape(-1))


def debug_overlap(ctx, triangles, regions, max_list=REGION_LIST_MAX):
    """rt_debug_overlap: (types.region_hits[n], types.region_member[n, max_list]) of `regions` by brute force over all `triangles` (types.triangle).
    ctx None = the host (csrc/region.h), else k_region_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    rg = region_records(regions)
    out = np.zeros(len(rg), T.region_hits)
    members = np.zeros((len(rg), max_list), T.region_member)
    handle = ctx.handle if ctx is not None else None
    rc = lib.rt_debug_overlap(handle, tris.ctypes.data if len(tris) else None, len(tris), rg.ctypes.data if len(rg) else None, len(rg), max_list,
                              out.ctypes.data if len(rg) else None, members.ctypes.data if members.size else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out, members


def debug_overlap_walk(nodes, triangles, regions, max_list=REGION_LIST_MAX, wide=True, counts=False):
    """rt_debug_overlap_walk (host only): k_region's walk over the child-pair form of `nodes` (types.bvh_node; wide=False) or over build_wide_bvh's 4-wide
    records of them (wide=True): (types.region_hits[n], types.region_member[n, max_list]), with uint32[n] triangles tested per region appended when counts=True"""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    rg = region_records(regions)
    out = np.zeros(len(rg), T.region_hits)
    members = np.zeros((len(rg), max_list), T.region_member)
    tested = np.zeros(len(rg), np.uint32)
    rc = lib.rt_debug_overlap_walk(nd.ctypes.data if len(nd) else None, len(nd), tris.ctypes.data if len(tris) else None, len(tris), int(wide),
                                   rg.ctypes.data if len(rg) else None, len(rg), max_list, out.ctypes.data if len(rg) else None,
                                   members.ctypes.data if members.size else None, tested.ctypes.data if len(rg) else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return (out, members, tested) if counts else (out, members)


def debug_select(ctx, triangles, regions, object_of_triangle=None, num_objects=0):
    """rt_debug_select: (touching uint32[nt], inside uint32[nt]) -- bit r: the triangle touches / is inside regions[r], at most 32 regions -- of all
    `triangles`; with object_of_triangle also (object_touching uint32[num_objects], object_inside uint32[num_objects]).  ctx None = the host
    (csrc/region.h), else k_select on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    rg = region_records(regions)
    touching, inside = np.zeros(len(tris), np.uint32), np.zeros(len(tris), np.uint32)
    ids = np.ascontiguousarray(object_of_triangle, np.uint32) if object_of_triangle is not None else None
    ot, oi = np.zeros(num_objects, np.uint32), np.zeros(num_objects, np.uint32)
    handle = ctx.handle if ctx is not None else None
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = lib.rt_debug_select(handle, p(tris), len(tris), p(ids), num_objects, p(rg), len(rg), p(touching), p(inside), p(ot) if ids is not None else None,
                             p(oi) if ids is not None else None)
    if rc != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return (touching, inside, ot, oi) if ids is not None else (touching, inside)


def debug_rect_region(camera, width, height, x0, y0, x1, y1, t_near=0.0, t_far=float("inf")):
    """rt_debug_rect_region (host only): the types.region scalar of the inclusive pixel rectangle (x0, y0) .. (x1, y1) of `camera` (types.camera)"""
    lib = load()
    cam = np.ascontiguousarray(camera, T.camera).reshape(1)
    out = np.zeros(1, T.region)
    if lib.rt_debug_rect_region(cam.ctypes.data, width, height, x0, y0, x1, y1, t_near, t_far, out.ctypes.data) != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return out[0]


CROSS_LIST_MAX = 8          # RT_CROSS_LIST_MAX
CROSS_ANY = 1               # RT_CROSS_ANY: options bit 0, the walk stops at the first member
CROSS_OTHER_OBJECTS = 2     # RT_CROSS_OTHER_OBJECTS: options bit 1 (self forms), pairs of one object are skipped
PROBE_HITS_SEARCHED = 1     # rt_probe_hits.flags bit 0
PROBE_HITS_ANY = 2          # rt_probe_hits.flags bit 1


def probe_records(probes):
    """types.probe[n], contiguous: an array of them, or float[n, 3, 3] corners (types.probes_from_corners)"""
    if isinstance(probes, np.ndarray) and probes.dtype == T.probe:
        return np.ascontiguousarray(probes.reshape(-1))
    return T.probes_from_corners(probes)


def _cross_outputs(n, max_list, options):
    """(out, members or None): an RT_CROSS_ANY answer lists nothing"""
    out = np.zeros(n, T.probe_hits)
    members = np.zeros((n, max_list), T.cross_member) if max_list and not options & CROSS_ANY else None
    return out, members


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def debug_cross(ctx, triangles, probes, max_list=CROSS_LIST_MAX, options=0):
    """rt_debug_cross: (types.probe_hits[n], types.cross_member[n, max_list]) of `probes` by brute force over all `triangles` (types.triangle); the records
    alone when nothing is listed (max_list == 0 or CROSS_ANY).  ctx None = the host (csrc/cross.h), else k_cross_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    pr = probe_records(probes)
    out, members = _cross_outputs(len(pr), max_list, options)
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_cross(handle, _p(tris), len(tris), _p(pr), len(pr), max_list, options, _p(out), _p(members)) != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out if members is None else (out, members)


def debug_cross_walk(nodes, triangles, probes, max_list=CROSS_LIST_MAX, options=0, wide=True, counts=False):
    """rt_debug_cross_walk (host only): k_cross's walk over the child-pair form of `nodes` (types.bvh_node; wide=False) or over build_wide_bvh's 4-wide
    records of them (wide=True): debug_cross's result, with uint32[n] triangles tested per probe appended when counts=True"""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    pr = probe_records(probes)
    out, members = _cross_outputs(len(pr), max_list, options)
    tested = np.zeros(len(pr), np.uint32)
    if lib.rt_debug_cross_walk(_p(nd), len(nd), _p(tris), len(tris), int(wide), _p(pr), len(pr), max_list, options, _p(out), _p(members), _p(tested)) != 0:
        raise RtError(lib.rt_last_error(None).decode())
    got = (out,) if members is None else (out, members)
    if counts:
        got += (tested,)
    return got[0] if len(got) == 1 else got


def debug_cross_self(ctx, triangles, first=0, n=None, max_list=CROSS_LIST_MAX, options=0, object_of_triangle=None):
    """rt_debug_cross_self: debug_cross's result where probe i is triangles[first + i] (n None: to the end); pairs of one index or of a shared corner are
    skipped, and with CROSS_OTHER_OBJECTS pairs of one object (object_of_triangle uint32[nt]).  ctx None = the host, else k_cross_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    n = len(tris) - first if n is None else n
    ids = np.ascontiguousarray(object_of_triangle, np.uint32) if object_of_triangle is not None else None
    out, members = _cross_outputs(n, max_list, options)
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_cross_self(handle, _p(tris), len(tris), _p(ids), first, n, max_list, options, _p(out), _p(members)) != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out if members is None else (out, members)


SEPARATION_OTHER_OBJECTS = 2     # RT_SEPARATION_OTHER_OBJECTS: options bit 1 (self forms), pairs of one object are skipped
SEPARATION_SEARCHED = 1          # rt_separation.flags bit 0
SEPARATION_FOUND = 2             # rt_separation.flags bit 1
SEPARATION_CROSSING = 4          # rt_separation.flags bit 2
SEPARATION_FEATURE_CROSSING = 15


def debug_separation(ctx, triangles, probes, max_distance=float("inf")):
    """rt_debug_separation: types.separation[n] of `probes` (probe_records' rule) by brute force over all `triangles` (types.triangle): the nearest triangle
    within max_distance, the two closest points and their distance.  ctx None = the host (csrc/separation.h), else k_separation_brute on ctx's GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    pr = probe_records(probes)
    out = np.zeros(len(pr), T.separation)
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_separation(handle, _p(tris), len(tris), _p(pr), len(pr), max_distance, _p(out)) != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def debug_separation_walk(nodes, triangles, probes, max_distance=float("inf"), wide=True, counts=False):
    """rt_debug_separation_walk (host only): k_separation's walk over the child-pair form of `nodes` (types.bvh_node; wide=False) or over build_wide_bvh's
    4-wide records of them (wide=True): debug_separation's result, with uint32[n] triangles tested per probe when counts=True"""
    lib = load()
    nd = np.ascontiguousarray(nodes, T.bvh_node)
    tris = np.ascontiguousarray(triangles, T.triangle)
    pr = probe_records(probes)
    out = np.zeros(len(pr), T.separation)
    tested = np.zeros(len(pr), np.uint32)
    if lib.rt_debug_separation_walk(_p(nd), len(nd), _p(tris), len(tris), int(wide), _p(pr), len(pr), max_distance, _p(out), _p(tested)) != 0:
        raise RtError(lib.rt_last_error(None).decode())
    return (out, tested) if counts else out


def debug_separation_self(ctx, triangles, first=0, n=None, max_distance=float("inf"), options=0, object_of_triangle=None):
    """rt_debug_separation_self: debug_separation's result where probe i is triangles[first + i] (n None: to the end); pairs of one index or of a shared
    corner are skipped, and with SEPARATION_OTHER_OBJECTS pairs of one object (object_of_triangle uint32[nt]).  ctx None = the host, else the GPU."""
    lib = load()
    tris = np.ascontiguousarray(triangles, T.triangle)
    n = len(tris) - first if n is None else n
    ids = np.ascontiguousarray(object_of_triangle, np.uint32) if object_of_triangle is not None else None
    out = np.zeros(n, T.separation)
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_separation_self(handle, _p(tris), len(tris), _p(ids), first, n, max_distance, options, _p(out)) != 0:
        raise RtError(lib.rt_last_error(handle).decode())
    return out


def choose_tree(scene, shadow=True, mode=1):
    """rt_debug_choose_tree (host only, no GPU): the 4-wide tree rt_scene_upload would give this scene's shadow / closest-hit
    rays under RT_CTX_OPT_SHADOW_TREE / RT_CTX_OPT_CLOSEST_TREE = mode.  scene: dict with triangles, nodes, lights.
    Returns (records as bytes-compatible uint8[n, 64], entry_ref, report)."""
    lib = load()
    tris, nodes, lights = (np.ascontiguousarray(scene[k]) for k in ("triangles", "nodes", "lights"))
    d = rt_scene_desc()
    d.triangles, d.num_triangles, d.nodes, d.num_nodes = tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes)
    d.lights, d.num_lights = (lights.ctypes.data if len(lights) else None), len(lights)
    n, entry = C.c_uint32(), C.c_uint32()
    rep = C.create_string_buffer(2048)
    if lib.rt_debug_choose_tree(C.byref(d), int(bool(shadow)), mode, None, 0, C.byref(n), C.byref(entry), rep, len(rep)):
        raise RtError(lib.rt_last_error(None).decode())
    out = np.zeros((n.value, 64), np.uint8)
    if lib.rt_debug_choose_tree(C.byref(d), int(bool(shadow)), mode, out.ctypes.data, n.value, C.byref(n), C.byref(entry), rep, len(rep)):
        raise RtError(lib.rt_last_error(None).decode())
    return out, entry.value, rep.value.decode()


ADAPTIVE_FOLD_DEFAULT = 25     # rt_ctx's RT_CTX_OPT_ADAPTIVE_FOLD as created (rt_hip.hip): bits 0 + 3 + 4 since round 5


def export_folds(ctx_handle):
    """rt_scene_export_folds: (closest records uint8[n, 64], shadow records uint8[m, 64] (m = 0: shared), (closest entry, shadow entry))"""
    lib = load()
    n, m = C.c_uint32(), C.c_uint32()
    ent = (C.c_uint32 * 2)()
    if lib.rt_scene_export_folds(ctx_handle, None, None, 0, C.byref(n), C.byref(m), ent):
        raise RtError(lib.rt_last_error(ctx_handle).decode())
    cap = max(n.value, m.value, 1)
    cl, sh = np.zeros((cap, 64), np.uint8), np.zeros((cap, 64), np.uint8)
    if lib.rt_scene_export_folds(ctx_handle, cl.ctypes.data, sh.ctypes.data, cap, C.byref(n), C.byref(m), ent):
        raise RtError(lib.rt_last_error(ctx_handle).decode())
    return cl[:n.value].copy(), sh[:m.value].copy(), (int(ent[0]), int(ent[1]))


def import_folds(ctx_handle, closest, shadow, entries):
    """rt_scene_import_folds: another context's records in place of this one's (same scene); its own adaptation goes off"""
    lib = load()
    cl = np.ascontiguousarray(closest, np.uint8)
    sh = np.ascontiguousarray(shadow, np.uint8) if shadow is not None and len(shadow) else None
    if lib.rt_scene_import_folds(ctx_handle, cl.ctypes.data, len(cl), entries[0], sh.ctypes.data if sh is not None else None, len(sh) if sh is not None else 0, entries[1]):
        raise RtError(lib.rt_last_error(ctx_handle).decode())


def check_folds(nodes, records, entry):
    """rt_debug_check_folds (host only, no context): rt_scene_import_folds' check of `records` (uint8[n, 64] or any 64-byte record array) and their entry against
    the leaves of the LinearBVHNode[] `nodes`.  Returns None, or raises RtError with the importer's words for the defect."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    recs = np.ascontiguousarray(records)
    recs = recs.view(np.uint8).reshape(recs.nbytes // 64, 64)
    if lib.rt_debug_check_folds(nodes.ctypes.data, len(nodes), recs.ctypes.data if len(recs) else None, len(recs), int(entry)):
        raise RtError(lib.rt_last_error(None).decode())


def device_fold(ctx, nodes, iso_weight=-1.0, dirs=None, weights=None):
    """rt_debug_device_fold: the SAH collapse of the LinearBVHNode[] `nodes` on ctx's device (raytracing_amd/csrc/fold_kernels.h).
    iso_weight < 0: the plain surface area; else the metric of rt_debug_wide_bvh_metric; weights: float64[n] per node or None.
    Returns (records uint8[n, 64], entry_ref, roots uint32[n], seconds)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    d = np.ascontiguousarray(dirs, np.float32) if dirs is not None else None
    w = np.ascontiguousarray(weights, np.float64) if weights is not None else None
    cap = len(nodes) // 2 + 2
    out, roots = np.zeros((cap, 64), np.uint8), np.zeros(cap, np.uint32)
    n, entry, sec = C.c_uint32(), C.c_uint32(), C.c_double()
    if lib.rt_debug_device_fold(ctx.handle, nodes.ctypes.data, len(nodes), iso_weight, d.ctypes.data if d is not None else None, len(d) if d is not None else 0,
                                w.ctypes.data if w is not None else None, out.ctypes.data, roots.ctypes.data, cap, C.byref(n), C.byref(entry), C.byref(sec)):
        raise RtError(lib.rt_last_error(ctx.handle).decode())
    return out[:n.value].copy(), entry.value, roots[:n.value].copy(), sec.value


def device_tree(ctx, nodes, iso_weight=1.0, dirs=None, radius=0, frame_dir=None, stretch=1.0):
    """rt_debug_device_tree: a binary tree over the leaves of `nodes` built on ctx's device (PLOC, raytracing_amd/csrc/ploc_kernels.h).  Returns (nodes, seconds, rounds)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3)) if dirs is not None else None
    out = np.zeros(len(nodes), nodes.dtype)
    n, sec, rounds = C.c_uint32(), C.c_double(), C.c_uint32()
    if lib.rt_debug_device_tree(ctx.handle, nodes.ctypes.data, len(nodes), iso_weight, d.ctypes.data if d is not None and len(d) else None, len(d) if d is not None else 0,
                                out.ctypes.data, len(out), C.byref(n), C.byref(sec), C.byref(rounds), radius,
                                np.ascontiguousarray(frame_dir, np.float32).ctypes.data if frame_dir is not None else None, stretch):
        raise RtError(lib.rt_last_error(ctx.handle).decode())
    return out[:n.value].copy(), sec.value, rounds.value


def wide_bvh_weights(nodes, weights):
    """rt_debug_wide_bvh_weights (host only): build_wide_bvh's SAH collapse with per-node weights in place of the area.  Returns (records, entry_ref, roots)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    w = np.ascontiguousarray(weights, np.float64)
    cap = len(nodes) // 2 + 2
    out, roots = np.zeros((cap, 64), np.uint8), np.zeros(cap, np.uint32)
    n, entry = C.c_uint32(), C.c_uint32()
    if lib.rt_debug_wide_bvh_weights(nodes.ctypes.data, len(nodes), w.ctypes.data, out.ctypes.data, roots.ctypes.data, cap, C.byref(n), C.byref(entry)):
        raise RtError(lib.rt_last_error(None).decode())
    return out[:n.value].copy(), entry.value, roots[:n.value].copy()


def count_box_passes(ctx, nodes, origins_tmax, directions):
    """rt_debug_count_box_passes: per node of the LinearBVHNode[] `nodes`, how many of the rays (as adapt_fold takes them) pass its slab test.  ctx None = the host's walk,
    else k_count_box_passes on ctx's GPU.  Returns (counts uint32[len(nodes)], walks cut short by the stack bound)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes, T.bvh_node)
    o = np.ascontiguousarray(origins_tmax, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 4)
    assert len(o) == len(d)
    counts = np.zeros(len(nodes), np.uint32)
    cut = C.c_ulonglong()
    handle = ctx.handle if ctx is not None else None
    if lib.rt_debug_count_box_passes(handle, nodes.ctypes.data, len(nodes), o.ctypes.data, d.ctypes.data, len(o), counts.ctypes.data, C.byref(cut)):
        raise RtError(lib.rt_last_error(handle).decode())
    return counts, cut.value


def adapt_fold(nodes, origins_tmax, directions):
    """rt_debug_adapt_fold (host only, no GPU): RT_CTX_OPT_ADAPTIVE_FOLD's re-fold of the LinearBVHNode[] `nodes` for the rays given
    (origins_tmax float32[n, 4] = x, y, z, t_max; directions float32[n, 4] = x, y, z, -).
    Returns (records uint8[n, 64], entry_ref, roots uint32[n], (cost of the surface-area fold, cost of the adapted fold), adopted)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    o = np.ascontiguousarray(origins_tmax, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 4)
    assert len(o) == len(d)
    n, entry, cheaper = C.c_uint32(), C.c_uint32(), C.c_int()
    cost = (C.c_double * 2)()
    out = np.zeros((len(nodes), 64), np.uint8)                  # a fold never has more records than the tree has nodes
    roots = np.zeros(len(nodes), np.uint32)
    if lib.rt_debug_adapt_fold(nodes.ctypes.data, len(nodes), o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data, roots.ctypes.data, len(out), C.byref(n), C.byref(entry),
                               cost, C.byref(cheaper)):
        raise RtError(lib.rt_last_error(None).decode())
    return out[:n.value].copy(), entry.value, roots[:n.value].copy(), (cost[0], cost[1]), bool(cheaper.value)


def adapt_shadow_side(nodes, origins_tmax, directions, mode, triangles=None):
    """rt_debug_adapt_shadow_side (host only): what FoldAdapt's worker does for the shadow rays under RT_CTX_OPT_ADAPTIVE_FOLD = mode
    (triangles: the scene's rt_triangle array, needed for bit 4).
    Returns (records uint8[n, 64], entry_ref, roots, the tree the records fold, (current cost, candidate cost), rotations, adopted, records reordered)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    o = np.ascontiguousarray(origins_tmax, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 4)
    tris = np.ascontiguousarray(triangles) if triangles is not None else None
    n, entry, made, moved = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    cost = (C.c_double * 2)()
    out = np.zeros((len(nodes), 64), np.uint8)
    roots = np.zeros(len(nodes), np.uint32)
    tree = np.zeros(len(nodes), nodes.dtype)
    rc = lib.rt_debug_adapt_shadow_side(nodes.ctypes.data, len(nodes), o.ctypes.data, d.ctypes.data, len(o), mode, out.ctypes.data, roots.ctypes.data, len(out),
                                        C.byref(n), C.byref(entry), tree.ctypes.data, cost, C.byref(made),
                                        tris.ctypes.data if tris is not None else None, len(tris) if tris is not None else 0, C.byref(moved))
    if rc < 0:
        raise RtError(lib.rt_last_error(None).decode())
    return out[:n.value].copy(), entry.value, roots[:n.value].copy(), tree, (cost[0], cost[1]), made.value, bool(rc), moved.value


def rotate_tree(nodes, origins_tmax, directions, max_passes=8, moves=3, min_gain=0.03):
    """rt_debug_rotate_tree (host only): tree_rotate.h's local search on the binary tree `nodes` for the rays given.
    Returns (rotated nodes, (crossings per ray before, after), rotations made)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes)
    o = np.ascontiguousarray(origins_tmax, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 4)
    out = np.zeros(len(nodes), nodes.dtype)
    cost = (C.c_double * 2)()
    made = C.c_uint32()
    if lib.rt_debug_rotate_tree(nodes.ctypes.data, len(nodes), o.ctypes.data, d.ctypes.data, len(o), max_passes, out.ctypes.data, cost, C.byref(made), moves, min_gain):
        raise RtError(lib.rt_last_error(None).decode())
    return out, (cost[0], cost[1]), made.value


class Context:
    """CLContext replacement (src/gpu_wrappers/cl_context.hpp:37-65)."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib, None, self.lib.rt_ctx_create(device, C.byref(h)))
        self.num_triangles = 0
        self.handle = h
        self._frames = []          # weakrefs: frames (and buffers) must be destroyed before their context

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int()
        mem = C.c_size_t()
        _check(self.lib, self.handle, self.lib.rt_ctx_device_info(self.handle, name, 256, C.byref(cu), C.byref(mem)))
        return name.value.decode(), cu.value, mem.value

    def stream(self):
        return self.lib.rt_ctx_stream(self.handle)

    def upload_blue_noise_tables(self, sobol, scrambling, ranking):
        t = [np.ascontiguousarray(x, np.int32) for x in (sobol, scrambling, ranking)]
        _check(self.lib, self.handle, self.lib.rt_upload_blue_noise_tables(self.handle, *[x.ctypes.data for x in t]))

    def set_treelet_nodes(self, n):
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 0, n))

    def set_wide_bvh(self, mode):
        """RT_CTX_OPT_WIDE_BVH: 1 = SAH-optimal frontier per wide record (default), 2 = two BVH2 levels per record, 0 = none"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 1, mode))

    def set_shadow_tree(self, mode):
        """RT_CTX_OPT_SHADOW_TREE (effective at the next upload_scene): 1 default (own tree where it measures cheaper), 2 own always,
        3 own with the surface-area metric, 0 shared with the closest-hit rays.  Results are bit-identical for every value."""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 2, mode))

    def set_closest_tree(self, mode):
        """RT_CTX_OPT_CLOSEST_TREE: 0 default (bit-identical), 1 / 2 = tolerance mode (own tree where cheaper / always)"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 3, mode))

    def set_adaptive_fold(self, mode):
        """RT_CTX_OPT_ADAPTIVE_FOLD (effective at the next upload_scene): bit 0 = the first integrate() probes the frame's own rays and the
        4-wide trees are folded again for them (exact), bit 1 = integrate() waits for the new fold, bit 2 = small trees too."""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 4, mode))

    def set_adapt_min_interval_ms(self, ms):
        """RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS (default 500): a camera that keeps leaving the adapted view starts at most one fold
        adaptation per this many milliseconds (not applied when bit 1 of the adaptive-fold mode waits for every adaptation)"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 5, ms))

    def set_refittable(self, on=True):
        """RT_CTX_OPT_REFITTABLE (effective at the next upload_scene): keep what refit_scene() needs on the device (about 34 bytes per triangle)"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 10, 1 if on else 0))

    def set_refit_motion(self, on=True):
        """RT_CTX_OPT_REFIT_MOTION (effective at the next upload_scene; needs set_refittable): every refit keeps the pose it replaces (96 bytes per
        triangle) and Frame.filter_temporal() follows the moved surfaces instead of dropping its history"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 11, 1 if on else 0))

    def refit_scene(self, triangles):
        """rt_scene_refit / rt_scene_refit_buffer: the uploaded scene's triangles moved (same count, same order).  `triangles`: a structured array
        (types.triangle), or a Buffer of this context that holds them (no host copy).  Frames keep their sums: reset() them."""
        if isinstance(triangles, Buffer):
            _check(self.lib, self.handle, self.lib.rt_scene_refit_buffer(self.handle, triangles.handle))
            return
        t = np.ascontiguousarray(triangles)
        if t.dtype != T.triangle:
            raise RtError("refit_scene: triangles has the wrong dtype")
        _check(self.lib, self.handle, self.lib.rt_scene_refit(self.handle, t.ctypes.data, len(t)))

    def set_objects(self, object_of_triangle, num_objects):
        """rt_scene_set_objects: which object each triangle of the uploaded scene belongs to (uint32, the upload's order).  The scene's current pose becomes the
        rest pose of pose_scene(); needs set_refittable() before upload_scene().  324 bytes per triangle on the device."""
        ids = np.ascontiguousarray(object_of_triangle, np.uint32)
        if ids.ndim != 1:
            raise RtError("set_objects: one object index per triangle")
        _check(self.lib, self.handle, self.lib.rt_scene_set_objects(self.handle, ids.ctypes.data, len(ids), num_objects))

    def pose_scene(self, matrices):
        """rt_scene_pose: the rest pose posed by one matrix per object (float32[num_objects, 3, 4]; absolute, never relative to the last pose), written on the
        device and refitted as refit_scene() would.  Frames keep their sums: reset() them."""
        m = _matrices3x4(matrices, "pose_scene")
        _check(self.lib, self.handle, self.lib.rt_scene_pose(self.handle, m.ctypes.data, len(m)))

    def set_skin(self, influences, num_bones):
        """rt_scene_set_skin: four bones and weights per triangle CORNER of the uploaded scene (types.skin_influence[3 * triangles] or [triangles, 3], the
        upload's order; types.influences packs them).  The scene's current pose becomes the rest pose of skin_scene(); needs set_refittable() before
        upload_scene().  392 bytes per triangle on the device.  Independent of set_objects()."""
        f = _influences(influences, None, "set_skin")
        _check(self.lib, self.handle, self.lib.rt_scene_set_skin(self.handle, f.ctypes.data, len(f) // 3, num_bones))

    def skin_scene(self, matrices):
        """rt_scene_skin: the rest pose skinned by a palette of one matrix per bone (float32[num_bones, 3, 4]; absolute, never relative to the last skin),
        written on the device and refitted as refit_scene() would.  Frames keep their sums: reset() them."""
        m = _matrices3x4(matrices, "skin_scene")
        _check(self.lib, self.handle, self.lib.rt_scene_skin(self.handle, m.ctypes.data, len(m)))

    def set_morph(self, deltas, offsets, num_triangles):
        """rt_scene_set_morph: sparse morph targets of the uploaded scene (types.morph_delta records and uint32 offsets, one more than targets: types.morph_targets
        packs them; corners are 3 * triangle + c in the upload's order).  The scene's current pose becomes the rest pose of morph_scene() and
        morph_skin_scene(); needs set_refittable() before upload_scene().  Independent of set_objects() and set_skin()."""
        d, o = _morph_table(deltas, offsets, "set_morph")
        _check(self.lib, self.handle, self.lib.rt_scene_set_morph(self.handle, d.ctypes.data, o.ctypes.data, len(o) - 1, num_triangles))

    def morph_scene(self, weights):
        """rt_scene_morph: the rest pose morphed by one weight per target (float32[targets]; absolute, never relative to the last morph), written on the device
        and refitted as refit_scene() would.  Frames keep their sums: reset() them."""
        w = _weights(weights, "morph_scene")
        _check(self.lib, self.handle, self.lib.rt_scene_morph(self.handle, w.ctypes.data, len(w)))

    def morph_skin_scene(self, weights, matrices):
        """rt_scene_morph_skin: the MORPH's rest pose morphed by `weights`, then skinned by set_skin()'s influences and the palette `matrices`
        (float32[num_bones, 3, 4]) in one kernel, and refitted.  Needs set_morph() and set_skin()."""
        w = _weights(weights, "morph_skin_scene")
        m = _matrices3x4(matrices, "morph_skin_scene")
        _check(self.lib, self.handle, self.lib.rt_scene_morph_skin(self.handle, w.ctypes.data, len(w), m.ctypes.data, len(m)))

    def trace(self, rays, any_hit=False, surfaces=False):
        """rt_scene_trace: the caller's rays (ray_records' rule) against the uploaded scene.  Closest hits: types.hit[n], or (hits, types.surface[n]) with
        surfaces=True.  any_hit=True: uint32[n], 1 where anything lies within [t_min, t_max]."""
        r = ray_records(rays)
        n = len(r)
        p = lambda a: a.ctypes.data if a is not None and len(a) else None
        if any_hit:
            if surfaces:
                raise RtError("trace: an any-hit query reports no surfaces")
            occ = np.zeros(n, np.uint32)
            _check(self.lib, self.handle, self.lib.rt_scene_trace(self.handle, p(r), n, QUERY_ANY_HIT, None, occ.ctypes.data, None))
            return occ
        hits = np.zeros(n, T.hit)
        surf = np.zeros(n, T.surface) if surfaces else None
        _check(self.lib, self.handle, self.lib.rt_scene_trace(self.handle, p(r), n, QUERY_CLOSEST, hits.ctypes.data, None, surf.ctypes.data if surfaces else None))
        return (hits, surf) if surfaces else hits

    def trace_buffer(self, rays, n, any_hit=False, hits=None, occluded=None, surfaces=None):
        """rt_scene_trace_buffer: the same over Buffers of this context (n records each; an output that is not wanted is None).  Only enqueues:
        Buffer.read() or finish() waits."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_trace_buffer(self.handle, h(rays), n, QUERY_ANY_HIT if any_hit else QUERY_CLOSEST, h(hits), h(occluded), h(surfaces)))

    def trace_all(self, rays, max_hits=ALL_HITS_MAX, surfaces=False):
        """rt_scene_trace_all: every surface each of the caller's rays (ray_records' rule) crosses: (types.ray_hits[n], types.hit[n, max_hits]) -- the
        counts, and the nearest max_hits crossings in ascending (t, primitive_id) order -- or (records, hits, types.surface[n, max_hits]) with
        surfaces=True.  max_hits=0: the records alone."""
        r = ray_records(rays)
        n = len(r)
        out = np.zeros(n, T.ray_hits)
        if max_hits == 0:
            if surfaces:
                raise RtError("trace_all: surfaces need max_hits > 0")
            _check(self.lib, self.handle, self.lib.rt_scene_trace_all(self.handle, r.ctypes.data if n else None, n, 0, out.ctypes.data, None, None))
            return out
        hits = np.zeros((n, max_hits), T.hit)
        surf = np.zeros((n, max_hits), T.surface) if surfaces else None
        _check(self.lib, self.handle, self.lib.rt_scene_trace_all(self.handle, r.ctypes.data if n else None, n, max_hits, out.ctypes.data, hits.ctypes.data,
                                                                    surf.ctypes.data if surfaces else None))
        return (out, hits, surf) if surfaces else (out, hits)

    def trace_all_buffer(self, rays, n, max_hits, out, hits=None, surfaces=None):
        """rt_scene_trace_all_buffer: the same over Buffers of this context (n rays and records, n * max_hits hits / surfaces; an output that is not
        wanted is None).  Only enqueues: Buffer.read() or finish() waits."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_trace_all_buffer(self.handle, h(rays), n, max_hits, h(out), h(hits), h(surfaces)))

    def nearest(self, points, surfaces=False):
        """rt_scene_nearest: for each of the caller's points (point_records' rule) the nearest triangle of the uploaded scene, where on it and how far:
        types.nearest[n], or (records, types.surface[n]) with surfaces=True"""
        pts = point_records(points)
        n = len(pts)
        out = np.zeros(n, T.nearest)
        surf = np.zeros(n, T.surface) if surfaces else None
        _check(self.lib, self.handle, self.lib.rt_scene_nearest(self.handle, pts.ctypes.data if n else None, n, out.ctypes.data, surf.ctypes.data if surfaces else None))
        return (out, surf) if surfaces else out

    def nearest_buffer(self, points, n, out=None, surfaces=None):
        """rt_scene_nearest_buffer: the same over Buffers of this context (n records each; an output that is not wanted is None).  Only enqueues:
        Buffer.read() or finish() waits."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_nearest_buffer(self.handle, h(points), n, h(out), h(surfaces)))

    def within(self, points, max_near=WITHIN_MAX, k_nearest=False, surfaces=False):
        """rt_scene_within: every triangle of the uploaded scene within max_distance of each of the caller's points (point_records' rule):
        (types.point_hits[n], types.nearest[n, max_near]) -- the counts, and the nearest max_near members in ascending (d2, primitive_id) order -- or
        (records, members, types.surface[n, max_near]) with surfaces=True.  max_near=0: the records alone.  k_nearest: list the max_near nearest and
        look no further (count == stored)."""
        pts = point_records(points)
        n = len(pts)
        out = np.zeros(n, T.point_hits)
        options = WITHIN_K_NEAREST if k_nearest else 0
        if max_near == 0:
            if surfaces:
                raise RtError("within: surfaces need max_near > 0")
            _check(self.lib, self.handle, self.lib.rt_scene_within(self.handle, pts.ctypes.data if n else None, n, 0, options, out.ctypes.data, None, None))
            return out
        near = np.zeros((n, max_near), T.nearest)
        surf = np.zeros((n, max_near), T.surface) if surfaces else None
        _check(self.lib, self.handle, self.lib.rt_scene_within(self.handle, pts.ctypes.data if n else None, n, max_near, options, out.ctypes.data, near.ctypes.data,
                                                                 surf.ctypes.data if surfaces else None))
        return (out, near, surf) if surfaces else (out, near)

    def within_buffer(self, points, n, max_near, out, near=None, surfaces=None, k_nearest=False):
        """rt_scene_within_buffer: the same over Buffers of this context (n points and records, n * max_near members / surfaces; an output that is not
        wanted is None).  Only enqueues: Buffer.read() or finish() waits."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_within_buffer(self.handle, h(points), n, max_near, WITHIN_K_NEAREST if k_nearest else 0, h(out), h(near), h(surfaces)))

    def overlap(self, regions, max_list=REGION_LIST_MAX):
        """rt_scene_overlap: every triangle of the uploaded scene that each of the caller's regions (region_records' rule) touches or encloses:
        (types.region_hits[n], types.region_member[n, max_list]) -- the counts, and the touching triangles with the lowest primitive ids, ascending.
        max_list=0: the records alone."""
        rg = region_records(regions)
        n = len(rg)
        out = np.zeros(n, T.region_hits)
        if max_list == 0:
            _check(self.lib, self.handle, self.lib.rt_scene_overlap(self.handle, rg.ctypes.data if n else None, n, 0, out.ctypes.data, None))
            return out
        members = np.zeros((n, max_list), T.region_member)
        _check(self.lib, self.handle, self.lib.rt_scene_overlap(self.handle, rg.ctypes.data if n else None, n, max_list, out.ctypes.data, members.ctypes.data))
        return out, members

    def overlap_buffer(self, regions, n, max_list, out, members=None):
        """rt_scene_overlap_buffer: the same over Buffers of this context (n regions and records, n * max_list members; None: not wanted).  Only
        enqueues: Buffer.read() or finish() waits."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_overlap_buffer(self.handle, h(regions), n, max_list, h(out), h(members)))

    def cross(self, probes, max_list=CROSS_LIST_MAX, options=0):
        """rt_scene_cross: every triangle of the uploaded scene that each of the caller's triangles (probe_records' rule) crosses:
        (types.probe_hits[n], types.cross_member[n, max_list]) -- the counts, and the crossing triangles with the lowest primitive ids, ascending, with
        their contact points; the records alone when nothing is listed (max_list == 0 or CROSS_ANY).  Bit for bit debug_cross's brute force."""
        pr = probe_records(probes)
        out, members = _cross_outputs(len(pr), max_list, options)
        _check(self.lib, self.handle, self.lib.rt_scene_cross(self.handle, _p(pr), len(pr), max_list, options, _p(out), _p(members)))
        return out if members is None else (out, members)

    def cross_buffer(self, probes, n, max_list, options, out, members=None):
        """rt_scene_cross_buffer: the same over Buffers of this context (n probes and records, n * max_list members; None: not wanted).  Only enqueues."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_cross_buffer(self.handle, h(probes), n, max_list, options, h(out), h(members)))

    def cross_self(self, first, n, max_list=CROSS_LIST_MAX, options=0):
        """rt_scene_cross_self: Context.cross's result where probe i is scene triangle first + i (select's triangle order); pairs of one index or of a shared
        corner are skipped, and with CROSS_OTHER_OBJECTS (needs set_objects) pairs of one object"""
        out, members = _cross_outputs(n, max_list, options)
        _check(self.lib, self.handle, self.lib.rt_scene_cross_self(self.handle, first, n, max_list, options, _p(out), _p(members)))
        return out if members is None else (out, members)

    def cross_self_buffer(self, first, n, max_list, options, out, members=None):
        """rt_scene_cross_self_buffer: the same into Buffers of this context.  Only enqueues."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_cross_self_buffer(self.handle, first, n, max_list, options, h(out), h(members)))

    def separation(self, probes, max_distance=float("inf"), options=0):
        """rt_scene_separation: types.separation[n] -- per caller's triangle (probe_records' rule) the nearest triangle of the uploaded scene within
        max_distance, the two closest points, their distance (0 and SEPARATION_CROSSING where the two cross).  Bit for bit debug_separation's brute force."""
        pr = probe_records(probes)
        out = np.zeros(len(pr), T.separation)
        _check(self.lib, self.handle, self.lib.rt_scene_separation(self.handle, _p(pr), len(pr), max_distance, options, _p(out)))
        return out

    def separation_buffer(self, probes, n, max_distance, options, out):
        """rt_scene_separation_buffer: the same over Buffers of this context (n probes, n records).  Only enqueues."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_separation_buffer(self.handle, h(probes), n, max_distance, options, h(out)))

    def separation_self(self, first, n, max_distance=float("inf"), options=0):
        """rt_scene_separation_self: Context.separation's result where probe i is scene triangle first + i; pairs of one index or of a shared corner are
        skipped, and with SEPARATION_OTHER_OBJECTS (needs set_objects) pairs of one object"""
        out = np.zeros(n, T.separation)
        _check(self.lib, self.handle, self.lib.rt_scene_separation_self(self.handle, first, n, max_distance, options, _p(out)))
        return out

    def separation_self_buffer(self, first, n, max_distance, options, out):
        """rt_scene_separation_self_buffer: the same into a Buffer of this context.  Only enqueues."""
        _check(self.lib, self.handle, self.lib.rt_scene_separation_self_buffer(self.handle, first, n, max_distance, options, out.handle if out is not None else None))

    def select(self, regions, objects=0):
        """rt_scene_select: at most 32 regions against every triangle: (touching uint32[num_triangles], inside uint32[num_triangles]), bit r for
        regions[r]; objects = set_objects' num_objects: also (object_touching uint32[objects], object_inside uint32[objects])"""
        rg = region_records(regions)
        if self.num_triangles == 0:
            raise RtError("select: no scene uploaded through upload_scene() (the per-triangle words are sized by its triangle count)")
        touching, inside = np.zeros(self.num_triangles, np.uint32), np.zeros(self.num_triangles, np.uint32)
        ot, oi = np.zeros(objects, np.uint32), np.zeros(objects, np.uint32)
        _check(self.lib, self.handle, self.lib.rt_scene_select(self.handle, rg.ctypes.data if len(rg) else None, len(rg), touching.ctypes.data, inside.ctypes.data,
                                                                 ot.ctypes.data if objects else None, oi.ctypes.data if objects else None))
        return (touching, inside, ot, oi) if objects else (touching, inside)

    def select_buffer(self, regions, n, touching=None, inside=None, object_touching=None, object_inside=None):
        """rt_scene_select_buffer: the same over Buffers of this context (None: not wanted).  Only enqueues."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_select_buffer(self.handle, h(regions), n, h(touching), h(inside), h(object_touching), h(object_inside)))

    def bake(self, points, samples, seed=0, bias=BAKE_BIAS_DEFAULT, radius=BAKE_RADIUS_DEFAULT, from_surfaces=False):
        """rt_scene_bake: ambient occlusion and bent normals at the caller's points (bake_points' rule): types.bake_result[n] -- unoccluded / samples is the
        ambient occlusion term, 0xFFFFFFFF marks a skipped point"""
        pts = bake_points(points, from_surfaces)
        d = bake_desc(samples, seed, bias, radius, from_surfaces)
        out = np.zeros(len(pts), T.bake_result)
        _check(self.lib, self.handle, self.lib.rt_scene_bake(self.handle, pts.ctypes.data if len(pts) else None, len(pts), C.byref(d), out.ctypes.data if len(pts) else None))
        return out

    def bake_buffer(self, points, n, out, samples, seed=0, bias=BAKE_BIAS_DEFAULT, radius=BAKE_RADIUS_DEFAULT, from_surfaces=False):
        """rt_scene_bake_buffer: the same over Buffers of this context (n point records in, n types.bake_result out).  Only enqueues: Buffer.read() or
        finish() waits."""
        d = bake_desc(samples, seed, bias, radius, from_surfaces)
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_bake_buffer(self.handle, h(points), n, C.byref(d), h(out)))

    def atlas(self, width, height, gutter=0, object=None, uv=None):
        """rt_scene_atlas: (types.texel[height * width], types.atlas_stats record) -- per texel of a width x height atlas the lowest triangle of the uploaded
        scene whose UVs cover its centre, where on it (bc) and how many do (atlas_uv's rule for a second UV set).  Byte for byte debug_atlas's."""
        d = atlas_desc(width, height, gutter, object)
        u = atlas_uv(uv, self.num_triangles)
        texels, stats = _atlas_texels(d), np.zeros(1, T.atlas_stats)
        _check(self.lib, self.handle, self.lib.rt_scene_atlas(self.handle, C.byref(d), u.ctypes.data if u is not None and u.size else None, texels.ctypes.data, stats.ctypes.data))
        return texels, stats[0]

    def atlas_buffer(self, width, height, texels, gutter=0, object=None, uv=None, stats=None):
        """rt_scene_atlas_buffer: the same over Buffers of this context (uv: 24 bytes per triangle or None; texels: width * height records; stats: one
        types.atlas_stats or None).  Only enqueues: Buffer.read() or finish() waits."""
        d = atlas_desc(width, height, gutter, object)
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_atlas_buffer(self.handle, C.byref(d), h(uv), h(texels), h(stats)))

    def atlas_surfaces(self, texels):
        """rt_scene_atlas_surfaces: types.surface[n] of types.texel[n] on the scene's triangles as posed now (a miss record where a texel is uncovered)"""
        tx = np.ascontiguousarray(texels, T.texel).reshape(-1)
        out = np.zeros(len(tx), T.surface)
        _check(self.lib, self.handle, self.lib.rt_scene_atlas_surfaces(self.handle, _p(tx), len(tx), _p(out)))
        return out

    def atlas_surfaces_buffer(self, texels, n, surfaces):
        """rt_scene_atlas_surfaces_buffer: the same over Buffers of this context.  Only enqueues."""
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_atlas_surfaces_buffer(self.handle, h(texels), n, h(surfaces)))

    def bake_atlas(self, width, height, samples, seed=0, bias=BAKE_BIAS_DEFAULT, radius=BAKE_RADIUS_DEFAULT, gutter=0, object=None, uv=None, flags=0):
        """rt_scene_atlas_bake: (types.bake_result[height * width], texels, stats) -- the cover, its surfaces and their occlusion bake in one call on the
        device; an uncovered texel is a skipped point (unoccluded = 0xFFFFFFFF)"""
        d = atlas_desc(width, height, gutter, object)
        bd = bake_desc(samples, seed, bias, radius, flags=flags)
        u = atlas_uv(uv, self.num_triangles)
        texels, stats = _atlas_texels(d), np.zeros(1, T.atlas_stats)
        out = np.zeros(len(texels), T.bake_result)
        _check(self.lib, self.handle, self.lib.rt_scene_atlas_bake(self.handle, C.byref(d), u.ctypes.data if u is not None and u.size else None, C.byref(bd), out.ctypes.data,
                                                                     texels.ctypes.data, stats.ctypes.data))
        return out, texels, stats[0]

    def bake_light(self, points, samples, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT, from_surfaces=False, sky=True, lights=True):
        """rt_scene_light_bake: the irradiance of the sky and of the scene's analytic lights at the caller's points (bake_points' rule), direct terms only,
        shadowed by the scene as posed now: types.light_bake_result[n]; a skipped point is zeros and both counts INVALID_ID"""
        pts = bake_points(points, from_surfaces)
        d = light_bake_desc(samples, seed, bias, sky_distance, from_surfaces, sky, lights)
        out = np.zeros(len(pts), T.light_bake_result)
        _check(self.lib, self.handle, self.lib.rt_scene_light_bake(self.handle, pts.ctypes.data if len(pts) else None, len(pts), C.byref(d), out.ctypes.data if len(pts) else None))
        return out

    def bake_light_buffer(self, points, n, out, samples, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT, from_surfaces=False, sky=True,
                          lights=True):
        """rt_scene_light_bake_buffer: the same over Buffers of this context (n point records in, n types.light_bake_result out).  Only enqueues."""
        d = light_bake_desc(samples, seed, bias, sky_distance, from_surfaces, sky, lights)
        h = lambda b: b.handle if b is not None else None
        _check(self.lib, self.handle, self.lib.rt_scene_light_bake_buffer(self.handle, h(points), n, C.byref(d), h(out)))

    def bake_light_atlas(self, width, height, samples, seed=0, bias=BAKE_BIAS_DEFAULT, sky_distance=LIGHT_BAKE_SKY_DISTANCE_DEFAULT, gutter=0, object=None, uv=None,
                         flags=0):
        """rt_scene_atlas_bake_light: (types.light_bake_result[height * width], texels, stats) -- the cover, its surfaces and their light bake in one call on
        the device; an uncovered texel is a skipped point"""
        d = atlas_desc(width, height, gutter, object)
        bd = light_bake_desc(samples, seed, bias, sky_distance, flags=flags)
        u = atlas_uv(uv, self.num_triangles)
        texels, stats = _atlas_texels(d), np.zeros(1, T.atlas_stats)
        out = np.zeros(len(texels), T.light_bake_result)
        _check(self.lib, self.handle, self.lib.rt_scene_atlas_bake_light(self.handle, C.byref(d), u.ctypes.data if u is not None and u.size else None, C.byref(bd),
                                                                         out.ctypes.data, texels.ctypes.data, stats.ctypes.data))
        return out, texels, stats[0]

    def set_bake_chunk_points(self, points):
        """RT_CTX_OPT_BAKE_CHUNK_POINTS: bake() stages at most this many points at a time (0 = the default, 1 Mi); no result depends on it"""
        _check(self.lib, self.handle, self.lib.rt_ctx_set_option(self.handle, 12, points))

    def create_buffer(self, data):
        """an rt_buffer of this context holding `data` (any contiguous array)"""
        return Buffer(self, data)

    def tree_report(self):
        return self.lib.rt_scene_tree_report(self.handle).decode()

    def finish(self):
        _check(self.lib, self.handle, self.lib.rt_finish(self.handle))

    def upload_scene(self, scene):
        """scene: dict with triangles (BVH order), nodes, materials, textures,
        texture_data, lights, emissive, env (H x W x 4 float32)."""
        s = {k: np.ascontiguousarray(v) for k, v in scene.items() if k not in ("scene_info", "flags")}
        for key, dt in (("triangles", T.triangle), ("nodes", T.bvh_node), ("materials", T.packed_material),
                        ("textures", T.texture), ("lights", T.light)):
            if s[key].dtype != dt:
                raise RtError("scene['%s'] has the wrong dtype" % key)
        env = s["env"].astype(np.float32, copy=False)
        p = lambda a: a.ctypes.data if a.size else None
        d = rt_scene_desc(p(s["triangles"]), len(s["triangles"]), p(s["nodes"]), len(s["nodes"]),
                          p(s["materials"]), len(s["materials"]), p(s["textures"]), len(s["textures"]),
                          p(s["texture_data"]), len(s["texture_data"]), p(s["lights"]), len(s["lights"]),
                          p(s["emissive"]), len(s["emissive"]), p(env), env.shape[1], env.shape[0])
        # opt-in extensions: 6 x uint16 texture indices per material, RT_SCENE_* flags
        tex16 = s.get("material_texture_indices")
        if tex16 is not None:
            tex16 = np.ascontiguousarray(tex16, np.uint16)
            if tex16.size != 6 * len(s["materials"]):
                raise RtError("scene['material_texture_indices'] needs 6 entries per material")
            d.material_texture_indices = tex16.ctypes.data
        d.flags = int(scene.get("flags", 0))
        _check(self.lib, self.handle, self.lib.rt_scene_upload(self.handle, C.byref(d)))
        self.num_triangles = len(s["triangles"])          # what select() and Frame.pick_rect() size their per-triangle words by

    def debug_eval(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        out = np.zeros_like(a)
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, np.float32)
            bp = b.ctypes.data
        _check(self.lib, self.handle, self.lib.rt_debug_eval(self.handle, fn, a.ctypes.data, bp, out.ctypes.data,
                                                             a.size))
        return out

    def close(self):
        if self.handle:
            for ref in self._frames:
                fr = ref()
                if fr is not None:
                    fr.close()
            self._frames = []
            self.lib.rt_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Buffer:
    """rt_buffer: device memory of a context (CLContext's buffers); close() it before its context."""

    def __init__(self, ctx, data):
        self.lib = ctx.lib
        self.ctx = ctx
        a = np.ascontiguousarray(data)
        h = C.c_void_p()
        _check(self.lib, ctx.handle, self.lib.rt_buffer_create(ctx.handle, a.nbytes, a.ctypes.data, C.byref(h)))
        self.handle = h
        self.nbytes = a.nbytes
        import weakref
        ctx._frames.append(weakref.ref(self))

    def write(self, data, offset=0):
        a = np.ascontiguousarray(data)
        _check(self.lib, self.ctx.handle, self.lib.rt_buffer_write(self.handle, offset, a.ctypes.data, a.nbytes))

    def read(self, dtype, count, offset=0):
        """rt_buffer_read (blocking): `count` records of `dtype` from byte `offset`"""
        out = np.zeros(count, dtype)
        if count:
            _check(self.lib, self.ctx.handle, self.lib.rt_buffer_read(self.handle, offset, out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if self.handle:
            self.lib.rt_buffer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame:
    """Device half of CLPathTraceIntegrator for one tile of the image."""

    def __init__(self, ctx, width, height, tile_rank=0, tile_count=1, band_height=8):
        self.ctx, self.lib = ctx, ctx.lib
        self.width, self.height = width, height
        d = rt_frame_desc(width, height, tile_rank, tile_count, band_height)
        h = C.c_void_p()
        _check(self.lib, ctx.handle, self.lib.rt_frame_create(ctx.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self.local_rows = self.lib.rt_frame_local_rows(h)
        import weakref
        ctx._frames.append(weakref.ref(self))

    def _c(self, rc):
        _check(self.lib, self.ctx.handle, rc)

    def global_rows(self):
        return np.array([self.lib.rt_frame_global_row(self.handle, r) for r in range(self.local_rows)], np.int64)

    def set_camera(self, cam):
        cam = np.ascontiguousarray(cam)
        self._c(self.lib.rt_set_camera(self.handle, cam.ctypes.data))

    def set_option(self, opt, value):
        self._c(self.lib.rt_set_option(self.handle, opt, value))

    def set_max_bounces(self, b):
        self.set_option(OPT_MAX_BOUNCES, b)

    def reset(self):
        self._c(self.lib.rt_reset(self.handle))

    def integrate(self, n=1):
        self._c(self.lib.rt_integrate(self.handle, n))

    def reserve_samples(self, n):
        got = C.c_uint32(0)
        self._c(self.lib.rt_frame_reserve_samples(self.handle, n, C.byref(got)))
        return got.value

    # stage API
    def generate_rays(self): self._c(self.lib.rt_generate_rays(self.handle))
    def intersect(self, b): self._c(self.lib.rt_intersect(self.handle, b))
    def shade(self, b): self._c(self.lib.rt_shade(self.handle, b))
    def intersect_shadow(self, b): self._c(self.lib.rt_intersect_shadow(self.handle, b))
    def advance_sample(self): self._c(self.lib.rt_advance_sample(self.handle))

    def radiance(self):
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.rt_frame_read_radiance(self.handle, out.ctypes.data))
        return out

    def resolve(self):
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.rt_frame_resolve(self.handle, out.ctypes.data))
        return out

    def filter(self, desc=None):
        """rt_frame_filter: the resolved image passed through the spatial filter (float32[rows, width, 4]); desc None = the header's defaults"""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.rt_frame_filter(self.handle, C.byref(filter_desc(desc)), out.ctypes.data))
        return out

    def guides(self):
        """rt_frame_read_guides: (albedo float32[h, w, 4], normal float32[h, w, 4], depth float32[h, w], guide passes run so far)"""
        alb = np.zeros((self.local_rows, self.width, 4), np.float32)
        nrm = np.zeros_like(alb)
        dep = np.zeros((self.local_rows, self.width), np.float32)
        passes = C.c_uint32()
        self._c(self.lib.rt_frame_read_guides(self.handle, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data, C.byref(passes)))
        return alb, nrm, dep, passes.value

    def pick(self, x, y):
        """rt_frame_pick: (ray, hit, surface) -- types.ray, types.hit, types.surface scalars -- of the ray through the centre of pixel (x, y) of the
        frame's current camera (the guide pass's ray)"""
        ray, hit, surf = np.zeros(1, T.ray), np.zeros(1, T.hit), np.zeros(1, T.surface)
        self._c(self.lib.rt_frame_pick(self.handle, x, y, ray.ctypes.data, hit.ctypes.data, surf.ctypes.data))
        return ray[0], hit[0], surf[0]

    def pick_all(self, x, y, max_hits=ALL_HITS_MAX):
        """rt_frame_pick_all: (ray, record, hits, surfaces) -- a types.ray and a types.ray_hits scalar, types.hit[max_hits], types.surface[max_hits] -- of
        every surface the ray through the centre of pixel (x, y) crosses, nearest first"""
        ray, rec = np.zeros(1, T.ray), np.zeros(1, T.ray_hits)
        hits, surf = np.zeros(max_hits, T.hit), np.zeros(max_hits, T.surface)
        self._c(self.lib.rt_frame_pick_all(self.handle, x, y, max_hits, ray.ctypes.data, rec.ctypes.data, hits.ctypes.data if max_hits else None,
                                           surf.ctypes.data if max_hits else None))
        return ray[0], rec[0], hits, surf

    def pick_rect(self, x0, y0, x1, y1, t_near=0.0, t_far=float("inf"), num_triangles=None, objects=0):
        """rt_frame_pick_rect: (region, touching uint32[num_triangles], inside uint32[num_triangles]) of the inclusive pixel rectangle of the frame's
        current camera -- bit 0 of each word --, with (object_touching, object_inside) appended when objects = set_objects' num_objects"""
        nt = self.ctx.num_triangles if num_triangles is None else num_triangles
        if nt == 0:
            raise RtError("pick_rect: no scene uploaded through upload_scene() (pass num_triangles: the per-triangle words are sized by it)")
        g = np.zeros(1, T.region)
        touching, inside = np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
        ot, oi = np.zeros(objects, np.uint32), np.zeros(objects, np.uint32)
        self._c(self.lib.rt_frame_pick_rect(self.handle, x0, y0, x1, y1, t_near, t_far, g.ctypes.data, touching.ctypes.data, inside.ctypes.data,
                                            ot.ctypes.data if objects else None, oi.ctypes.data if objects else None))
        return (g[0], touching, inside, ot, oi) if objects else (g[0], touching, inside)

    def guide_motion(self):
        """rt_frame_read_guide_motion: (previous position float32[h, w, 4] = (X', 1), previous normal float32[h, w, 4] = (n', 0)) of every pixel's first
        hit in the pose the context's last refit replaced; zeros without a hit or while the context keeps no pose"""
        pos = np.zeros((self.local_rows, self.width, 4), np.float32)
        nrm = np.zeros_like(pos)
        self._c(self.lib.rt_frame_read_guide_motion(self.handle, pos.ctypes.data, nrm.ctypes.data))
        return pos, nrm

    def filter_temporal(self, desc=None):
        """rt_frame_filter_temporal: the resolved image reprojected, accumulated with the frame's history and passed through the variance-guided
        filter (float32[rows, width, 4], tone-mapped); the history advances.  desc None = the header's defaults"""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.rt_frame_filter_temporal(self.handle, C.byref(temporal_filter_desc(desc)), out.ctypes.data))
        return out

    def filter_history(self):
        """rt_frame_read_filter_history: (colour float32[h, w, 4], moments float32[h, w, 4] = (mu1, mu2, L, 0))"""
        col = np.zeros((self.local_rows, self.width, 4), np.float32)
        mom = np.zeros_like(col)
        self._c(self.lib.rt_frame_read_filter_history(self.handle, col.ctypes.data, mom.ctypes.data))
        return col, mom

    def filter_history_reset(self):
        """rt_frame_filter_history_reset: every pixel misses at the next filter_temporal"""
        self._c(self.lib.rt_frame_filter_history_reset(self.handle))

    def present(self, out=None):
        """rt_frame_present: resolve + Finish() on the frame's kernels; the image travels to `out` (kept alive by the caller) on a
        copy stream and is complete after present_wait().  Returns `out`."""
        if out is None:
            out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.rt_frame_present(self.handle, out.ctypes.data))
        return out

    def present_wait(self):
        self._c(self.lib.rt_frame_present_wait(self.handle))

    def radiance_device_ptr(self):
        return self.lib.rt_frame_radiance_device_ptr(self.handle)

    def sample_count(self):
        return self.lib.rt_frame_sample_count(self.handle)

    def stats(self):
        st = rt_stats()
        self._c(self.lib.rt_frame_get_stats(self.handle, C.byref(st)))
        return st

    def profile(self):
        p = rt_profile()
        self._c(self.lib.rt_frame_get_profile(self.handle, C.byref(p)))
        return p

    def copy_radiance_to(self, device_ptr):
        self._c(self.lib.rt_frame_copy_radiance(self.handle, device_ptr))

    def read_queue(self, which, bounce):
        cnt = C.c_uint32()
        # two-call pattern: size query first (the queue holds up to samples-in-flight x tile pixels entries)
        self._c(self.lib.rt_frame_debug_read_queue(self.handle, which, bounce, None, None, None, 0, C.byref(cnt)))
        n = cnt.value
        rays = np.zeros(max(n, 1), T.ray)
        pix = np.zeros(max(n, 1), np.uint32)
        payload = np.zeros(max(n, 1), T.float4)
        self._c(self.lib.rt_frame_debug_read_queue(self.handle, which, bounce, rays.ctypes.data, pix.ctypes.data,
                                                   payload.ctypes.data, n, C.byref(cnt)))
        assert cnt.value == n
        return rays[:n], pix[:n], payload[:n]

    def read_hits(self, count):
        hits = np.zeros(count, T.hit)
        self._c(self.lib.rt_frame_debug_read_hits(self.handle, hits.ctypes.data, count))
        return hits

    def close(self):
        if self.handle:
            self.lib.rt_frame_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """rt_group: ranks of one tiled image and their single RCCL gather (include/rt_hip.h, "device groups").

      Group.create([0, 1, ...])            all ranks in this process (one per device)
      Group.join(nranks, rank, id, device) one process per GPU; id = Group.unique_id() made by rank 0 and
                                           carried to the others by the launcher's own channel"""

    ID_BYTES = 128

    def __init__(self, handle):
        self.lib = load()
        self.handle = handle

    @classmethod
    def create(cls, devices, unchecked=False):
        """unchecked: rt_group_create_unchecked -- the device list goes to ncclCommInitAll as it is (wiring test)"""
        lib = load()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        if (lib.rt_group_create_unchecked if unchecked else lib.rt_group_create)(len(devices), arr, C.byref(h)) != 0:
            raise RtError(lib.rt_group_last_error(None).decode())
        return cls(h)

    @classmethod
    def create_local(cls, n, device=0):
        """n ranks on ONE device, device copies instead of RCCL: the test / plumbing transport."""
        lib = load()
        h = C.c_void_p()
        if lib.rt_group_create_local(n, device, C.byref(h)) != 0:
            raise RtError(lib.rt_group_last_error(None).decode())
        return cls(h)

    @staticmethod
    def unique_id():
        lib = load()
        buf = C.create_string_buffer(Group.ID_BYTES)
        if lib.rt_group_unique_id(buf, Group.ID_BYTES) != 0:
            raise RtError(lib.rt_group_last_error(None).decode())
        return buf.raw

    @classmethod
    def join(cls, nranks, rank, id_bytes, device):
        lib = load()
        assert len(id_bytes) == Group.ID_BYTES
        h = C.c_void_p()
        if lib.rt_group_join(nranks, rank, id_bytes, device, C.byref(h)) != 0:
            raise RtError(lib.rt_group_last_error(None).decode())
        return cls(h)

    def size(self):
        return self.lib.rt_group_size(self.handle)

    def local_ranks(self):
        return [self.lib.rt_group_local_rank(self.handle, i) for i in range(self.lib.rt_group_local_count(self.handle))]

    def comm_count(self, i=0):
        """(ncclCommCount, ncclCommUserRank) of local member i's communicator -- RCCL's own word on how many ranks the
        gather spans; (0, -1) for a local group (device copies, no RCCL)."""
        n, r = C.c_int(0), C.c_int(-1)
        if self.lib.rt_group_comm_count(self.handle, i, C.byref(n), C.byref(r)) != 0:
            raise RtError(self.lib.rt_group_last_error(self.handle).decode())
        return n.value, r.value

    def gather_radiance(self, frame_handles, root, height, width, want_host=True):
        """frame_handles: rt_frame* of the local members, in member order.  Returns the image (numpy,
        height x width x 4) on the process that owns `root` when want_host, else None."""
        n = len(frame_handles)
        arr = (C.c_void_p * n)(*[h if isinstance(h, int) else h.value for h in frame_handles])
        owns_root = root in self.local_ranks()
        out = np.zeros((height, width, 4), np.float32) if (owns_root and want_host) else None
        dev = C.c_void_p()
        rc = self.lib.rt_group_gather_radiance(self.handle, arr, root, out.ctypes.data if out is not None else None, C.byref(dev))
        if rc != 0:
            raise RtError(self.lib.rt_group_last_error(self.handle).decode())
        self.device_image = dev.value
        return out

    def denoise(self, frame_handles, root, height, width):
        """Gather-then-denoise on the root (rt_group_denoise).  Returns (resolved, radiance) on the root's process."""
        n = len(frame_handles)
        arr = (C.c_void_p * n)(*[h if isinstance(h, int) else h.value for h in frame_handles])
        owns_root = root in self.local_ranks()
        res = np.zeros((height, width, 4), np.float32) if owns_root else None
        rad = np.zeros((height, width, 4), np.float32) if owns_root else None
        rc = self.lib.rt_group_denoise(self.handle, arr, root, res.ctypes.data if owns_root else None, rad.ctypes.data if owns_root else None)
        if rc != 0:
            raise RtError(self.lib.rt_group_last_error(self.handle).decode())
        return res, rad

    def close(self):
        if self.handle:
            self.lib.rt_group_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
