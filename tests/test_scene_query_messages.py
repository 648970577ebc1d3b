"""The exact text of what the scene queries' entry points (scene_queries.cpp) and the three picks refuse without a context: every scene form and pick
with its handle NULL, every debug form's NULL-argument, bound, option and `wide` refusals.  No device is needed: each call is refused before anything
is read or launched, so the non-NULL arguments are one scratch array."""
import numpy as np
from raytracing_amd import capi

WIDE = "wide must be 0 (the child-pair form) or 1 (the 4-wide records)"


def test_every_refusal_without_a_context_keeps_its_text():
    lib = capi.load()
    scratch = np.zeros(64, np.uint8)
    B = scratch.ctypes.data                     # stands for any array that is passed but never read
    over_hits, over_near, over_list = capi.ALL_HITS_MAX + 1, capi.WITHIN_MAX + 1, capi.REGION_LIST_MAX + 1
    other_bits = 0xFFFFFFFF & ~capi.WITHIN_K_NEAREST
    cam = np.zeros(256, np.uint8).ctypes.data   # rt_debug_rect_region refuses the rectangle before it reads the camera
    table = [
        # the scene forms, ctx NULL
        ("rt_scene_trace", (None, B, 1, capi.QUERY_CLOSEST, B, None, None), "ctx is NULL"),
        ("rt_scene_trace_buffer", (None, B, 1, capi.QUERY_CLOSEST, B, None, None), "ctx is NULL"),
        ("rt_scene_bake", (None, B, 1, None, B), "ctx is NULL"),
        ("rt_scene_bake_buffer", (None, B, 1, None, B), "ctx is NULL"),
        ("rt_scene_nearest", (None, B, 1, B, None), "ctx is NULL"),
        ("rt_scene_nearest_buffer", (None, B, 1, B, None), "ctx is NULL"),
        ("rt_scene_trace_all", (None, B, 1, 1, B, B, None), "ctx is NULL"),
        ("rt_scene_trace_all_buffer", (None, B, 1, 1, B, B, None), "ctx is NULL"),
        ("rt_scene_within", (None, B, 1, 1, 0, B, B, None), "ctx is NULL"),
        ("rt_scene_within_buffer", (None, B, 1, 1, 0, B, B, None), "ctx is NULL"),
        ("rt_scene_overlap", (None, B, 1, 1, B, B), "ctx is NULL"),
        ("rt_scene_overlap_buffer", (None, B, 1, 1, B, B), "ctx is NULL"),
        ("rt_scene_select", (None, B, 1, B, B, None, None), "ctx is NULL"),
        ("rt_scene_select_buffer", (None, B, 1, B, B, None, None), "ctx is NULL"),
        # n == 0 is no licence to pass no context
        ("rt_scene_trace", (None, None, 0, capi.QUERY_CLOSEST, None, None, None), "ctx is NULL"),
        ("rt_scene_within", (None, None, 0, 0, 0, None, None, None), "ctx is NULL"),
        # the picks, frame NULL
        ("rt_frame_pick", (None, 0, 0, B, B, B), "frame is NULL"),
        ("rt_frame_pick_all", (None, 0, 0, 1, B, B, B, B), "frame is NULL"),
        ("rt_frame_pick_rect", (None, 0, 0, 1, 1, 0.0, 1.0, B, B, B, None, None), "frame is NULL"),
        # the debug forms, ctx NULL: the surface record, the bake's rays and reduction
        ("rt_debug_query_surface", (None, B, 1, None, None, B, 1, B), "NULL argument"),
        ("rt_debug_query_surface", (None, B, 1, None, B, None, 1, B), "NULL argument"),
        ("rt_debug_query_surface", (None, None, 1, None, B, B, 1, B), "NULL argument"),
        ("rt_debug_bake_rays", (None, None, 1, 0, None, B), "NULL argument"),
        ("rt_debug_bake_rays", (None, B, 1, 0, None, B), "NULL argument"),
        ("rt_debug_bake_reduce", (None, B, 1, 16, B), "NULL argument"),
        ("rt_debug_bake_reduce", (B, B, 1, 16, None), "NULL argument"),
        ("rt_debug_bake_reduce", (B, B, 1, 17, B), "samples must be a power of two in 16 .. 4096"),
        ("rt_debug_bake_reduce", (B, B, 1, 8, B), "samples must be a power of two in 16 .. 4096"),
        # ... the nearest point
        ("rt_debug_nearest", (None, B, 1, None, 1, B), "NULL argument"),
        ("rt_debug_nearest", (None, None, 1, B, 1, B), "NULL argument"),
        ("rt_debug_nearest_walk", (B, 1, B, 1, 1, None, 1, B, None), "NULL argument"),
        ("rt_debug_nearest_walk", (B, 0, B, 1, 1, B, 1, B, None), "NULL argument"),
        ("rt_debug_nearest_walk", (B, 1, B, 1, 2, B, 1, B, None), WIDE),
        # ... every hit of a ray
        ("rt_debug_trace_all", (None, B, 1, B, 1, None, 1, 1, B, B), "NULL argument"),
        ("rt_debug_trace_all", (None, B, 1, B, 1, B, 1, 1, B, None), "NULL argument"),
        ("rt_debug_trace_all", (None, B, 1, B, 1, B, 1, over_hits, B, B), "max_hits is above RT_ALL_HITS_MAX"),
        # ... the triangles within a radius: the shape of max_near and options comes before the arguments
        ("rt_debug_within", (None, B, 1, B, 1, over_near, 0, B, B), "max_near is above RT_WITHIN_MAX"),
        ("rt_debug_within", (None, None, 1, None, 1, 1, other_bits, None, None), "unknown option bits"),
        ("rt_debug_within", (None, B, 1, B, 1, 0, capi.WITHIN_K_NEAREST, B, None), "RT_WITHIN_K_NEAREST needs max_near >= 1"),
        ("rt_debug_within", (None, B, 1, B, 1, 1, 0, B, None), "NULL argument"),
        ("rt_debug_within", (None, B, 1, None, 1, 1, 0, B, B), "NULL argument"),
        ("rt_debug_within_walk", (B, 1, B, 1, 1, B, 1, over_near, 0, B, B, None), "max_near is above RT_WITHIN_MAX"),
        ("rt_debug_within_walk", (B, 1, B, 1, 1, B, 1, 1, other_bits, B, B, None), "unknown option bits"),
        ("rt_debug_within_walk", (None, 1, B, 1, 1, B, 1, 1, 0, B, B, None), "NULL argument"),
        ("rt_debug_within_walk", (B, 1, B, 1, 2, B, 1, 1, 0, B, None, None), "NULL argument"),
        ("rt_debug_within_walk", (B, 1, B, 1, 2, B, 1, 1, 0, B, B, None), WIDE),
        # ... the triangles of a region, the select, the rectangle's region
        ("rt_debug_overlap", (None, B, 1, None, 1, over_list, B, B), "max_list is above RT_REGION_LIST_MAX"),
        ("rt_debug_overlap", (None, B, 1, None, 1, 1, B, B), "NULL argument"),
        ("rt_debug_overlap", (None, B, 1, B, 1, 1, B, None), "NULL argument"),
        ("rt_debug_overlap_walk", (None, 1, B, 1, 1, B, 1, over_list, B, B, None), "max_list is above RT_REGION_LIST_MAX"),
        ("rt_debug_overlap_walk", (None, 1, B, 1, 1, B, 1, 1, B, B, None), "NULL argument"),
        ("rt_debug_overlap_walk", (B, 1, B, 1, -1, B, 1, 1, B, B, None), WIDE),
        ("rt_debug_select", (None, B, 1, None, 0, B, 0, B, B, None, None), "n must be 1 .. RT_SELECT_MAX_REGIONS (a bit per region in a 32-bit word)"),
        ("rt_debug_select", (None, B, 1, None, 0, B, capi.SELECT_MAX_REGIONS + 1, B, B, None, None),
         "n must be 1 .. RT_SELECT_MAX_REGIONS (a bit per region in a 32-bit word)"),
        ("rt_debug_select", (None, B, 1, None, 0, None, 1, B, B, None, None), "NULL argument"),
        ("rt_debug_select", (None, B, 1, None, 0, B, 1, B, None, None, None), "NULL argument"),
        ("rt_debug_rect_region", (None, 32, 32, 0, 0, 1, 1, 0.0, 1.0, B), "NULL argument"),
        ("rt_debug_rect_region", (cam, 32, 32, 0, 0, 1, 1, 0.0, 1.0, None), "NULL argument"),
        ("rt_debug_rect_region", (cam, 32, 32, 2, 0, 1, 1, 0.0, 1.0, B), "an empty rectangle (x1 < x0 or y1 < y0)"),
        ("rt_debug_rect_region", (cam, 32, 32, 0, 2, 1, 1, 0.0, 1.0, B), "an empty rectangle (x1 < x0 or y1 < y0)"),
        ("rt_debug_rect_region", (cam, 32, 32, 0, 0, 32, 1, 0.0, 1.0, B), "the rectangle is outside the image"),
        ("rt_debug_rect_region", (cam, 32, 32, 0, 0, 1, 32, 0.0, 1.0, B), "the rectangle is outside the image"),
    ]
    assert {name for name, _, _ in table} == {n for n in capi.EXPORTS if n.startswith(("rt_scene_trace", "rt_scene_bake", "rt_scene_nearest", "rt_scene_within",
        "rt_scene_overlap", "rt_scene_select", "rt_frame_pick", "rt_debug_query_surface", "rt_debug_bake", "rt_debug_nearest", "rt_debug_trace_all", "rt_debug_within",
        "rt_debug_overlap", "rt_debug_select", "rt_debug_rect_region"))}
    for name, args, text in table:
        rc = getattr(lib, name)(*args)
        said = lib.rt_last_error(None).decode()
        assert rc != 0 and said == name + ": " + text, (name, args, rc, said)
    assert not scratch.any()                    # nothing was written through a refused call's arguments
