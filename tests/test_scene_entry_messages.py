"""The exact text of what the scene's own entry points (scene_upload.cpp: upload, refit, the folds' export and import, the tree report and the
rt_debug_* forms of the tree work; scene_moved.cpp: pose) refuse without a context: every scene entry with its handle NULL, every debug form's NULL-argument refusals and the
mismatched arrays the host forms of rt_debug_refit, rt_debug_pose and rt_debug_count_box_passes turn down.  No device is needed: each call is refused
before anything is launched, and what a refusal reads first is a few zeroed records."""
import ctypes as C
import numpy as np
from raytracing_amd import capi, types as T

NULL_ARG = "NULL argument"


def test_every_refusal_without_a_context_keeps_its_text():
    lib = capi.load()
    scratch = np.zeros(64, np.uint8)
    B = scratch.ctypes.data                     # stands for any array that is passed but never read
    U = C.cast(B, C.POINTER(C.c_uint32))        # ... where the prototype wants a typed pointer
    D = C.cast(B, C.POINTER(C.c_double))
    I = C.cast(B, C.POINTER(C.c_int32))
    desc = capi.rt_scene_desc()                 # all NULL, all zero
    sd = C.byref(desc)
    # what the host forms read before they refuse: one interior node without children, one leaf of one triangle, two triangles, object ids, matrices
    interior = np.zeros(1, T.bvh_node)
    leaf = np.zeros(1, T.bvh_node)
    leaf["num_primitives_axis"] = 1 << 16
    tris = np.zeros(2, T.triangle)
    ids = np.array([0, 3], np.uint32)
    eye = np.zeros((1, 3, 4), np.float32)
    nan = np.full((1, 3, 4), np.nan, np.float32)
    N, L, TR, ID, M, MN = (a.ctypes.data for a in (interior, leaf, tris, ids, eye, nan))
    table = [
        # the scene's entries, ctx NULL
        ("rt_scene_upload", (None, sd), NULL_ARG),
        ("rt_scene_upload", (None, None), NULL_ARG),
        ("rt_scene_refit", (None, B, 1), NULL_ARG),
        ("rt_scene_refit", (None, None, 0), NULL_ARG),
        ("rt_scene_refit_buffer", (None, B), NULL_ARG),
        ("rt_scene_refit_buffer", (None, None), NULL_ARG),
        ("rt_scene_set_objects", (None, B, 1, 1), NULL_ARG),
        ("rt_scene_set_objects", (None, None, 0, 0), NULL_ARG),
        ("rt_scene_pose", (None, B, 1), NULL_ARG),
        ("rt_scene_pose", (None, None, 0), NULL_ARG),
        ("rt_scene_export_folds", (None, B, B, 1, U, U, U), NULL_ARG),
        ("rt_scene_export_folds", (None, None, None, 0, None, None, None), NULL_ARG),
        ("rt_scene_import_folds", (None, B, 1, 0, B, 1, 0), NULL_ARG),
        ("rt_scene_import_folds", (None, None, 0, 0, None, 0, 0), NULL_ARG),
        # the folds on the host
        ("rt_debug_wide_bvh", (None, 1, 1, None, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh", (B, 0, 1, None, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh", (B, 1, 1, None, None, 0, None, U), NULL_ARG),
        ("rt_debug_wide_bvh", (B, 1, 2, None, None, 0, U, None), NULL_ARG),
        ("rt_debug_wide_bvh_weights", (None, 1, B, None, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh_weights", (B, 0, B, None, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh_weights", (B, 1, None, None, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh_weights", (B, 1, B, None, None, 0, None, U), NULL_ARG),
        ("rt_debug_wide_bvh_weights", (B, 1, B, None, None, 0, U, None), NULL_ARG),
        ("rt_debug_wide_bvh_metric", (None, 1, 1.0, None, 0, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh_metric", (B, 0, 1.0, None, 0, None, 0, U, U), NULL_ARG),
        ("rt_debug_wide_bvh_metric", (B, 1, 1.0, None, 0, None, 0, None, U), NULL_ARG),
        ("rt_debug_wide_bvh_metric", (B, 1, 1.0, None, 0, None, 0, U, None), NULL_ARG),
        ("rt_debug_pair_layout", (None, 1, B, B, 1), NULL_ARG),
        ("rt_debug_pair_layout", (B, 1, None, B, 1), NULL_ARG),
        ("rt_debug_pair_layout", (B, 1, B, None, 1), NULL_ARG),
        ("rt_debug_pair_layout", (B, 0, B, B, 1), NULL_ARG),
        ("rt_debug_check_folds", (None, 1, B, 1, 0), NULL_ARG),
        ("rt_debug_check_folds", (L, 0, B, 1, 0), NULL_ARG),
        ("rt_debug_check_folds", (L, 1, None, 1, 0), NULL_ARG),
        ("rt_debug_check_folds", (L, 1, B, 1 << 26, 0), "too many records"),
        ("rt_debug_check_folds", (L, 1, None, 0, 0), "the records do not fit this scene (the entry is not a record of the array, or without records not a leaf)"),
        ("rt_debug_check_folds", (L, 1, B, 1, 0), "the records do not fit this scene (a record is reached twice)"),
        # the own trees and the choice between them
        ("rt_debug_own_bvh", (None, 1, 1.0, None, 0, None, 0, U), NULL_ARG),
        ("rt_debug_own_bvh", (B, 0, 1.0, None, 0, None, 0, U), NULL_ARG),
        ("rt_debug_own_bvh", (B, 1, 1.0, None, 0, None, 0, None), NULL_ARG),
        ("rt_debug_choose_tree", (None, 1, 1, None, 0, U, U, None, 0), NULL_ARG),
        ("rt_debug_choose_tree", (sd, 1, 1, None, 0, U, U, None, 0), NULL_ARG),
        # the fold and the tree builder on the device: no context, no device
        ("rt_debug_device_fold", (None, B, 1, -1.0, None, 0, None, None, None, 0, U, U, D), NULL_ARG),
        ("rt_debug_device_tree", (None, B, 1, 1.0, None, 0, None, 0, U, D, U, 0, None, 1.0), NULL_ARG),
        # the adaptation's halves
        ("rt_debug_count_box_passes", (None, None, 1, B, B, 1, B, None), NULL_ARG),
        ("rt_debug_count_box_passes", (None, B, 0, B, B, 1, B, None), NULL_ARG),
        ("rt_debug_count_box_passes", (None, B, 1, B, B, 1, None, None), NULL_ARG),
        ("rt_debug_count_box_passes", (None, B, 1, None, B, 1, B, None), NULL_ARG),
        ("rt_debug_count_box_passes", (None, B, 1, B, None, 1, B, None), NULL_ARG),
        ("rt_debug_count_box_passes", (None, N, 1, None, None, 0, B, None), "the node array is not a tree in the reference's layout"),
        ("rt_debug_adapt_fold", (None, 1, B, B, 1, None, None, 0, U, U, D, I), NULL_ARG),
        ("rt_debug_adapt_fold", (B, 0, B, B, 1, None, None, 0, U, U, D, I), NULL_ARG),
        ("rt_debug_adapt_fold", (B, 1, None, B, 1, None, None, 0, U, U, D, I), NULL_ARG),
        ("rt_debug_adapt_fold", (B, 1, B, None, 1, None, None, 0, U, U, D, I), NULL_ARG),
        ("rt_debug_adapt_fold", (B, 1, B, B, 1, None, None, 0, None, U, D, I), NULL_ARG),
        ("rt_debug_adapt_fold", (B, 1, B, B, 1, None, None, 0, U, None, D, I), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (None, 1, B, B, 1, 1, None, None, 0, U, U, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (B, 0, B, B, 1, 1, None, None, 0, U, U, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (B, 1, None, B, 1, 1, None, None, 0, U, U, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (B, 1, B, None, 1, 1, None, None, 0, U, U, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (B, 1, B, B, 1, 1, None, None, 0, None, U, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_adapt_shadow_side", (B, 1, B, B, 1, 1, None, None, 0, U, None, None, D, U, None, 0, U), NULL_ARG),
        ("rt_debug_fold_abandon", (None, 1, B, B, 1, 1, 0, I), NULL_ARG),
        ("rt_debug_fold_abandon", (B, 0, B, B, 1, 1, 0, I), NULL_ARG),
        ("rt_debug_fold_abandon", (B, 1, None, B, 1, 1, 0, I), NULL_ARG),
        ("rt_debug_fold_abandon", (B, 1, B, None, 1, 1, 0, I), NULL_ARG),
        ("rt_debug_rotate_tree", (None, 1, B, B, 1, 1, B, D, U, 3, 0.03), NULL_ARG),
        ("rt_debug_rotate_tree", (B, 0, B, B, 1, 1, B, D, U, 3, 0.03), NULL_ARG),
        ("rt_debug_rotate_tree", (B, 1, None, B, 1, 1, B, D, U, 3, 0.03), NULL_ARG),
        ("rt_debug_rotate_tree", (B, 1, B, None, 1, 1, B, D, U, 3, 0.03), NULL_ARG),
        ("rt_debug_rotate_tree", (B, 1, B, B, 1, 1, None, D, U, 3, 0.03), NULL_ARG),
        # the refit's host restatement: what it turns down before it writes
        ("rt_debug_refit", (None, None, 1, TR, 1, None, 0, 0, B, None), "no nodes or no triangles"),
        ("rt_debug_refit", (None, L, 0, TR, 1, None, 0, 0, B, None), "no nodes or no triangles"),
        ("rt_debug_refit", (None, L, 1, None, 1, None, 0, 0, B, None), "no nodes or no triangles"),
        ("rt_debug_refit", (None, L, 1, TR, 0, None, 0, 0, B, None), "no nodes or no triangles"),
        ("rt_debug_refit", (None, L, 1, TR, 2, None, 0, 0, B, None), "the leaves do not partition the triangle array"),
        ("rt_debug_refit", (None, N, 1, TR, 1, None, 0, 0, B, None), "the leaves do not partition the triangle array"),
        # ... and the pose's
        ("rt_debug_pose", (None, None, ID, 2, M, 1, B), NULL_ARG),
        ("rt_debug_pose", (None, TR, None, 2, M, 1, B), NULL_ARG),
        ("rt_debug_pose", (None, TR, ID, 2, None, 1, B), NULL_ARG),
        ("rt_debug_pose", (None, TR, ID, 2, M, 1, None), NULL_ARG),
        ("rt_debug_pose", (None, TR, ID, 0, M, 1, B), "no triangles"),
        ("rt_debug_pose", (None, TR, ID, 2, M, 0, B), "no objects"),
        ("rt_debug_pose", (None, TR, ID, 2, M, 1, B), "an object index is not below num_objects"),
        ("rt_debug_pose", (None, TR, ID, 2, M, 3, B), "an object index is not below num_objects"),
        ("rt_debug_pose", (None, TR, ID, 1, MN, 1, B), "a matrix entry is not finite"),
    ]
    silent = {"rt_scene_tree_report", "rt_debug_fold_view_left"}          # refuse without a message: below
    assert {name for name, _, _ in table} | silent == {n for n in capi.EXPORTS if n.startswith(("rt_scene_upload", "rt_scene_refit", "rt_scene_set_objects",
        "rt_scene_pose", "rt_scene_export_folds", "rt_scene_import_folds", "rt_scene_tree_report", "rt_debug_wide_bvh", "rt_debug_pair_layout", "rt_debug_own_bvh",
        "rt_debug_check_folds", "rt_debug_choose_tree", "rt_debug_device_fold", "rt_debug_device_tree", "rt_debug_count_box_passes", "rt_debug_adapt_", "rt_debug_fold_", "rt_debug_rotate_tree",
        "rt_debug_refit", "rt_debug_pose"))}
    for name, args, text in table:
        rc = getattr(lib, name)(*args)
        said = lib.rt_last_error(None).decode()
        assert rc != 0 and said == name + ": " + text, (name, args, rc, said)
    # each kind of entry answers a refusal in its own way: RT_ERROR, or -1 where the answer is a verdict or a time
    assert lib.rt_scene_upload(None, None) == 1 and lib.rt_debug_refit(None, None, 1, TR, 1, None, 0, 0, B, None) == 1
    assert lib.rt_debug_adapt_shadow_side(None, 1, B, B, 1, 1, None, None, 0, U, U, None, D, U, None, 0, U) == -1
    assert lib.rt_debug_fold_abandon(None, 1, B, B, 1, 1, 0, I) == -1.0
    # the two that refuse without a message
    lib.rt_debug_pose(None, None, None, 0, None, 0, None)
    assert lib.rt_scene_tree_report(None) == b""
    for args in ((None, B, 1.0), (B, None, 1.0), (None, None, 0.0)):
        assert lib.rt_debug_fold_view_left(*args) == -1
    assert lib.rt_last_error(None).decode() == "rt_debug_pose: " + NULL_ARG
    assert not scratch.any()                    # nothing was written through a refused call's arguments
    assert not interior.view(np.uint8).any() and not tris.view(np.uint8).any() and ids.tolist() == [0, 3]
