"""The refit of a scene's trees when its triangles move (raytracing_amd/csrc/refit.hip), checked ON THE CPU through the host restatement
of the kernels' rule (rt_debug_refit with ctx = NULL):

  * the node array: offsets, counts and axes untouched, leaf bounds = min / max over the leaf's vertices, interior bounds = min / max of the two children --
    against ten lines of numpy (children follow their parent in the reference's layout, so one pass from the last node to the first does it);
  * any fold of it, record by record, bottom-up, from the leaf boxes alone: the refitted records are a valid fold of the refitted nodes by test_wide_bvh.check,
    which asserts containment, representability AND tightness to one cell -- a refit that merely grows boxes fails;
  * with the triangles unmoved the records come back byte for byte: the quantisation is the builder's own function;
  * a leaf root, two triangles, coordinates that disqualify a record (the flag is raised, the record's bytes stay).

Float bounds are compared by VALUE (min / max leave the sign of a zero to the operand order), records bit for bit except the frame origin (a float: by value).
The device half is tests/test_gpu_refit.py."""
import os
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_wide_bvh import check, wide_of, bvh_of, WIDE
from tests.test_own_tree import own_tree
from tests._trees import refit_soup, leaf_root_scene, two_triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = np.array([S.make_material(kd=(0.7, 0.7, 0.7))], dtype=T.packed_material)


def positions(tris):
    """float32[nt, 3 vertices, 3]"""
    return np.stack([np.stack([tris[v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1)


def moved(tris, P):
    out = tris.copy()
    for k, v in enumerate(("v1", "v2", "v3")):
        for a, c in enumerate("xyz"):
            out[v]["position"][c] = P[:, k, a]
    return out


def smooth(tris, amplitude=0.05, phase=0.0):
    """every vertex displaced by a smooth field of its position (shared vertices stay shared), scaled to the scene"""
    P = positions(tris).astype(np.float64)
    size = float(np.ptp(P.reshape(-1, 3), axis=0).max()) or 1.0
    Q = P / size * 5.0 + phase
    D = np.stack([np.sin(Q[..., 1] * 1.3 + Q[..., 2]), np.cos(Q[..., 0] * 0.7 - Q[..., 2] * 1.1), np.sin(Q[..., 0] + Q[..., 1] * 0.9)], -1)
    return moved(tris, (P + amplitude * size * D).astype(np.float32))


def jitter(tris, rng, amplitude=0.05):
    P = positions(tris).astype(np.float64)
    size = float(np.ptp(P.reshape(-1, 3), axis=0).max()) or 1.0
    return moved(tris, (P + rng.normal(size=P.shape) * amplitude * size).astype(np.float32))


def np_refit(nodes, tris):
    """the reference refit: children follow parents in the node array (c0 = i + 1, c1 = offset > i)"""
    out = nodes.copy()
    P = positions(tris)
    lo, hi = np.zeros((len(nodes), 3), np.float32), np.zeros((len(nodes), 3), np.float32)
    for i in range(len(nodes) - 1, -1, -1):
        n, off = int(nodes["num_primitives_axis"][i]) >> 16, int(nodes["offset"][i])
        if n:
            lo[i], hi[i] = P[off:off + n].reshape(-1, 3).min(0), P[off:off + n].reshape(-1, 3).max(0)
        else:
            lo[i], hi[i] = np.minimum(lo[i + 1], lo[off]), np.maximum(hi[i + 1], hi[off])
    for a, c in enumerate("xyz"):
        out["bounds_min"][c], out["bounds_max"][c] = lo[:, a], hi[:, a]
    return out


def same_nodes(got, want):
    for f in ("offset", "num_primitives_axis"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("bounds_min", "bounds_max"):
        for c in "xyz":
            assert np.array_equal(got[f][c], want[f][c]), (f, c)      # by value: -0 equals +0


def same_records(got, want):
    got, want = got.view(WIDE).reshape(-1), want.view(WIDE).reshape(-1)
    assert np.array_equal(got["origin"], want["origin"])
    for f in ("meta", "lo", "hi", "ref", "order", "pad"):
        assert got[f].tobytes() == want[f].tobytes(), f


def refit_and_check(nodes, tris, folds):
    """nodes refitted to tris against numpy; every fold (records, entry, roots) of `nodes` refitted and validated as a fold of the refitted nodes"""
    want = np_refit(nodes, tris)
    for rec, entry, roots in folds or [(None, 0, None)]:
        got, got_rec, bad = capi.debug_refit(None, nodes, tris, rec, entry)
        same_nodes(got, want)
        if rec is None or not len(rec):
            continue
        assert not bad
        for f in ("ref", "order", "pad"):
            assert got_rec[f].tobytes() == rec[f].tobytes(), f
        assert (got_rec["meta"] >> 24).tobytes() == (rec["meta"] >> 24).tobytes()
        check(want, 1, fold=(got_rec, entry, roots))
    return want


def folds_of(nodes):
    return [wide_of(nodes, 1, with_roots=True), wide_of(nodes, 2, with_roots=True)]


def scenes_of(golden_scenes):
    yield golden_scenes["cornell"]["nodes"], golden_scenes["cornell"]["triangles"]
    yield golden_scenes["coverage"]["nodes"], golden_scenes["coverage"]["triangles"]


def test_node_refit_and_folds_on_the_golden_scenes(golden_scenes):
    rng = np.random.default_rng(5)
    for nodes, tris in scenes_of(golden_scenes):
        folds = folds_of(nodes)
        for pose in (smooth(tris), smooth(tris, 0.3, 1.0), jitter(tris, rng), jitter(tris, rng, 0.5)):
            refit_and_check(nodes, pose, folds)


@pytest.mark.parametrize("seed", range(6))
def test_node_refit_and_folds_on_random_soups(seed):
    tris, mats, rng = refit_soup(seed)
    nodes, tris = bvh_of(tris, mats)
    folds = folds_of(nodes)
    refit_and_check(nodes, smooth(tris, 0.1), folds)
    refit_and_check(nodes, jitter(tris, rng, 0.2), folds)


def test_refit_of_the_shadow_rays_own_tree_and_of_an_adapted_fold(golden_scenes):
    """another binary tree over the same leaves (own_bvh.h) and its fold; a fold adapted to rays (FoldAdapt's host half): the same rule refits them"""
    rng = np.random.default_rng(9)
    nodes, tris = golden_scenes["coverage"]["nodes"], golden_scenes["coverage"]["triangles"]
    own = own_tree(nodes, 0.5, [(0.3, -0.8, 0.5)])
    pose = smooth(tris, 0.2)
    refit_and_check(own, pose, [wide_of(own, 1, with_roots=True)])
    P = positions(tris).reshape(-1, 3)
    o = np.concatenate([rng.uniform(P.min(0), P.max(0), (4000, 3)), np.full((4000, 1), 1e30)], 1).astype(np.float32)
    d = rng.normal(size=(4000, 4)).astype(np.float32)
    rec, entry, roots, cost, adopted = capi.adapt_fold(nodes, o, d)
    refit_and_check(nodes, pose, [(rec.view(WIDE).reshape(-1), entry, roots)])


def test_unmoved_triangles_give_the_records_back_byte_for_byte(golden_scenes):
    """node arrays whose leaf bounds are the exact min / max of the vertices and whose interior bounds are exact unions (host/bvh.cpp, the golden scenes):
    the refit changes no value, so every record must come back as the builder quantised it"""
    cases = list(scenes_of(golden_scenes))
    s = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    s.build_bvh()
    cases.append((s.arrays()["nodes"].copy(), s.arrays()["triangles"].copy()))
    cases.append(bvh_of(*S.cornell_blob(20_000, 2_000)))
    for nodes, tris in cases:
        same_nodes(np_refit(nodes, tris), nodes)
        for rec, entry, roots in folds_of(nodes):
            got, got_rec, bad = capi.debug_refit(None, nodes, tris, rec, entry)
            assert not bad
            same_nodes(got, nodes)
            same_records(got_rec, rec)


def test_refit_back_to_the_first_pose_reproduces_the_first_records(golden_scenes):
    nodes, tris = golden_scenes["coverage"]["nodes"], golden_scenes["coverage"]["triangles"]
    rec, entry, roots = wide_of(nodes, 1, with_roots=True)
    n1, r1, _ = capi.debug_refit(None, nodes, smooth(tris, 0.4), rec, entry)
    n2, r2, _ = capi.debug_refit(None, n1, tris, r1, entry)
    same_nodes(n2, nodes)
    same_records(r2, rec)


def test_a_leaf_root_and_a_two_triangle_scene():
    nodes, tris = bvh_of(*leaf_root_scene())
    assert len(nodes) == 1
    pose = moved(tris, positions(tris) + np.float32(3.0))
    got, rec, bad = capi.debug_refit(None, nodes, pose)
    same_nodes(got, np_refit(nodes, pose))
    assert rec is None and not bad
    check(got)
    nodes, tris = bvh_of(*two_triangle_scene())
    assert len(nodes) == 3
    refit_and_check(nodes, jitter(tris, np.random.default_rng(1), 0.3), folds_of(nodes))


def test_coordinates_that_disqualify_a_record_raise_the_flag():
    rng = np.random.default_rng(3)
    P = rng.normal(size=(64, 3, 3)).astype(np.float32)
    tris = S.to_triangles([(P, np.tile(np.array([0, 0, 1], np.float32), (64, 3, 1)), np.zeros((64, 3, 2), np.float32), 0)])
    nodes, tris = bvh_of(tris, MATS)
    rec, entry, roots = wide_of(nodes, 1, with_roots=True)
    far = positions(tris).copy()
    far[0, 0, 0] = np.float32(3e8)                                  # one vertex beyond 2^28: the records above it no longer qualify
    pose = moved(tris, far)
    got, got_rec, bad = capi.debug_refit(None, nodes, pose, rec, entry)
    assert bad
    same_nodes(got, np_refit(nodes, pose))                          # the exact bounds are refitted all the same
    assert got_rec[0].tobytes() == rec[0].tobytes()                 # the root record holds that vertex: left as it was
    with pytest.raises(capi.RtError, match="does not qualify"):
        wide_of(np_refit(nodes, pose))                              # ... exactly where the builder refuses the tree
    wide = positions(tris).copy()                                   # coordinates within 2^28, an extent that needs cells above 2^20
    wide[0, 0, 0], wide[1, 0, 0] = np.float32(2.6e8), np.float32(-2.6e8)
    assert capi.debug_refit(None, nodes, moved(tris, wide), rec, entry)[2]
    # the next pose qualifies again, from the flagged records on
    back, back_rec, bad = capi.debug_refit(None, got, tris, got_rec, entry)
    assert not bad
    same_records(back_rec, rec)


def test_input_that_is_not_a_refittable_tree_is_refused(golden_scenes):
    nodes, tris = golden_scenes["cornell"]["nodes"], golden_scenes["cornell"]["triangles"]
    rec, entry, roots = wide_of(nodes, 1, with_roots=True)
    bad = tris.copy()
    bad["v2"]["position"]["y"][7] = np.inf
    with pytest.raises(capi.RtError, match="non-finite"):
        capi.debug_refit(None, nodes, bad, rec, entry)
    with pytest.raises(capi.RtError, match="partition"):
        capi.debug_refit(None, nodes, tris[:-1], rec, entry)
    loop = rec.copy()
    loop["ref"][len(loop) - 1][0] = 0
    with pytest.raises(capi.RtError, match="not a tree"):
        capi.debug_refit(None, nodes, tris, loop, entry)


def test_the_symbols_are_declared_exported_and_bound():
    lib = capi.load()
    for name in ("rt_scene_refit", "rt_scene_refit_buffer", "rt_debug_refit"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "RT_CTX_OPT_REFITTABLE = 10" in text
    for name in ("rth_render_set_refittable", "rth_render_refit"):
        assert name in host.EXPORTS and hasattr(host.load(), name)
