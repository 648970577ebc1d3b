"""-m gpu: the UV atlas on the device (raytracing_amd/csrc/atlas.hip).  The kernels against the host restatement byte for byte -- which
tests/test_atlas.py compares with Python integers --, the uploaded scene's cover with either tree form and across a pose, the surfaces of the posed
triangles, the bake into the atlas against rt_scene_bake of those surfaces, and the buffer forms' stream order.  One process, every step once."""
import ctypes as C
import numpy as np
import pytest
from raytracing_amd import capi, scenes as S, types as T
from tests.test_atlas import CASES, INVALID, f32, run, same_cover, random_triangles, triangles_of, refused
from tests.test_gpu_pose import context, scene_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same_bytes(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---- the cover kernels against the host restatement

@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_equal_the_host_restatement_on_the_rules_cases(ctx, name):
    uv, w, h, kw = CASES[name]
    same_cover(run(ctx, uv, w, h, **kw), run(None, uv, w, h, **kw), name)
    same_cover(run(ctx, uv, w, h, own=False, **kw), run(None, uv, w, h, own=False, **kw), name + " (uv override)")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_small_and_large_triangles_within_one_wave(ctx, n):
    """at 64 x 64 the small ones' boxes are at most 2 x 2 texels (each lane tests its own), the others span tiles (the wave sweeps them)"""
    for small, gutter in ((0.5, 1), (0.0, 0), (1.0, 0)):                     # mixed within a wave; every lane large; every lane small
        uv = random_triangles(n, 1000 + n, small)
        same_cover(run(ctx, uv, 64, 64, gutter=gutter), run(None, uv, 64, 64, gutter=gutter), (n, small))


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (130, 67), (16384, 1)])
def test_atlas_sizes(ctx, w, h):
    uv = random_triangles(30, 7, 0.3)
    same_cover(run(ctx, uv, w, h, gutter=2), run(None, uv, w, h, gutter=2), (w, h))


def test_one_triangle_over_a_whole_atlas_and_random_overlaps(ctx):
    whole = [[-1, -1, 3, -1, -1, 3]]
    got = run(ctx, whole, 256, 256)
    assert got[1]["covered"] == 256 * 256 and (got[0]["count"] == 1).all()
    same_cover(got, run(None, whole, 256, 256), "whole")
    uv = random_triangles(200, 11, 0.2)                                       # deliberate overlaps: the atomicMin and the count paths
    got = run(ctx, uv, 64, 64)
    assert got[1]["overlapped"] > 100 and got[0]["count"].max() > 4
    same_cover(got, run(None, uv, 64, 64), "random")
    ids = (np.arange(200) % 3).astype(np.uint32)
    same_cover(run(ctx, uv, 64, 64, gutter=1, object=2, ids=ids), run(None, uv, 64, 64, gutter=1, object=2, ids=ids), "object")


# ---- the uploaded scene

def atlas_of(tris):
    columns, rows = S.synthetic_atlas_grid(len(tris), 1, 1)
    return S.synthetic_atlas(tris, 3 * columns, 3 * rows), 3 * columns, 3 * rows


@pytest.mark.parametrize("name", ["cornell", "coverage"])
@pytest.mark.parametrize("wide", [True, False])
def test_the_scenes_cover_equals_the_host(name, wide, golden_scenes):
    sc = golden_scenes[name]
    uv, w, h = atlas_of(sc["triangles"])
    c = context(refittable=False, wide=wide)
    try:
        c.upload_scene(sc)
        for gutter in (0, 2):
            want = capi.debug_atlas(None, sc["triangles"], w, h, gutter, uv=uv)
            assert want[1]["overlapped"] == 0 and want[1]["triangles_without_texel"] == 0
            same_cover(c.atlas(w, h, gutter, uv=uv), want, (name, wide, gutter))
        same_cover(c.atlas(64, 48, 1), capi.debug_atlas(None, sc["triangles"], 64, 48, 1), "the triangles' own UVs")
    finally:
        c.close()


def test_after_a_pose_the_cover_holds_and_the_surfaces_follow(golden_scenes):
    sc, ids, n, mats = scene_case("cornell", golden_scenes, None)
    uv, w, h = atlas_of(sc["triangles"])
    c = context()
    try:
        c.upload_scene(sc)
        c.set_objects(ids, n)
        cover, _ = c.atlas(w, h, 1, uv=uv)
        rest = c.atlas_surfaces(cover)
        same_bytes(rest, capi.atlas_surfaces_host(sc["triangles"], cover, ids), "rest pose")
        c.pose_scene(mats)
        posed = capi.debug_pose(None, sc["triangles"], ids, mats)
        moved = c.atlas_surfaces(cover)                                       # the SAME cover: it depends on the UVs alone
        same_bytes(moved, capi.atlas_surfaces_host(posed, cover, ids), "posed")
        assert moved.tobytes() != rest.tobytes()
        same_bytes(c.atlas(w, h, 1, uv=uv)[0], cover, "a fresh cover after the pose")
        filtered = c.atlas(w, h, 0, object=1, uv=uv)
        same_cover(filtered, capi.debug_atlas(None, sc["triangles"], w, h, 0, 1, ids, uv=uv), "object filter on the scene")
        assert filtered[1]["triangles_filtered"] == int((ids != 1).sum())
    finally:
        c.close()


# ---- the bake into the atlas

def test_bake_atlas_equals_the_bake_of_the_atlas_surfaces(golden_scenes):
    sc = golden_scenes["cornell"]
    uv = S.synthetic_atlas(sc["triangles"], 32, 32) * f32(0.75)                    # (the charts leave a margin: uncovered texels, room for a gutter)
    c = context(refittable=False)
    try:
        c.upload_scene(sc)
        out, texels, stats = c.bake_atlas(32, 32, 16, seed=3, radius=0.5, uv=uv)
        cover = c.atlas(32, 32, uv=uv)
        same_cover((texels, stats), cover, "the cover bake_atlas returns")
        want = c.bake(c.atlas_surfaces(texels), 16, seed=3, radius=0.5, from_surfaces=True)
        same_bytes(out, want, "bake_atlas against bake(atlas_surfaces)")
        uncovered = texels["flags"] == 0
        assert uncovered.any() and (out["unoccluded"][uncovered] == INVALID).all() and (out["unoccluded"][~uncovered] <= 16).all()
        assert ((out["unoccluded"] > 0) & (out["unoccluded"] < 16)).any()          # a bake that did nothing cannot pass
        c.set_bake_chunk_points(100)                                                # eleven chunks, the last one short
        chunked, _, _ = c.bake_atlas(32, 32, 16, seed=3, radius=0.5, uv=uv)
        same_bytes(chunked, out, "chunk size")
        c.set_bake_chunk_points(0)
        guttered, gt, _ = c.bake_atlas(32, 32, 16, seed=3, radius=0.5, gutter=2, uv=uv)
        same_bytes(guttered, c.bake(c.atlas_surfaces(gt), 16, seed=3, radius=0.5, from_surfaces=True), "with a gutter")
        assert (guttered["unoccluded"][gt["flags"] == capi.TEXEL_GUTTER] <= 16).all() and (gt["flags"] == capi.TEXEL_GUTTER).any()
    finally:
        c.close()


# ---- the buffer forms only enqueue

def test_buffer_forms_in_stream_order_equal_the_host_forms(golden_scenes):
    sc = golden_scenes["cornell"]
    uv, w, h = atlas_of(sc["triangles"])
    c = context(refittable=False)
    bufs = []
    try:
        c.upload_scene(sc)
        make = lambda a: bufs.append(c.create_buffer(a)) or bufs[-1]
        for gutter in (0, 1, 2):                                                    # the ping-pong ends in the caller's buffer either way
            b_uv, b_tx, b_st, b_sf = make(uv), make(np.zeros(w * h, T.texel)), make(np.zeros(1, T.atlas_stats)), make(np.zeros(w * h, T.surface))
            c.atlas_buffer(w, h, b_tx, gutter, uv=b_uv, stats=b_st)
            c.atlas_surfaces_buffer(b_tx, w * h, b_sf)
            c.finish()
            texels, stats = c.atlas(w, h, gutter, uv=uv)
            same_cover((b_tx.read(T.texel, w * h), b_st.read(T.atlas_stats, 1)[0]), (texels, stats), gutter)
            same_bytes(b_sf.read(T.surface, w * h), c.atlas_surfaces(texels), gutter)
        wild = np.zeros(3, T.texel)
        wild["primitive_id"] = [0, len(sc["triangles"]), INVALID]
        b_w, b_o = make(wild), make(np.zeros(3, T.surface))
        c.atlas_surfaces_buffer(b_w, 3, b_o)
        assert b_o.read(T.surface, 3)["primitive_id"].tolist() == [0, INVALID, INVALID]   # beyond the scene: a miss record in the buffer form ...
        refused("rt_scene_atlas_surfaces: a record's primitive_id is not below the scene's triangle count", c.atlas_surfaces, wild)   # ... refused by the host form
    finally:
        for b in bufs:
            b.close()
        c.close()


# ---- refusals that need a context

def test_refusals(golden_scenes):
    sc, ids, n, _ = scene_case("cornell", golden_scenes, None)
    c, other = context(), capi.Context(0)
    bufs = []
    try:
        refused("rt_scene_atlas: no scene uploaded", c.atlas, 8, 8)
        refused("rt_scene_atlas_bake: no scene uploaded", c.bake_atlas, 8, 8, 16)
        refused("rt_scene_atlas_surfaces: no scene uploaded", c.atlas_surfaces, np.zeros(1, T.texel))
        c.upload_scene(sc)
        lib, d, bd, tx, out = c.lib, capi.atlas_desc(8, 8), capi.bake_desc(16), np.zeros(64, T.texel), np.zeros(64, T.bake_result)
        for call, msg in ((lambda: lib.rt_scene_atlas(c.handle, None, None, tx.ctypes.data, None), "rt_scene_atlas: desc is NULL"),
                          (lambda: lib.rt_scene_atlas(c.handle, C.byref(d), None, None, None), "rt_scene_atlas: texels is NULL"),
                          (lambda: lib.rt_scene_atlas_buffer(c.handle, C.byref(d), None, None, None), "rt_scene_atlas_buffer: texels is NULL"),
                          (lambda: lib.rt_scene_atlas_surfaces(c.handle, tx.ctypes.data, 64, None), "rt_scene_atlas_surfaces: surfaces is NULL"),
                          (lambda: lib.rt_scene_atlas_bake(c.handle, C.byref(d), None, None, out.ctypes.data, None, None), "rt_scene_atlas_bake: bake_desc is NULL"),
                          (lambda: lib.rt_scene_atlas_bake(c.handle, C.byref(d), None, C.byref(bd), None, None, None), "rt_scene_atlas_bake: out is NULL")):
            assert call() != 0 and lib.rt_last_error(c.handle).decode() == msg
        for fn in (c.atlas, lambda w, h, **k: c.bake_atlas(w, h, 16, **k)):
            refused("width and height must be 1 .. 16384", fn, 0, 8)
            refused("width and height must be 1 .. 16384", fn, 16384, 8192)
            refused("gutter must be 0 .. 4", fn, 8, 8, gutter=5)
            refused("desc.object needs rt_scene_set_objects", fn, 8, 8, object=0)
        refused("rt_scene_atlas_bake: bake_desc->flags must be 0", c.bake_atlas, 8, 8, 16, flags=capi.BAKE_FROM_SURFACES)
        refused("rt_scene_atlas_bake: samples must be a power of two", c.bake_atlas, 8, 8, 17)
        c.set_objects(ids, n)
        refused("rt_scene_atlas: desc.object is not below the object count", c.atlas, 8, 8, object=n)
        make = lambda who, a: bufs.append(who.create_buffer(a)) or bufs[-1]
        mine, small, theirs = make(c, np.zeros(64, T.texel)), make(c, np.zeros(63, T.texel)), make(other, np.zeros(64, T.texel))
        refused("rt_scene_atlas_buffer: the texels buffer is smaller than n records", c.atlas_buffer, 8, 8, small)
        refused("rt_scene_atlas_buffer: the texels buffer belongs to another context", c.atlas_buffer, 8, 8, theirs)
        refused("rt_scene_atlas_buffer: the uv buffer is smaller than n records", c.atlas_buffer, 8, 8, mine, uv=make(c, np.zeros(6 * len(ids) - 1, f32)))
        refused("rt_scene_atlas_buffer: the stats buffer belongs to another context", c.atlas_buffer, 8, 8, mine, stats=theirs)
        refused("rt_scene_atlas_surfaces_buffer: the surfaces buffer is smaller than n records", c.atlas_surfaces_buffer, mine, 64, small)
        c.atlas_buffer(8, 8, mine)                                                  # and the scene still answers
        c.finish()
    finally:
        for b in bufs:
            b.close()
        c.close()
        other.close()
