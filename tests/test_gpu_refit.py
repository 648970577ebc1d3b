"""-m gpu: rt_scene_refit / rt_scene_refit_buffer (raytracing_amd/csrc/refit.hip) on the device.

The contract: after a refit the context behaves exactly as a FRESH context would after rt_scene_upload of the moved triangles with the node array "same
topology, same split axes, bounds refitted" (tests/test_refit.py: np_refit).  So context A uploads the first pose, renders, refits, resets and renders; context B
is fresh and uploads (moved triangles, numpy-refitted nodes); radiance, resolved image and ray counters are compared bit for bit, and with the CPU oracle where it
renders the scene.  The kernels alone: rt_debug_refit on the device against the host restatement, bit for bit (bounds by value).
One process, no retries; nothing here provokes a fault."""
import os
import numpy as np
import pytest
from tests import _oracle
from tests.test_refit import np_refit, smooth, jitter, same_nodes, same_records, positions, moved
from tests.test_wide_bvh import wide_of, bvh_of
from raytracing_amd import capi, host, scenes as S, types as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BOUNCES = 96, 64, 4
OPT_REFITTABLE, OPT_ADAPT_WAIT, OPT_WIDE_LAYOUT, OPT_TREE_BUILDER = 10, 6, 8, 9


@pytest.fixture(scope="module")
def city():
    scene = host.Scene(arrays=S.city_block(40_000))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    sc = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
    assert len(sc["nodes"]) >= 8192                                   # large enough for the default fold adaptation
    return sc


def posed(sc, tris):
    """the scene a fresh context uploads for a pose: the moved triangles and the refitted node array"""
    out = dict(sc)
    out["triangles"] = tris
    out["nodes"] = np_refit(sc["nodes"], tris)
    return out


def context(ctx_options=(), refittable=False, blue=False):
    c = capi.Context(0)
    for opt, value in ctx_options:
        assert c.lib.rt_ctx_set_option(c.handle, opt, value) == 0
    if refittable:
        c.set_refittable(True)
    if blue:
        c.upload_blue_noise_tables(*S.blue_noise_tables())
    return c


def stage_sample(fr, bounces):
    fr.generate_rays()
    for b in range(bounces + 1):
        fr.intersect(b); fr.shade(b); fr.intersect_shadow(b)
    fr.advance_sample()


def frame(ctx, cam, frame_options=()):
    fr = capi.Frame(ctx, W, H)
    fr.set_camera(cam)
    fr.set_max_bounces(BOUNCES)
    for opt, value in frame_options:
        fr.set_option(opt, value)
    return fr


def shoot(fr, spp, stages=False):
    fr.reset()
    if stages:
        for _ in range(spp):
            stage_sample(fr, BOUNCES)
    else:
        fr.integrate(spp)
    st = fr.stats()
    return fr.radiance().copy(), fr.resolve().copy(), (st.closest_rays, st.shadow_rays)


def same_shot(a, b, what=""):
    assert a[2] == b[2], (what, a[2], b[2])
    assert a[0].tobytes() == b[0].tobytes(), what
    assert a[1].tobytes() == b[1].tobytes(), what


CASES = {
    # name: (context options, frame options, stage calls, blue noise, wait for the adaptation before the refit)
    "defaults": ((), (), False, False, False),
    "wide_tree_off": (((1, 0),), (), False, False, False),
    "shadow_tree_shared": (((2, 0),), (), False, False, False),
    "shadow_tree_own_always": (((2, 2),), (), False, False, False),
    "shadow_tree_device_builder": (((2, 2), (OPT_TREE_BUILDER, 1)), (), False, False, False),
    "adaptation_waited_for": (((4, capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4),), (), False, False, True),
    "pair_layout": (((OPT_WIDE_LAYOUT, 1),), (), False, False, False),
    "stage_calls": ((), (), True, False, False),
    "samples_ahead": ((), ((capi.OPT_SAMPLES_AHEAD, 8),), True, False, False),
    "frame_kernel": ((), ((capi.OPT_FRAME_KERNEL, 1),), False, False, False),
    "blue_noise": ((), ((capi.OPT_SAMPLER, 1),), False, True, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_rendered_parity_with_a_fresh_upload(case, city):
    ctx_options, frame_options, stages, blue, wait = CASES[case]
    spp = 8 if case == "samples_ahead" else 3                         # enough stage samples for a bank to be traced ahead and consumed
    cam = T.default_camera(W, H)
    pose = smooth(city["triangles"], 0.03, 0.5)
    a = context(ctx_options, refittable=True, blue=blue)
    b = context(ctx_options, blue=blue)
    try:
        a.upload_scene(city)
        if wait:
            assert a.lib.rt_ctx_set_option(a.handle, OPT_ADAPT_WAIT, 1) == 0
        fa = frame(a, cam, frame_options)
        first = shoot(fa, spp, stages)
        if case == "samples_ahead":
            assert fa.stats().samples_ahead > 0
        if wait:
            assert "adaptive fold" in a.tree_report(), a.tree_report()
        a.refit_scene(pose)
        assert "refit 1" in a.tree_report() and "no longer qualifies" not in a.tree_report(), a.tree_report()
        got = shoot(fa, spp, stages)
        b.upload_scene(posed(city, pose))
        fb = frame(b, cam, frame_options)
        want = shoot(fb, spp, stages)
        same_shot(got, want, case)
        assert got[0].tobytes() != first[0].tobytes()                 # the pose does move what the camera sees
        if case == "defaults":
            orc = _oracle.Oracle(W, H, posed(city, pose))
            orc.set_camera(cam)
            orc.set_max_bounces(BOUNCES)
            orc.integrate(3)
            assert np.array_equal(got[0][..., :3], orc.radiance()[..., :3])
            assert got[2] == orc.ray_totals()
    finally:
        a.close(); b.close()


def test_emissive_nee_scene_against_the_oracle(golden_scenes):
    sc = dict(golden_scenes["coverage"])
    sc["flags"] = 1
    cam = T.default_camera(W, H)
    pose = smooth(sc["triangles"], 0.04, 2.0)
    a, b = context(refittable=True), context()
    try:
        a.upload_scene(sc)
        fa = frame(a, cam)
        shoot(fa, 2)
        a.refit_scene(pose)
        got = shoot(fa, 3)
        b.upload_scene(posed(sc, pose))
        same_shot(got, shoot(frame(b, cam), 3))
        orc = _oracle.Oracle(W, H, posed(sc, pose))
        orc.set_camera(cam)
        orc.set_max_bounces(BOUNCES)
        orc.integrate(3)
        assert np.array_equal(got[0][..., :3], orc.radiance()[..., :3])
        assert got[2] == orc.ray_totals()
    finally:
        a.close(); b.close()


def test_eight_refits_in_a_row_and_back_to_the_first_pose(city):
    cam = T.default_camera(W, H)
    a, b = context(refittable=True), context()
    try:
        a.upload_scene(city)
        fa = frame(a, cam)
        first = shoot(fa, 3)
        buf = a.create_buffer(city["triangles"])
        for k in range(1, 9):
            pose = smooth(city["triangles"], 0.01 * k, 0.3 * k)
            if k % 2:
                a.refit_scene(pose)
            else:                                                     # the buffer variant: the triangles are on the device already
                buf.write(pose)
                a.refit_scene(buf)
        assert "refit 8" in a.tree_report()
        got = shoot(fa, 3)
        b.upload_scene(posed(city, pose))
        same_shot(got, shoot(frame(b, cam), 3), "eight refits")
        a.refit_scene(city["triangles"])
        same_shot(shoot(fa, 3), first, "back to the first pose")
        buf.close()
    finally:
        a.close(); b.close()


def test_the_buffer_variant_equals_the_host_pointer_variant(city):
    cam = T.default_camera(W, H)
    pose = jitter(city["triangles"], np.random.default_rng(4), 0.002)
    a, b = context(refittable=True), context(refittable=True)
    try:
        a.upload_scene(city); b.upload_scene(city)
        a.refit_scene(pose)
        buf = b.create_buffer(pose)
        b.refit_scene(buf)
        same_shot(shoot(frame(a, cam), 2), shoot(frame(b, cam), 2))
        buf.close()
    finally:
        a.close(); b.close()


def test_a_pose_that_disqualifies_a_wide_record_renders_through_the_fallback(city):
    cam = T.default_camera(W, H)
    far = positions(city["triangles"]).copy()
    far[11, 1, 2] = np.float32(-3e8)                                  # one vertex beyond 2^28 (far below the camera)
    pose = moved(city["triangles"], far)
    a, b = context(refittable=True), context(((1, 0),))              # b: no wide tree at all -- the BVH2 kernels
    try:
        a.upload_scene(city)
        fa = frame(a, cam)
        first = shoot(fa, 2)
        a.refit_scene(pose)
        assert "no longer qualifies" in a.tree_report(), a.tree_report()
        got = shoot(fa, 2)
        b.upload_scene(posed(city, pose))
        same_shot(got, shoot(frame(b, cam), 2), "fallback")
        a.refit_scene(city["triangles"])                               # the next pose qualifies: the wide kernel again
        assert "the 4-wide trees qualify" in a.tree_report(), a.tree_report()
        same_shot(shoot(fa, 2), first, "after the fallback")
    finally:
        a.close(); b.close()


def test_every_refusal_leaves_the_next_render_as_it_was(city):
    cam = T.default_camera(W, H)
    off = context()
    a = context(refittable=True)
    try:
        off.upload_scene(city)
        with pytest.raises(capi.RtError, match="RT_CTX_OPT_REFITTABLE"):
            off.refit_scene(city["triangles"])
        with pytest.raises(capi.RtError, match="no scene"):
            a.refit_scene(city["triangles"])
        a.upload_scene(city)
        fa = frame(a, cam)
        before = shoot(fa, 2)
        with pytest.raises(capi.RtError, match="count"):
            a.refit_scene(city["triangles"][:-1])
        buf = a.create_buffer(city["triangles"][:-1])
        with pytest.raises(capi.RtError, match="count"):
            a.refit_scene(buf)
        buf.close()
        bad = smooth(city["triangles"], 0.05)
        bad["v3"]["position"]["z"][len(bad) // 2] = np.nan
        with pytest.raises(capi.RtError, match="non-finite"):
            a.refit_scene(bad)
        bad = smooth(city["triangles"], 0.05)
        bad["mtl_index"][5] = len(city["materials"])
        with pytest.raises(capi.RtError, match="material index"):
            a.refit_scene(bad)
        a.set_closest_tree(1)
        with pytest.raises(capi.RtError, match="tolerance"):
            a.refit_scene(smooth(city["triangles"], 0.05))
        a.set_closest_tree(0)
        assert a.lib.rt_scene_refit(a.handle, None, 0) != 0 and a.lib.rt_scene_refit(None, None, 0) != 0
        assert "refit" not in a.tree_report()
        same_shot(shoot(fa, 2), before, "after the refusals")
    finally:
        off.close(); a.close()


def test_guides_and_the_temporal_filter_after_a_refit_equal_a_fresh_context(city):
    cam = T.default_camera(W, H)
    pose = smooth(city["triangles"], 0.03, 0.5)
    a, b = context(refittable=True), context()
    try:
        a.upload_scene(city)
        fa = frame(a, cam)
        shoot(fa, 2)
        fa.guides()
        fa.filter_temporal()                                          # a history of the first pose
        a.refit_scene(pose)
        shoot(fa, 2)
        b.upload_scene(posed(city, pose))
        fb = frame(b, cam)
        shoot(fb, 2)
        for x, y in zip(fa.guides()[:3], fb.guides()[:3]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        assert np.asarray(fa.filter_temporal()).tobytes() == np.asarray(fb.filter_temporal()).tobytes()      # history dropped: the first call on both
    finally:
        a.close(); b.close()


def test_two_tiles_on_one_device_through_host_render():
    def scene_of():
        s = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
        s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
        return s
    cam = host.default_camera(W, H)
    renders = [host.Render(W, H, scene_of(), tile_rank=r, tile_count=2) for r in range(2)]
    tris = renders[0].scene_arrays()["triangles"].copy()
    nodes = renders[0].scene_arrays()["nodes"].copy()
    pose = smooth(tris, 0.02, 1.0)
    got = []
    for r in renders:
        r.set_refittable(True)
        r.set_camera(cam); r.set_max_bounces(BOUNCES)
        r.render_samples(2)
        r.refit(pose)
        r.render_samples(3)
        assert r.sample_count() == 3                                  # the refit requested a reset
        got.append((r.radiance().copy(), r.stats()))
    arrays = dict(renders[0].scene_arrays())
    arrays["triangles"], arrays["nodes"] = pose, np_refit(nodes, pose)
    c = capi.Context(0)
    try:
        c.upload_scene(arrays)
        for rank in range(2):
            fr = capi.Frame(c, W, H, tile_rank=rank, tile_count=2)
            fr.set_camera(cam); fr.set_max_bounces(BOUNCES)
            fr.integrate(3)
            assert fr.radiance().tobytes() == got[rank][0].tobytes()
            st = fr.stats()
            assert (st.closest_rays, st.shadow_rays) == (got[rank][1].closest_rays, got[rank][1].shadow_rays)
            fr.close()
    finally:
        c.close()


def test_debug_refit_on_the_device_equals_the_host_restatement(golden_scenes):
    ctx = capi.Context(0)
    rng = np.random.default_rng(2)
    try:
        cases = [(golden_scenes[k]["nodes"], golden_scenes[k]["triangles"]) for k in ("cornell", "coverage")]
        cases.append(bvh_of(*S.cornell_blob(871_200, 20_000)))        # about a million triangles
        for nodes, tris in cases:
            for collapse in (1, 2):
                rec, entry = wide_of(nodes, collapse)
                for pose in (smooth(tris, 0.05), jitter(tris, rng, 0.01)):
                    hn, hr, hbad = capi.debug_refit(None, nodes, pose, rec, entry)
                    dn, dr, dbad = capi.debug_refit(ctx, nodes, pose, rec, entry)
                    assert hbad == dbad
                    same_nodes(dn, hn)
                    same_records(dr, hr)
        # a leaf root, and a pose that disqualifies records: the same flag, the same bytes
        nodes, tris = bvh_of(S.to_triangles([(np.eye(3, dtype=np.float32).reshape(1, 3, 3), np.zeros((1, 3, 3), np.float32), np.zeros((1, 3, 2), np.float32), 0)]),
                             np.array([S.make_material()], dtype=T.packed_material))
        same_nodes(capi.debug_refit(ctx, nodes, tris)[0], capi.debug_refit(None, nodes, tris)[0])
        nodes, tris = cases[1]
        rec, entry = wide_of(nodes)
        far = positions(tris).copy()
        far[3, 0, 1] = np.float32(3e8)
        hn, hr, hbad = capi.debug_refit(None, nodes, moved(tris, far), rec, entry)
        dn, dr, dbad = capi.debug_refit(ctx, nodes, moved(tris, far), rec, entry)
        assert hbad and dbad
        same_nodes(dn, hn)
        same_records(dr, hr)
    finally:
        ctx.close()
