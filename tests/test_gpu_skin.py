"""-m gpu: rt_scene_set_skin / rt_scene_skin (raytracing_amd/csrc/skin.hip) on the device.

The contract: after rt_scene_skin(M) the context is what rt_scene_refit of rt_debug_skin(NULL, rest, influences, M)'s output would have left.  So the kernel alone
is compared with the host restatement bit for bit (which tests/test_skin.py compares with numpy) on both of its palette paths, and context A (upload, set_skin,
skin) with context B (upload, refit of the restatement's triangles): radiance, counters, guides, the filters' outputs and histories, queries, bit for bit.  One
process, each GPU step once, nothing retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, scenes as S, types as T
from tests.test_refit import positions
from tests.test_pose import IDENTITY, translation, rotation, scale, same_bytes
from tests.test_skin import random_case, palette, np_skin
from tests.test_motion_filter import moving_triangles, STEP
from tests.test_gpu_temporal_filter import bits, moving_cameras
from tests.test_gpu_motion_filter import DESC
from tests.test_gpu_pose import context, camera, frame, shoot, same_shot, sequence, cornell_objects, city  # noqa: F401  (city: a module fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
K = capi.SKIN_LDS_BONES
W, H = 64, 64


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


# ---- the kernel against the host restatement: every tail shape, both palette paths

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1000])
def test_kernel_equals_host_restatement_bit_for_bit(ctx, n):
    rng = np.random.default_rng(200 + n)
    for n_bones in (1, 2, 7, K, K + 1, 4096):
        tris, infl, mats = random_case(rng, n, n_bones)
        same_bytes(capi.debug_skin(ctx, tris, infl, mats), capi.debug_skin(None, tris, infl, mats))
    tris, infl, _ = random_case(rng, n, 2)
    infl["weight"][:] = (0.5, 0.5, 0, 0)
    same_bytes(capi.debug_skin(ctx, tris, infl, np.stack([IDENTITY] * 2)), tris)


@pytest.mark.parametrize("n_bones", [K, K + 1, 4096])
def test_every_corner_on_four_different_shuffled_bones(ctx, n_bones):
    rng = np.random.default_rng(300 + n_bones)
    tris, infl, mats = random_case(rng, 257, n_bones, shuffled=True)
    assert all(len(set(b)) == 4 for b in infl["bone"].reshape(-1, 4).tolist())
    got = capi.debug_skin(ctx, tris, infl, mats)
    same_bytes(got, capi.debug_skin(None, tris, infl, mats))
    assert (positions(got) != positions(tris)).any()


def test_the_two_palette_paths_agree(ctx):
    """the same influences (bones below K) and the same first K matrices, once as a palette of K (staged in LDS) and once of K + 1 (gathered from memory)"""
    rng = np.random.default_rng(77)
    tris, infl, mats = random_case(rng, 513, K)
    more = np.concatenate([mats, palette(rng, 1)])
    staged, gathered = capi.debug_skin(ctx, tris, infl, mats), capi.debug_skin(ctx, tris, infl, more)
    same_bytes(staged, gathered)
    same_bytes(staged, capi.debug_skin(None, tris, infl, mats))


# ---- in a scene

def skin_case(name, golden_scenes, city):
    """the scene, its influences (BVH order), the bone count and a bend"""
    sc, n_bones, angle = (golden_scenes["cornell"], 7, 0.06) if name == "cornell" else (city, 64, 0.03)
    tris = sc["triangles"]
    infl = T.influences(*S.synthetic_skin(tris, n_bones))
    axis, lo, hi = S.skin_extent(tris)
    centre = positions(tris).reshape(-1, 3).astype(np.float64).mean(0)
    return sc, infl, n_bones, S.bend_palette(n_bones, angle, axis, lo, hi, centre=centre)


@pytest.mark.parametrize("wide", [True, False], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_a_skin_equals_the_refit_of_the_restatement(name, wide, golden_scenes, golden_radiance, city):
    sc, infl, n_bones, bend = skin_case(name, golden_scenes, city)
    cam = camera(name, golden_radiance)
    a, b = context(wide=wide), context(wide=wide)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        first = shoot(fa)
        a.set_skin(infl, n_bones)
        assert "skinned triangles: %d bones, 392 bytes per triangle" % n_bones in a.tree_report(), a.tree_report()
        a.skin_scene(bend)
        assert "refit 1:" in a.tree_report() and "skinned triangles: " in a.tree_report(), a.tree_report()
        b.refit_scene(capi.debug_skin(None, sc["triangles"], infl, bend))
        got = shoot(fa)
        same_shot(got, shoot(fb), name)
        assert got["radiance"].tobytes() != first["radiance"].tobytes()       # the skin does move what the camera sees
    finally:
        a.close(); b.close()


def test_skins_are_absolute(golden_scenes, golden_radiance):
    sc, infl, n, m2 = skin_case("cornell", golden_scenes, None)
    axis, lo, hi = S.skin_extent(sc["triangles"])
    m1 = S.bend_palette(n, -0.1, axis, lo, hi, about=(axis + 2) % 3)
    ident = np.stack([IDENTITY] * n)
    cam = camera("cornell", golden_radiance)
    a, b = context(), context()
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        uploaded = shoot(fa)
        a.set_skin(infl, n); b.set_skin(infl, n)
        a.skin_scene(m1)
        after_m1 = shoot(fa)
        a.skin_scene(m2)
        b.skin_scene(m2)
        want = shoot(fb)
        same_shot(shoot(fa), want, "M1 then M2 = M2")
        assert after_m1["radiance"].tobytes() != want["radiance"].tobytes()
        # a refit from a buffer in between does not become the rest pose
        buf = a.create_buffer(capi.debug_skin(None, sc["triangles"], infl, m1))
        a.refit_scene(buf)
        same_shot(shoot(fa), after_m1, "the refit itself")
        a.skin_scene(m2)
        same_shot(shoot(fa), want, "M2 after a refit in between")
        buf.close()
        a.skin_scene(ident)
        same_shot(shoot(fa), uploaded, "the identity palette gives the upload's image")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_scene_untouched(golden_scenes, golden_radiance):
    sc, infl, n, mats = skin_case("cornell", golden_scenes, None)
    cam = camera("cornell", golden_radiance)
    flat = np.ascontiguousarray(infl).reshape(-1)
    plain = context(refittable=False)
    try:
        plain.upload_scene(sc)
        fr = frame(plain, cam)
        before = shoot(fr)
        with pytest.raises(capi.RtError, match="rt_scene_set_skin: RT_CTX_OPT_REFITTABLE was off"):
            plain.set_skin(infl, n)
        with pytest.raises(capi.RtError, match="rt_scene_skin: RT_CTX_OPT_REFITTABLE was off"):
            plain.skin_scene(mats)
        same_shot(shoot(fr), before, "not refittable")
    finally:
        plain.close()
    c = context()
    try:
        with pytest.raises(capi.RtError, match="rt_scene_set_skin: no scene"):
            c.set_skin(infl, n)
        with pytest.raises(capi.RtError, match="rt_scene_skin: no scene"):
            c.skin_scene(mats)
        c.upload_scene(sc)
        fr = frame(c, cam)
        before = shoot(fr)
        report = c.tree_report()

        def refused(message, call, *args):
            with pytest.raises(capi.RtError, match=message):
                call(*args)
            same_shot(shoot(fr), before, message)

        def null_refused(rc, message):
            assert rc != 0 and message in c.lib.rt_last_error(c.handle).decode()
            same_shot(shoot(fr), before, message)

        def bad_table(edit):
            f = infl.copy()
            edit(f)
            return f

        refused("rt_scene_skin: no skin", c.skin_scene, mats)
        null_refused(c.lib.rt_scene_set_skin(c.handle, None, len(infl), n), "rt_scene_set_skin: NULL argument")
        refused("rt_scene_set_skin: the triangle count differs", c.set_skin, infl[:-1], n)
        refused("rt_scene_set_skin: no bones", c.set_skin, infl, 0)
        refused("rt_scene_set_skin: more than 65536 bones", c.set_skin, infl, 65537)
        refused("rt_scene_set_skin: a bone index is not below num_bones", c.set_skin, infl, n - 1)
        for bad in (np.nan, np.inf):
            refused("rt_scene_set_skin: a weight is not finite", c.set_skin, bad_table(lambda f: f["weight"].__setitem__((3, 1, 2), bad)), n)
        assert c.tree_report() == report                          # nothing kept
        refused("rt_scene_skin: no skin", c.skin_scene, mats)
        c.set_skin(infl, n)
        kept = c.tree_report()
        # an earlier skin stays in place through a refused replacement
        refused("rt_scene_set_skin: a bone index is not below num_bones", c.set_skin, infl, n - 1)
        assert c.tree_report() == kept
        null_refused(c.lib.rt_scene_skin(c.handle, None, n), "rt_scene_skin: NULL argument")
        refused("rt_scene_skin: the bone count differs", c.skin_scene, mats[:-1])
        nan = mats.copy()
        nan[1, 0, 0] = np.nan
        refused("rt_scene_skin: a matrix entry is not finite", c.skin_scene, nan)
        big = np.stack([scale(3e38, 3e38, 3e38)] * n)
        big[:, :, 3] = 3e38
        assert not np.isfinite(positions(np_skin(sc["triangles"], infl, big))).all()
        refused("rt_scene_skin: a triangle has a non-finite position", c.skin_scene, big)
        assert "refit 1" not in c.tree_report()
        c.skin_scene(mats)                                        # ... and the skin is still set
        skinned = shoot(fr)
        assert skinned["radiance"].tobytes() != before["radiance"].tobytes()
        c.upload_scene(sc)                                        # a new upload drops it
        fr.reset()
        refused("rt_scene_skin: no skin", c.skin_scene, mats)
        assert "skinned triangles" not in c.tree_report()
        c.set_skin(infl, n)
        c.skin_scene(mats)
        same_shot(shoot(fr), skinned, "set again after the upload")
    finally:
        c.close()


def test_a_skin_and_posed_objects_are_independent(golden_scenes, golden_radiance):
    sc, infl, n, bend = skin_case("cornell", golden_scenes, None)
    ids, n_objects = cornell_objects(sc["triangles"])
    M = np.stack([IDENTITY, translation(0.05, 0.02, -0.03), rotation((0, 1, 0), 0.02)])
    cam = camera("cornell", golden_radiance)
    a, b, p = context(), context(), context()
    try:
        for c in (a, b, p):
            c.upload_scene(sc)
        fa, fb, fp = frame(a, cam), frame(b, cam), frame(p, cam)
        a.set_objects(ids, n_objects)
        a.set_skin(infl, n)
        assert "posed objects: " in a.tree_report() and "skinned triangles: " in a.tree_report()
        a.pose_scene(M)
        posed = shoot(fa)
        a.skin_scene(bend)
        b.set_skin(infl, n)
        b.skin_scene(bend)
        want = shoot(fb)
        same_shot(shoot(fa), want, "pose then skin = the skin alone")
        assert posed["radiance"].tobytes() != want["radiance"].tobytes()
        a.pose_scene(M)                                           # ... and back: the objects' rest pose is the upload's, not the skinned scene
        p.set_objects(ids, n_objects)
        p.pose_scene(M)
        same_shot(shoot(fa), shoot(fp), "skin then pose = the pose alone")
        same_shot(shoot(fa), posed, "the pose as before")
        assert "posed objects: " in a.tree_report() and "skinned triangles: " in a.tree_report()
    finally:
        a.close(); b.close(); p.close()


# ---- the temporal filter's history follows a skinned surface

def test_the_history_follows_a_skinned_surface(golden_scenes, golden_radiance):
    sc = golden_scenes["cornell"]
    tris = sc["triangles"]
    box = moving_triangles(tris)                                  # bone 1 = the short box, all of its weight
    bones = np.zeros((len(tris), 3, 4), np.int64)
    bones[box, :, 0] = 1
    weights = np.zeros((len(tris), 3, 4), f32)
    weights[..., 0] = 1.0
    infl = T.influences(bones, weights)
    n = 4
    cams = moving_cameras(golden_radiance["cornell_64_b4_s2/camera"], n, (0.0, 0.0, 0.0))
    step = np.array(STEP, f32) * f32(2.0)
    mats = [np.stack([IDENTITY, translation(*(f32(k) * step))]) for k in range(n)]
    a, b = context(motion=True), context(motion=True)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        a.set_skin(infl, 2)
        ra = sequence(a, sc, lambda k: a.skin_scene(mats[k]), cams)
        rb = sequence(b, sc, lambda k: b.refit_scene(capi.debug_skin(None, tris, infl, mats[k])), cams)
    finally:
        a.close(); b.close()
    for k, (x, y) in enumerate(zip(ra, rb)):
        for key in ("ppos", "pn", "out"):
            assert np.array_equal(bits(x[key]), bits(y[key])), (k, key)
        for i in (0, 1):
            assert np.array_equal(bits(x["after"][i]), bits(y["after"][i])), (k, "history", i)
    assert ra[-1]["ppos"][..., 3].any()                            # the kept pose was there to follow
    assert (ra[-1]["after"][1][..., 2] > 1).any()                  # ... and a history longer than one frame survived the moves


# ---- queries after a skin

def test_queries_after_a_skin_equal_those_after_the_refit(golden_scenes, city):
    for name in ("cornell", "city"):
        sc, infl, n, bend = skin_case(name, golden_scenes, city)
        rng = np.random.default_rng(31)
        P = positions(sc["triangles"]).reshape(-1, 3)
        lo, hi = P.min(0), P.max(0)
        pts = np.concatenate([rng.uniform(lo, hi, (500, 3)), np.full((500, 1), np.inf)], 1).astype(f32)
        o = rng.uniform(lo, hi, (500, 3))
        d = rng.normal(size=(500, 3))
        rays = np.concatenate([o, np.zeros((500, 1)), d, np.full((500, 1), 1e30)], 1).astype(f32)
        a, b = context(), context()
        try:
            a.upload_scene(sc); b.upload_scene(sc)
            a.set_skin(infl, n)
            a.skin_scene(bend)
            b.refit_scene(capi.debug_skin(None, sc["triangles"], infl, bend))
            na, sa = a.nearest(pts, surfaces=True)
            nb, sb = b.nearest(pts, surfaces=True)
            assert na.tobytes() == nb.tobytes() and sa.tobytes() == sb.tobytes(), name
            ha, ta = a.trace(rays, surfaces=True)
            hb, tb = b.trace(rays, surfaces=True)
            hit = ha["primitive_id"] != 0xFFFFFFFF                # (of a miss only the primitive_id is specified)
            assert np.array_equal(ha["primitive_id"], hb["primitive_id"]) and ha[hit].tobytes() == hb[hit].tobytes() and ta.tobytes() == tb.tobytes(), name
            assert hit.any() and (na["primitive_id"] != 0xFFFFFFFF).all()
            assert a.trace(rays, any_hit=True).tobytes() == b.trace(rays, any_hit=True).tobytes()
        finally:
            a.close(); b.close()
