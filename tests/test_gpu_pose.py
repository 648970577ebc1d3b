"""-m gpu: rt_scene_set_objects / rt_scene_pose (raytracing_amd/csrc/pose.hip) on the device.

The contract: after rt_scene_pose(M) the context is what rt_scene_refit of rt_debug_pose(NULL, rest, ids, M)'s output would have left.  So the kernel alone is
compared with the host restatement bit for bit (which tests/test_pose.py compares with numpy), and context A (upload, set_objects, pose) with context B (upload,
refit of the restatement's triangles): radiance, counters, guides, the filters' outputs and histories, bit for bit.  One process, each GPU step once, nothing
retried; nothing here provokes a fault."""
import os
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_refit import positions
from tests.test_pose import IDENTITY, translation, rotation, scale, random_case, same_bytes, np_pose
from tests.test_motion_filter import moving_triangles, STEP
from tests.test_gpu_temporal_filter import bits, moving_cameras
from tests.test_gpu_motion_filter import classes, DESC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H, SPP, BOUNCES = 64, 64, 2, 4
OPT_WIDE_BVH = 1


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def context(refittable=True, motion=False, wide=True):
    c = capi.Context(0)
    if not wide:
        assert c.lib.rt_ctx_set_option(c.handle, OPT_WIDE_BVH, 0) == 0
    if refittable:
        c.set_refittable(True)
    if motion:
        c.set_refit_motion(True)
    return c


# ---- 5. the kernel against the host restatement

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1000])
def test_kernel_equals_host_restatement_bit_for_bit(ctx, n):
    rng = np.random.default_rng(100 + n)
    for n_objects in sorted({1, 2, 7, n}):
        tris, ids, mats = random_case(rng, n, n_objects)
        if n_objects == n:
            ids = rng.permutation(n).astype(np.uint32)        # one object per triangle, shuffled: neighbouring lanes read different matrices
        same_bytes(capi.debug_pose(ctx, tris, ids, mats), capi.debug_pose(None, tris, ids, mats))
    tris, ids, _ = random_case(rng, n, 2)
    same_bytes(capi.debug_pose(ctx, tris, ids, np.stack([IDENTITY] * 2)), tris)


# ---- 6. in a scene

@pytest.fixture(scope="module")
def city():
    scene = host.Scene(arrays=S.city_block(40_000))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}


def cornell_objects(tris):
    """object 1 = the short box, object 2 = every other triangle with an odd index, object 0 = the rest"""
    ids = np.where(np.arange(len(tris)) % 2 == 1, 2, 0).astype(np.uint32)
    ids[moving_triangles(tris)] = 1
    return ids, 3


def city_objects(tris, cells=7):
    """spatial clusters: a cells x cells grid over the two widest axes of the triangles' centroids"""
    c = positions(tris).mean(1)
    ax = np.argsort(np.ptp(c, axis=0))[-2:]
    lo, size = c[:, ax].min(0), np.ptp(c[:, ax], axis=0)
    cell = np.minimum(((c[:, ax] - lo) / size * cells).astype(np.int64), cells - 1)
    return (cell[:, 0] * cells + cell[:, 1]).astype(np.uint32), cells * cells


def scene_case(name, golden_scenes, city):
    rng = np.random.default_rng(5)
    if name == "cornell":
        sc = golden_scenes["cornell"]
        ids, n = cornell_objects(sc["triangles"])
        mats = np.stack([IDENTITY, translation(0.05, 0.02, -0.03), rotation((0, 1, 0), 0.02)])
    else:
        sc = city
        ids, n = city_objects(sc["triangles"])
        c = positions(sc["triangles"]).mean(1)
        size = float(np.ptp(c, axis=0).max())
        mats = []
        for k in range(n):
            pivot = c[ids == k].mean(0) if (ids == k).any() else np.zeros(3)
            m = rotation(rng.normal(size=3), rng.uniform(-0.2, 0.2), pivot)
            m[:, 3] += (rng.normal(size=3) * 0.004 * size).astype(f32)
            mats.append(IDENTITY if k % 5 == 0 else m)
        mats = np.stack(mats).astype(f32)
    return sc, ids, n, mats


def camera(name, golden_radiance):
    return golden_radiance["cornell_64_b4_s2/camera"] if name == "cornell" else T.default_camera(W, H)


def frame(c, cam):
    fr = capi.Frame(c, W, H)
    fr.set_camera(cam)
    fr.set_max_bounces(BOUNCES)
    return fr


def shoot(fr):
    """everything test 6 compares: radiance, resolved image, ray counters, guides, the spatial filter's output"""
    fr.reset()
    fr.integrate(SPP)
    st = fr.stats()
    alb, nrm, dep, _ = fr.guides()
    return dict(radiance=fr.radiance().copy(), image=fr.resolve().copy(), rays=np.array([st.closest_rays, st.shadow_rays]), albedo=alb, normal=nrm, depth=dep,
                filtered=fr.filter())


def same_shot(a, b, what=""):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("wide", [True, False], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_a_pose_equals_the_refit_of_the_restatement(name, wide, golden_scenes, golden_radiance, city):
    sc, ids, n, mats = scene_case(name, golden_scenes, city)
    cam = camera(name, golden_radiance)
    a, b = context(wide=wide), context(wide=wide)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        first = shoot(fa)
        a.set_objects(ids, n)
        assert "posed objects: %d objects, 324 bytes per triangle" % n in a.tree_report(), a.tree_report()
        a.pose_scene(mats)
        assert "refit 1:" in a.tree_report() and "posed objects: " in a.tree_report(), a.tree_report()
        b.refit_scene(capi.debug_pose(None, sc["triangles"], ids, mats))
        got = shoot(fa)
        same_shot(got, shoot(fb), name)
        assert got["radiance"].tobytes() != first["radiance"].tobytes()       # the pose does move what the camera sees
    finally:
        a.close(); b.close()


# ---- 7. poses are absolute

def test_poses_are_absolute(golden_scenes, golden_radiance):
    sc, ids, n, m2 = scene_case("cornell", golden_scenes, None)
    m1 = np.stack([rotation((1, 0, 0), 0.01), translation(-0.1, 0.0, 0.05), IDENTITY])
    ident = np.stack([IDENTITY] * n)
    cam = camera("cornell", golden_radiance)
    a, b = context(), context()
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        uploaded = shoot(fa)
        a.set_objects(ids, n); b.set_objects(ids, n)
        a.pose_scene(m1)
        after_m1 = shoot(fa)
        a.pose_scene(m2)
        b.pose_scene(m2)
        want = shoot(fb)
        same_shot(shoot(fa), want, "M1 then M2 = M2")
        assert after_m1["radiance"].tobytes() != want["radiance"].tobytes()
        # a refit from a buffer in between does not become the rest pose
        buf = a.create_buffer(capi.debug_pose(None, sc["triangles"], ids, m1))
        a.refit_scene(buf)
        same_shot(shoot(fa), after_m1, "the refit itself")
        a.pose_scene(m2)
        same_shot(shoot(fa), want, "M2 after a refit in between")
        buf.close()
        a.pose_scene(ident)
        same_shot(shoot(fa), uploaded, "the identity gives the upload's image")
    finally:
        a.close(); b.close()


# ---- 8. refusals leave the scene untouched

def test_refusals_leave_the_scene_untouched(golden_scenes, golden_radiance):
    sc, ids, n, mats = scene_case("cornell", golden_scenes, None)
    cam = camera("cornell", golden_radiance)
    plain = context(refittable=False)
    try:
        plain.upload_scene(sc)
        fr = frame(plain, cam)
        before = shoot(fr)
        with pytest.raises(capi.RtError, match="RT_CTX_OPT_REFITTABLE was off"):
            plain.set_objects(ids, n)
        with pytest.raises(capi.RtError, match="RT_CTX_OPT_REFITTABLE was off"):
            plain.pose_scene(mats)
        same_shot(shoot(fr), before, "not refittable")
    finally:
        plain.close()
    c = context()
    try:
        with pytest.raises(capi.RtError, match="no scene"):
            c.set_objects(ids, n)
        c.upload_scene(sc)
        fr = frame(c, cam)
        before = shoot(fr)
        report = c.tree_report()

        def refused(message, call, *args):
            with pytest.raises(capi.RtError, match=message):
                call(*args)
            same_shot(shoot(fr), before, message)

        refused("no objects", c.pose_scene, mats)
        refused("triangle count differs", c.set_objects, ids[:-1], n)
        refused("no objects", c.set_objects, ids, 0)
        refused("not below num_objects", c.set_objects, ids, n - 1)
        assert c.tree_report() == report                          # nothing kept
        refused("no objects", c.pose_scene, mats)
        c.set_objects(ids, n)
        refused("object count differs", c.pose_scene, mats[:-1])
        nan = mats.copy()
        nan[1, 0, 0] = np.nan
        refused("not finite", c.pose_scene, nan)
        big = np.stack([scale(3e38, 3e38, 3e38)] * n)
        big[:, :, 3] = 3e38
        assert not np.isfinite(positions(np_pose(sc["triangles"], ids, big))).all()
        refused("rt_scene_pose: a triangle has a non-finite position", c.pose_scene, big)
        assert "refit 1" not in c.tree_report()
        c.pose_scene(mats)                                        # ... and the objects are still set
        posed = shoot(fr)
        assert posed["radiance"].tobytes() != before["radiance"].tobytes()
        c.upload_scene(sc)                                        # a new upload drops them
        fr.reset()
        refused("no objects", c.pose_scene, mats)
        assert "posed objects" not in c.tree_report()
        c.set_objects(ids, n)
        c.pose_scene(mats)
        same_shot(shoot(fr), posed, "set again after the upload")
    finally:
        c.close()


# ---- 9. the temporal filter's history follows a posed object

def sequence(c, scene, move, cams):
    """upload, then per frame: move(k), one sample, the motion images, the temporal filter, its history (tests/test_gpu_motion_filter.py: run_sequence)"""
    fr = capi.Frame(c, W, H)
    fr.set_max_bounces(BOUNCES)
    rec = []
    for k, cam in enumerate(cams):
        move(k)
        fr.set_camera(cam)
        fr.reset()
        fr.integrate(1)
        alb, nrm, dep, _ = fr.guides()
        ppos, pn = fr.guide_motion()
        out = fr.filter_temporal(DESC)
        rec.append(dict(cam=cam, hdr=fr.radiance() / f32(fr.sample_count()), nrm=nrm, dep=dep, ppos=ppos, pn=pn, out=out, after=fr.filter_history()))
    fr.close()
    return rec


def test_the_history_follows_a_posed_object(golden_scenes, golden_radiance):
    sc = golden_scenes["cornell"]
    tris = sc["triangles"]
    ids = moving_triangles(tris).astype(np.uint32)                # object 1 = the short box
    n = 4
    cams = moving_cameras(golden_radiance["cornell_64_b4_s2/camera"], n, (0.0, 0.0, 0.0))
    step = np.array(STEP, f32) * f32(2.0)                         # STEP is a pixel at 128 x 128
    mats = [np.stack([IDENTITY, translation(*(f32(k) * step))]) for k in range(n)]
    a, b = context(motion=True), context(motion=True)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        a.set_objects(ids, 2)
        ra = sequence(a, sc, lambda k: a.pose_scene(mats[k]), cams)
        rb = sequence(b, sc, lambda k: b.refit_scene(capi.debug_pose(None, tris, ids, mats[k])), cams)
    finally:
        a.close(); b.close()
    for k, (x, y) in enumerate(zip(ra, rb)):
        for key in ("ppos", "pn", "out"):
            assert np.array_equal(bits(x[key]), bits(y[key])), (k, key)
        for i in (0, 1):
            assert np.array_equal(bits(x["after"][i]), bits(y["after"][i])), (k, "history", i)
    moving = classes(ra, tuple(step))[-1][1]
    L = ra[-1]["after"][1][..., 2]
    assert moving.sum() > 0 and (L[moving] > 1).any(), (int(moving.sum()), L[moving].max() if moving.any() else None)
