"""-m gpu: rt_scene_set_morph / rt_scene_morph / rt_scene_morph_skin (raytracing_amd/csrc/morph.hip) on the device.

The contract: after rt_scene_morph(w) the context is what rt_scene_refit of rt_debug_morph(NULL, rest, targets, w)'s output would have left, and after
rt_scene_morph_skin(w, M) what rt_scene_refit of rt_debug_skin(NULL, rt_debug_morph(NULL, ...), influences, M) would have.  So each kernel alone is compared with
the host restatement bit for bit (which tests/test_morph.py compares with numpy) on every tail shape, both weight paths, both palette paths and the row shapes
that can go wrong, and context A (upload, set_morph, morph) with context B (upload, refit of the restatement's triangles): radiance, counters, guides, the
filters' outputs and histories, queries, bit for bit.  One process, each GPU step once, nothing retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, scenes as S, types as T
from tests.test_refit import positions
from tests.test_pose import IDENTITY, translation, rotation, same_bytes, decorated
from tests.test_skin import random_case as random_skin_case
from tests.test_morph import random_case, random_targets, np_morph
from tests.test_motion_filter import moving_triangles, random_triangles, STEP
from tests.test_gpu_temporal_filter import bits, moving_cameras
from tests.test_gpu_pose import context, camera, frame, shoot, same_shot, sequence, cornell_objects  # noqa: F401
from tests.test_gpu_skin import skin_case

pytestmark = pytest.mark.gpu
f32 = np.float32
L = capi.MORPH_LDS_TARGETS
K = capi.SKIN_LDS_BONES
TARGET_COUNTS = (1, 2, L, L + 1, 4096)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def host_morph_skin(tris, deltas, offsets, w, infl, mats):
    return capi.debug_skin(None, capi.debug_morph(None, tris, deltas, offsets, w), infl, mats)


def both_kernels(ctx, tris, deltas, offsets, w, seed):
    """k_morph_triangles against the restatement, then k_morph_skin_triangles on the same shape against the composition, with a palette staged in LDS and one
    gathered from memory; returns the morph"""
    got = capi.debug_morph(ctx, tris, deltas, offsets, w)
    same_bytes(got, capi.debug_morph(None, tris, deltas, offsets, w))
    for n_bones in (K, K + 1):
        _, infl, mats = random_skin_case(np.random.default_rng(seed + n_bones), len(tris), n_bones)
        same_bytes(capi.debug_morph_skin(ctx, tris, deltas, offsets, w, infl, mats), host_morph_skin(tris, deltas, offsets, w, infl, mats))
    return got


# ---- the kernels against the host restatement: every tail shape, both weight paths, both palette paths

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1000])
def test_kernels_equal_the_host_restatement_bit_for_bit(ctx, n):
    rng = np.random.default_rng(400 + n)
    for n_targets in TARGET_COUNTS:
        per_target = min(3 * n, 6) if n_targets > 2 else 3 * n // 2 + 1             # many small targets, or few that touch half of everything
        tris, deltas, offsets, w = random_case(rng, n, n_targets, share=per_target / (3 * n))
        w[-1] = 1.5                                                                # the last target counts (the last weight is read)
        got = both_kernels(ctx, tris, deltas, offsets, w, 1000 * n + n_targets)
        assert (positions(got) != positions(tris)).any()
    same_bytes(capi.debug_morph(ctx, tris, deltas, offsets, np.zeros(len(w), f32)), tris)


# ---- row shapes

def test_no_deltas_at_all(ctx):
    tris = decorated(random_triangles(np.random.default_rng(1), 300), np.random.default_rng(2))
    empty = (np.zeros(0, np.int64), np.zeros((0, 3), f32), None)
    deltas, offsets = T.morph_targets([empty] * 3)
    same_bytes(both_kernels(ctx, tris, deltas, offsets, np.array([1, -2, 3], f32), 10), tris)


def test_one_triangle_touched_by_every_one_of_4096_targets(ctx):
    """the long, lopsided row: triangle 70's three corners in every target, its neighbours in none"""
    rng = np.random.default_rng(3)
    n, n_targets = 300, 4096
    tris = decorated(random_triangles(rng, n), rng)
    corners = np.array([3 * 70, 3 * 70 + 1, 3 * 70 + 2])
    targets = [(corners[rng.permutation(3)], rng.normal(0, 0.01, (3, 3)).astype(f32), rng.normal(0, 0.01, (3, 3)).astype(f32)) for _ in range(n_targets)]
    deltas, offsets = T.morph_targets(targets)
    w = rng.normal(0, 1, n_targets).astype(f32)
    got = both_kernels(ctx, tris, deltas, offsets, w, 20)
    moved = (positions(got) != positions(tris)).any((1, 2))
    assert moved[70] and moved.sum() == 1


def test_every_corner_in_every_target(ctx):
    rng = np.random.default_rng(4)
    n = 513
    tris = decorated(random_triangles(rng, n), rng)
    targets = [(rng.permutation(3 * n), rng.normal(0, 0.1, (3 * n, 3)).astype(f32), rng.normal(0, 0.3, (3 * n, 3)).astype(f32)) for _ in range(3)]
    deltas, offsets = T.morph_targets(targets)
    got = both_kernels(ctx, tris, deltas, offsets, np.array([0.5, -1.0, 0.25], f32), 30)
    assert (positions(got) != positions(tris)).all((1, 2)).all()


def test_the_last_triangle_of_a_tail_block_owns_the_last_record(ctx):
    rng = np.random.default_rng(5)
    n = 256 + 37
    tris = decorated(random_triangles(rng, n), rng)
    targets = random_targets(rng, n - 1, 4, share=0.1)                             # nothing on the last triangle ...
    targets.append((np.array([3 * (n - 1) + 2]), np.array([[0.5, -0.25, 1.0]], f32), np.array([[0.1, 0.2, -0.3]], f32)))     # ... but the last target's one delta
    deltas, offsets = T.morph_targets(targets)
    w = np.array([1.0, -0.5, 0.0, 2.0, 3.0], f32)
    got = both_kernels(ctx, tris, deltas, offsets, w, 40)
    assert got["v3"]["position"]["x"][n - 1] == tris["v3"]["position"]["x"][n - 1] + f32(3.0) * f32(0.5)


def test_the_two_weight_paths_agree(ctx):
    """the same first L targets, once as a set of L (weights staged in LDS) and once with one empty target appended (L + 1: gathered from memory)"""
    rng = np.random.default_rng(6)
    n = 513
    tris = decorated(random_triangles(rng, n), rng)
    targets = random_targets(rng, n, L, share=4 / (3 * n))
    w = rng.normal(0, 1, L).astype(f32)
    staged = capi.debug_morph(ctx, tris, *T.morph_targets(targets), w)
    more = targets + [(np.zeros(0, np.int64), np.zeros((0, 3), f32), None)]
    gathered = capi.debug_morph(ctx, tris, *T.morph_targets(more), np.concatenate([w, np.array([7.0], f32)]))
    same_bytes(staged, gathered)
    same_bytes(staged, capi.debug_morph(None, tris, *T.morph_targets(targets), w))


# ---- in a scene

def morph_case(golden_scenes, n_targets=6, huge=False):
    """the Cornell scene, synthetic targets over it (BVH order) and two weight vectors.  huge: one more target, of weight 0 in both vectors, that moves
    corner 0 by 1e20"""
    sc = golden_scenes["cornell"]
    targets = S.synthetic_morph(sc["triangles"], n_targets, radius=0.25, amplitude=0.04)
    w2 = np.linspace(0.3, 1.0, n_targets).astype(f32)
    w1 = np.linspace(-0.8, 0.5, n_targets).astype(f32)
    if huge:
        targets.append((np.array([0]), np.array([[1e20, 0, 0]], f32), None))
        w1, w2 = np.append(w1, f32(0)), np.append(w2, f32(0))
    deltas, offsets = T.morph_targets(targets)
    assert len(deltas) > n_targets
    return sc, deltas, offsets, w1, w2


def same_queries(a, b, tris):
    """nearest points and closest hits with their surfaces, and any-hit verdicts, of the same points and rays in two contexts, bit for bit"""
    rng = np.random.default_rng(31)
    P = positions(tris).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    pts = np.concatenate([rng.uniform(lo, hi, (300, 3)), np.full((300, 1), np.inf)], 1).astype(f32)
    rays = np.concatenate([rng.uniform(lo, hi, (300, 3)), np.zeros((300, 1)), rng.normal(size=(300, 3)), np.full((300, 1), 1e30)], 1).astype(f32)
    na, sa = a.nearest(pts, surfaces=True)
    nb, sb = b.nearest(pts, surfaces=True)
    assert na.tobytes() == nb.tobytes() and sa.tobytes() == sb.tobytes()
    ha, ta = a.trace(rays, surfaces=True)
    hb, tb = b.trace(rays, surfaces=True)
    hit = ha["primitive_id"] != 0xFFFFFFFF                        # (of a miss only the primitive_id is specified)
    assert np.array_equal(ha["primitive_id"], hb["primitive_id"]) and ha[hit].tobytes() == hb[hit].tobytes() and ta.tobytes() == tb.tobytes()
    assert hit.any() and (na["primitive_id"] != 0xFFFFFFFF).all()
    assert a.trace(rays, any_hit=True).tobytes() == b.trace(rays, any_hit=True).tobytes()


@pytest.mark.parametrize("wide", [True, False], ids=["wide_trees", "wide_trees_off"])
def test_a_morph_equals_the_refit_of_the_restatement(wide, golden_scenes, golden_radiance):
    sc, deltas, offsets, _, w = morph_case(golden_scenes)
    tris = sc["triangles"]
    cam = camera("cornell", golden_radiance)
    a, b = context(wide=wide), context(wide=wide)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        first = shoot(fa)
        a.set_morph(deltas, offsets, len(tris))
        assert "morph targets: %d targets, %d deltas, " % (len(w), len(deltas)) in a.tree_report(), a.tree_report()
        a.morph_scene(w)
        assert "refit 1:" in a.tree_report() and "morph targets: " in a.tree_report(), a.tree_report()
        b.refit_scene(capi.debug_morph(None, tris, deltas, offsets, w))
        got = shoot(fa)
        same_shot(got, shoot(fb), "morph")
        assert got["radiance"].tobytes() != first["radiance"].tobytes()       # the morph does move what the camera sees
        same_queries(a, b, tris)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("wide", [True, False], ids=["wide_trees", "wide_trees_off"])
def test_a_morph_and_skin_equals_the_refit_of_the_restatement(wide, golden_scenes, golden_radiance):
    sc, deltas, offsets, _, w = morph_case(golden_scenes)
    _, infl, n_bones, bend = skin_case("cornell", golden_scenes, None)
    tris = sc["triangles"]
    cam = camera("cornell", golden_radiance)
    a, b, s = context(wide=wide), context(wide=wide), context(wide=wide)
    try:
        for c in (a, b, s):
            c.upload_scene(sc)
        fa, fb, fs = frame(a, cam), frame(b, cam), frame(s, cam)
        a.set_morph(deltas, offsets, len(tris))
        a.set_skin(infl, n_bones)
        assert "morph targets: " in a.tree_report() and "skinned triangles: " in a.tree_report()
        a.morph_skin_scene(w, bend)
        b.refit_scene(host_morph_skin(tris, deltas, offsets, w, infl, bend))
        got = shoot(fa)
        same_shot(got, shoot(fb), "morph and skin")
        same_queries(a, b, tris)
        s.set_skin(infl, n_bones)
        s.skin_scene(bend)
        assert got["radiance"].tobytes() != shoot(fs)["radiance"].tobytes()   # ... and is not the skin alone
        # the fused call works from the MORPH's rest pose: a skin set after a morph moved the scene has another rest pose, which is not read
        a.morph_scene(w)
        a.set_skin(infl, n_bones)
        a.morph_skin_scene(w, bend)
        same_shot(shoot(fa), got, "the skin's own rest pose is not read")
    finally:
        a.close(); b.close(); s.close()


def test_morphs_are_absolute(golden_scenes, golden_radiance):
    sc, deltas, offsets, w1, w2 = morph_case(golden_scenes)
    tris = sc["triangles"]
    cam = camera("cornell", golden_radiance)
    a, b = context(), context()
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        fa, fb = frame(a, cam), frame(b, cam)
        uploaded = shoot(fa)
        a.set_morph(deltas, offsets, len(tris)); b.set_morph(deltas, offsets, len(tris))
        a.morph_scene(w1)
        after_w1 = shoot(fa)
        a.morph_scene(w2)
        b.morph_scene(w2)
        want = shoot(fb)
        same_shot(shoot(fa), want, "w1 then w2 = w2")
        assert after_w1["radiance"].tobytes() != want["radiance"].tobytes()
        a.refit_scene(capi.debug_morph(None, tris, deltas, offsets, w1))          # a refit in between does not become the rest pose
        same_shot(shoot(fa), after_w1, "the refit itself")
        a.morph_scene(w2)
        same_shot(shoot(fa), want, "w2 after a refit in between")
        a.morph_scene(np.zeros(len(w2), f32))
        same_shot(shoot(fa), uploaded, "zero weights give the upload's image")
    finally:
        a.close(); b.close()


def test_every_producer_keeps_the_rest_pose_its_own_set_call_saw(golden_scenes, golden_radiance):
    """the objects are set on the upload, the skin and the morph on the POSED scene: three rest poses in one context, each of them its producer's alone"""
    sc, deltas, offsets, _, w = morph_case(golden_scenes)
    _, infl, n_bones, bend = skin_case("cornell", golden_scenes, None)
    tris = sc["triangles"]
    assert len(tris) % 256 != 0                                   # the last block of every kernel here is a tail block
    ids, n_objects = cornell_objects(tris)
    M = np.stack([IDENTITY, translation(0.05, 0.02, -0.03), rotation((0, 1, 0), 0.02)])
    cam = camera("cornell", golden_radiance)
    a, p, u, d = context(), context(), context(), context()
    try:
        for c in (a, p, u, d):
            c.upload_scene(sc)
        fa, fp, fu, fd = frame(a, cam), frame(p, cam), frame(u, cam), frame(d, cam)
        uploaded = shoot(fu)
        p.set_objects(ids, n_objects)
        p.pose_scene(M)
        posed = shoot(fp)
        assert posed["radiance"].tobytes() != uploaded["radiance"].tobytes()
        a.set_objects(ids, n_objects)
        a.pose_scene(M)
        a.set_skin(infl, n_bones)                                 # their rest pose: the posed scene
        a.set_morph(deltas, offsets, len(tris))
        a.skin_scene(np.stack([IDENTITY] * n_bones))
        same_shot(shoot(fa), posed, "the identity palette gives the scene rt_scene_set_skin saw")
        a.pose_scene(np.stack([IDENTITY] * n_objects))
        same_shot(shoot(fa), uploaded, "the identity pose gives the scene rt_scene_set_objects saw")
        a.morph_scene(np.zeros(len(w), f32))
        same_shot(shoot(fa), posed, "zero weights give the scene rt_scene_set_morph saw")
        a.pose_scene(np.stack([IDENTITY] * n_objects))            # the scene is the upload again when the fused call starts from the morph's rest pose
        a.morph_skin_scene(w, bend)
        d.set_objects(ids, n_objects)
        d.pose_scene(M)
        d.set_skin(infl, n_bones)
        d.set_morph(deltas, offsets, len(tris))
        d.morph_skin_scene(w, bend)
        got = shoot(fa)
        same_shot(got, shoot(fd), "morph and skin after all that = morph and skin alone")
        assert got["radiance"].tobytes() != posed["radiance"].tobytes()
    finally:
        a.close(); p.close(); u.close(); d.close()


def test_refusals_leave_the_scene_and_an_earlier_morph_untouched(golden_scenes, golden_radiance):
    sc, deltas, offsets, w1, w = morph_case(golden_scenes, huge=True)
    _, infl, n_bones, bend = skin_case("cornell", golden_scenes, None)
    tris = sc["triangles"]
    n, k = len(tris), len(w)
    cam = camera("cornell", golden_radiance)
    plain = context(refittable=False)
    try:
        plain.upload_scene(sc)
        fr = frame(plain, cam)
        before = shoot(fr)
        with pytest.raises(capi.RtError, match="rt_scene_set_morph: RT_CTX_OPT_REFITTABLE was off"):
            plain.set_morph(deltas, offsets, n)
        with pytest.raises(capi.RtError, match="rt_scene_morph: RT_CTX_OPT_REFITTABLE was off"):
            plain.morph_scene(w)
        with pytest.raises(capi.RtError, match="rt_scene_morph_skin: RT_CTX_OPT_REFITTABLE was off"):
            plain.morph_skin_scene(w, bend)
        same_shot(shoot(fr), before, "not refittable")
    finally:
        plain.close()
    c = context()
    try:
        with pytest.raises(capi.RtError, match="rt_scene_set_morph: no scene"):
            c.set_morph(deltas, offsets, n)
        with pytest.raises(capi.RtError, match="rt_scene_morph: no scene"):
            c.morph_scene(w)
        with pytest.raises(capi.RtError, match="rt_scene_morph_skin: no scene"):
            c.morph_skin_scene(w, bend)
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

        def bad(field, at, value):
            d = deltas.copy()
            d[field][at] = value
            return d

        o = offsets.astype(np.int64)
        refused("rt_scene_morph: no morph", c.morph_scene, w)
        refused("rt_scene_morph_skin: no morph", c.morph_skin_scene, w, bend)
        null_refused(c.lib.rt_scene_set_morph(c.handle, None, offsets.ctypes.data, k, n), "rt_scene_set_morph: NULL argument")
        null_refused(c.lib.rt_scene_set_morph(c.handle, deltas.ctypes.data, None, k, n), "rt_scene_set_morph: NULL argument")
        refused("rt_scene_set_morph: the triangle count differs", c.set_morph, deltas, offsets, n - 1)
        null_refused(c.lib.rt_scene_set_morph(c.handle, deltas.ctypes.data, offsets.ctypes.data, 0, n), "rt_scene_set_morph: no targets")
        null_refused(c.lib.rt_scene_set_morph(c.handle, deltas.ctypes.data, offsets.ctypes.data, 65537, n), "rt_scene_set_morph: more than 65536 targets")
        refused(r"rt_scene_set_morph: target_offsets\[0\] is not 0", c.set_morph, deltas, np.concatenate([[1], o[1:]]), n)
        refused("rt_scene_set_morph: target_offsets decrease", c.set_morph, deltas, np.concatenate([o[:1], o[2:3], o[1:2], o[3:]]), n)
        refused("rt_scene_set_morph: a corner is not below", c.set_morph, bad("corner", 1, 3 * n), offsets, n)
        for value in (np.nan, np.inf):
            refused("rt_scene_set_morph: a delta is not finite", c.set_morph, bad("normal", (2, 1), value), offsets, n)
        refused("rt_scene_set_morph: a delta's pad is not 0", c.set_morph, bad("pad", 0, 1), offsets, n)
        refused("rt_scene_set_morph: a target moves the same corner twice", c.set_morph, bad("corner", 1, deltas["corner"][0]), offsets, n)
        assert c.tree_report() == report                          # nothing kept
        refused("rt_scene_morph: no morph", c.morph_scene, w)
        c.set_morph(deltas, offsets, n)
        kept = c.tree_report()
        # an earlier morph stays in place through a refused replacement
        refused("rt_scene_set_morph: a delta's pad is not 0", c.set_morph, bad("pad", 0, 1), offsets, n)
        assert c.tree_report() == kept
        null_refused(c.lib.rt_scene_morph(c.handle, None, k), "rt_scene_morph: NULL argument")
        refused("rt_scene_morph: the target count differs", c.morph_scene, w[:-1])
        for value in (np.nan, np.inf):
            nan = w.copy()
            nan[1] = value
            refused("rt_scene_morph: a weight is not finite", c.morph_scene, nan)
        refused("rt_scene_morph_skin: no skin", c.morph_skin_scene, w, bend)
        c.set_skin(infl, n_bones)
        kept = c.tree_report()
        refused("rt_scene_morph_skin: the bone count differs", c.morph_skin_scene, w, bend[:-1])
        refused("rt_scene_morph_skin: the target count differs", c.morph_skin_scene, w[:-1], bend)
        nan = bend.copy()
        nan[1, 0, 0] = np.nan
        refused("rt_scene_morph_skin: a matrix entry is not finite", c.morph_skin_scene, w, nan)
        for value in (np.nan, np.inf):
            nan = w.copy()
            nan[1] = value
            refused("rt_scene_morph_skin: a weight is not finite", c.morph_skin_scene, nan, bend)
        null_refused(c.lib.rt_scene_morph_skin(c.handle, None, k, bend.ctypes.data, n_bones), "rt_scene_morph_skin: NULL argument")
        null_refused(c.lib.rt_scene_morph_skin(c.handle, w.ctypes.data, k, None, n_bones), "rt_scene_morph_skin: NULL argument")
        # an overflowing morph: huge weight x delta -> inf, refused by the refit's validation with the scene untouched
        big = w.copy()
        big[-1] = 1e30                                            # 1e30 * 1e20
        assert not np.isfinite(positions(np_morph(tris, deltas, offsets, big))).all()
        refused("rt_scene_morph: a triangle has a non-finite position", c.morph_scene, big)
        refused("rt_scene_morph_skin: a triangle has a non-finite position", c.morph_skin_scene, big, bend)
        assert "refit 1" not in c.tree_report() and c.tree_report() == kept
        c.morph_scene(w)                                          # ... and the morph is still set
        morphed = shoot(fr)
        assert morphed["radiance"].tobytes() != before["radiance"].tobytes()
        c.upload_scene(sc)                                        # a new upload drops it
        fr.reset()
        refused("rt_scene_morph: no morph", c.morph_scene, w)
        assert "morph targets" not in c.tree_report()
        c.set_morph(deltas, offsets, n)
        c.morph_scene(w)
        same_shot(shoot(fr), morphed, "set again after the upload")
    finally:
        c.close()


# ---- the temporal filter's history follows a morphed surface

def test_the_motion_guide_follows_a_morphed_surface(golden_scenes, golden_radiance):
    sc = golden_scenes["cornell"]
    tris = sc["triangles"]
    box = np.flatnonzero(moving_triangles(tris))                   # one target: the short box, every corner by the same step
    corners = (3 * box[:, None] + np.arange(3)).reshape(-1)
    step = np.array(STEP, f32) * f32(2.0)
    deltas, offsets = T.morph_targets([(corners, np.tile(step, (len(corners), 1)), None)])
    n = 4
    cams = moving_cameras(golden_radiance["cornell_64_b4_s2/camera"], n, (0.0, 0.0, 0.0))
    a, b = context(motion=True), context(motion=True)
    try:
        a.upload_scene(sc); b.upload_scene(sc)
        a.set_morph(deltas, offsets, len(tris))
        ra = sequence(a, sc, lambda k: a.morph_scene(np.array([k], f32)), cams)
        rb = sequence(b, sc, lambda k: b.refit_scene(capi.debug_morph(None, tris, deltas, offsets, np.array([k], f32))), cams)
    finally:
        a.close(); b.close()
    for k, (x, y) in enumerate(zip(ra, rb)):
        for key in ("ppos", "pn", "out"):
            assert np.array_equal(bits(x[key]), bits(y[key])), (k, key)
        for i in (0, 1):
            assert np.array_equal(bits(x["after"][i]), bits(y["after"][i])), (k, "history", i)
    assert ra[-1]["ppos"][..., 3].any()                            # the kept pose was there to follow
