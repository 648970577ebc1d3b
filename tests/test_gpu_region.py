"""-m gpu: overlap queries (rt_scene_overlap / rt_scene_overlap_buffer / rt_scene_select / rt_frame_pick_rect / rt_debug_overlap / rt_debug_select,
raytracing_amd/csrc/region.hip) on the device.

The contract: per region the triangles no plane rejects, counted, those wholly inside counted, the lowest ids listed -- a statement about the triangles alone,
so the device's answer is compared byte for byte with brute force on the host (rt_debug_overlap(NULL, ...), which tests/test_region.py compares with numpy),
whichever tree is walked, whichever fold is in place, after a refit or a pose.  One process, each GPU step once, nothing retried; nothing here provokes a
fault."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_refit import positions
from tests.test_gpu_pose import scene_case
from tests.test_gpu_nearest import context
from tests.test_nearest import city, INVALID                                   # noqa: F401 (fixtures)
from tests.test_region import rcases, same, check_classes, corpus_regions, make_regions, MAX_LISTS, SEARCHED, CLASSES, NOT_SEARCHED      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = [1, 63, 64, 65, 130]


def overlap(c, regions, max_list, want_members):
    """Context.overlap as (records, members): max_list == 0 returns the records alone"""
    got = c.overlap(regions, max_list)
    return got if max_list else (got, want_members)


# ---- 1. k_region_brute and k_select: the rule on the device

def test_brute_and_select_kernels_equal_host_byte_for_byte(rcases):
    case = rcases["coverage"]
    tris = case.scene["triangles"]
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 7, len(tris)).astype(np.uint32)                    # object 7 has no triangle
    c = context()
    try:
        for max_list in MAX_LISTS:
            same(capi.debug_overlap(c, tris, case.regions, max_list), case.want(max_list), max_list)
        same(capi.debug_overlap(c, tris, case.regions[:1], 8), capi.debug_overlap(None, tris, case.regions[:1], 8), "n = 1")
        for n in (1, 31, 32):
            got, want = capi.debug_select(c, tris, case.regions[:n], ids, 8), capi.debug_select(None, tris, case.regions[:n], ids, 8)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), n
            got, want = capi.debug_select(c, tris, case.regions[:n]), capi.debug_select(None, tris, case.regions[:n])
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), n
        sorted_ids = np.sort(ids)                                             # whole waves of one object: the wave-wide OR's path
        got, want = capi.debug_select(c, tris, case.regions[:32], sorted_ids, 8), capi.debug_select(None, tris, case.regions[:32], sorted_ids, 8)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and want[2].any() and want[3].any()
    finally:
        c.close()


# ---- 2. the walk on the device equals brute force, whichever tree

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_overlap_equals_brute_force(rcases, name, wide):
    case = rcases[name]
    check_classes(case.want(0)[0], len(case.scene["triangles"]))
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for max_list in MAX_LISTS:
            want = case.want(max_list)
            same(overlap(c, case.regions, max_list, want[1]), want, (name, wide, max_list, "all"))
            for n in COUNTS:                                               # the chunk edges: the first n regions (every class, the not-searched ones included)
                same(overlap(c, case.regions[:n], max_list, want[1][:n]), (want[0][:n], want[1][:n]), (name, wide, max_list, n))
        c.finish()
    finally:
        c.close()


def test_corpus_trees_and_the_stack_status(env_map):
    """every BUILT tree of the corpus through rt_scene_upload, on the 4-wide records where the tree folds and with RT_CTX_OPT_WIDE_BVH = 0; a quarter of the
    regions (and with the half-spaces about half) enclose the whole scene, where a counting walk leaves the most entries pending: rt_finish would report a
    stack that ran over its bound."""
    from tests.test_gpu_tree_edges import finished
    for name in _trees.names("built"):
        c0 = _trees.case(name)
        sc = finished(c0.tris.copy(), _trees.MATS, env_map)
        regions = corpus_regions(sc["triangles"], 130)
        regions[1::4] = regions[0]                                          # half of them enclose everything
        wants = {m: capi.debug_overlap(None, sc["triangles"], regions, m) for m in (0, 8)}
        assert (wants[0][0]["count"][0::4] == len(sc["triangles"])).all() and (wants[0][0]["count"][1::4] == len(sc["triangles"])).all()
        for wide in (1, 0):
            c = context(wide=wide)
            try:
                c.upload_scene(sc)
                for max_list, want in wants.items():
                    same(overlap(c, regions, max_list, want[1]), want, (name, wide, max_list))
                c.finish()                                                 # raises if the stack status word was set
            finally:
                c.close()


def test_adapted_fold_answers_the_same(rcases):
    case = rcases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the queries below walk
        for max_list in (0, 8):
            want = case.want(max_list)
            same(overlap(c, case.regions, max_list, want[1]), want, ("adapted", max_list))
        fr.close()
    finally:
        c.close()


# ---- 3. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_overlap_follows_pose_and_refit(rcases, name, golden_scenes, city):
    case = rcases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    regions = case.regions
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    want = capi.debug_overlap(None, posed, regions, 8)
    assert not np.array_equal(want[0]["count"], case.want(8)[0]["count"]) or not np.array_equal(want[0]["inside"], case.want(8)[0]["inside"])   # (the pose did move something)
    sel = capi.debug_select(None, posed, regions[:32], ids, n_objects)
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        same(a.overlap(regions, 8), case.want(8), "before the pose")
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        same(a.overlap(regions, 8), want, "pose")
        got = a.select(regions[:32], objects=n_objects)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, sel)), "select after the pose"
    finally:
        a.close()
    b = context(refittable=True)
    try:
        b.upload_scene(sc)
        b.refit_scene(posed)
        same(b.overlap(regions, 8), want, "refit")
    finally:
        b.close()


# ---- 4. select and its objects, the buffer forms, a call of more than one staging chunk

def test_select_objects_and_buffer_forms(rcases, golden_scenes, city):
    case = rcases["cornell"]
    sc, ids, n_objects, _ = scene_case("cornell", golden_scenes, city)
    tris, nt = sc["triangles"], len(sc["triangles"])
    P = positions(tris).reshape(nt, 3, 3)
    # a box around one whole object, and one through its middle: the object is inside the first and straddles the second
    o = int(np.argmin([np.ptp(P[ids == k].reshape(-1, 3), axis=0).max() if (ids == k).any() else np.inf for k in range(n_objects)]))
    lo, hi = P[ids == o].reshape(-1, 3).min(0), P[ids == o].reshape(-1, 3).max(0)
    around, through = T.box_region(lo - 1e-3, hi + 1e-3), T.box_region(lo - 1e-3, (lo + hi) / 2)
    regions = np.concatenate([np.array([around, through], T.region), case.regions[:30]])
    want = capi.debug_select(None, tris, regions, ids, n_objects)
    assert want[3][o] & 1 and want[2][o] & 2 and not want[3][o] & 2           # window-selected by the first, crossing-selected only by the second
    c, other = context(refittable=True), context()
    try:
        c.upload_scene(sc)
        lib, h = c.lib, c.handle
        word = np.zeros(nt, np.uint32)
        assert lib.rt_scene_select(h, regions.ctypes.data, 32, word.ctypes.data, None, None, word.ctypes.data) != 0 and "rt_scene_set_objects" in lib.rt_last_error(h).decode()
        got = c.select(regions)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        c.set_objects(ids, n_objects)
        got = c.select(regions, objects=n_objects)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        for n in (1, 31):
            got, w = c.select(regions[:n], objects=n_objects), capi.debug_select(None, tris, regions[:n], ids, n_objects)
            assert all(g.tobytes() == x.tobytes() for g, x in zip(got, w)), n
        with pytest.raises(capi.RtError, match="RT_SELECT_MAX_REGIONS"):
            c.select(np.concatenate([regions, regions[:1]]), objects=n_objects)
        # the buffer forms
        b_rg = c.create_buffer(regions)
        b_t, b_i = c.create_buffer(np.zeros(nt, np.uint32)), c.create_buffer(np.zeros(nt, np.uint32))
        b_ot, b_oi = c.create_buffer(np.zeros(n_objects, np.uint32)), c.create_buffer(np.zeros(n_objects, np.uint32))
        c.select_buffer(b_rg, 32, b_t, b_i, b_ot, b_oi)
        got = (b_t.read(np.uint32, nt), b_i.read(np.uint32, nt), b_ot.read(np.uint32, n_objects), b_oi.read(np.uint32, n_objects))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        n, k = len(case.regions), 3
        b_all, b_out, b_mem = c.create_buffer(case.regions), c.create_buffer(np.zeros(n, T.region_hits)), c.create_buffer(np.zeros(n * k, T.region_member))
        c.overlap_buffer(b_all, n, k, b_out, b_mem)
        same((b_out.read(T.region_hits, n), b_mem.read(T.region_member, n * k).reshape(n, k)), case.want(k), "buffers")
        same(c.overlap(case.regions, k), case.want(k), "host arrays")
        b_out2 = c.create_buffer(np.zeros(n, T.region_hits))
        c.overlap_buffer(b_all, n, k, b_out2)                                # nowhere to list: the counting walk answers
        assert b_out2.read(T.region_hits, n).tobytes() == case.want(k)[0].tobytes()
        # refusals of the buffer forms leave the context usable
        small, alien = c.create_buffer(np.zeros(n * k - 1, T.region_member)), other.create_buffer(np.zeros(n * k, T.region_member))
        small_t = c.create_buffer(np.zeros(nt - 1, np.uint32))
        B = lambda b: b.handle if b is not None else None

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())
            same(c.overlap(case.regions[:65], k), (case.want(k)[0][:65], case.want(k)[1][:65]), "after a refusal")

        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n, k, B(b_out), B(small)), "the members buffer is smaller than n")
        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n, k, B(b_out), B(alien)), "another context")
        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n + 1, k, B(b_out), None), "the regions buffer is smaller than n")
        refused(lib.rt_scene_overlap_buffer(h, None, n, k, B(b_out), None), "regions is NULL")
        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n, k, None, None), "out is NULL")
        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n, 9, B(b_out), None), "RT_REGION_LIST_MAX")
        refused(lib.rt_scene_overlap_buffer(h, B(b_all), n, 0, B(b_out), B(b_mem)), "max_list == 0")
        refused(lib.rt_scene_select_buffer(h, B(b_rg), 32, B(small_t), None, None, None), "the touching buffer is smaller than n")
        refused(lib.rt_scene_select_buffer(h, B(b_rg), 33, B(b_t), None, None, None), "RT_SELECT_MAX_REGIONS")
        refused(lib.rt_scene_select_buffer(h, B(b_rg), 32, None, None, None, None), "no output")
        assert lib.rt_scene_overlap_buffer(h, None, 0, 0, None, None) == 0
        for b in (b_rg, b_t, b_i, b_ot, b_oi, b_all, b_out, b_mem, b_out2, small, alien, small_t):
            b.close()
    finally:
        c.close(); other.close()


def test_a_call_of_more_than_one_staging_chunk_equals_its_chunks(rcases):
    """the host form stages at most 4 Mi member records at a time: with max_list 8 a chunk holds 512 Ki regions"""
    case = rcases["cornell"]
    chunk = (4 << 20) // 8
    reps = -(-(chunk + 1000) // len(case.regions))
    regions = np.tile(case.regions, reps)[:chunk + 1000]
    c = context()
    try:
        c.upload_scene(case.scene)
        out, members = c.overlap(regions, 8)
        a, b = c.overlap(regions[:chunk], 8), c.overlap(regions[chunk:], 8)
        assert out.tobytes() == a[0].tobytes() + b[0].tobytes() and members.tobytes() == a[1].tobytes() + b[1].tobytes()
        want = case.want(8)
        idx = np.arange(len(regions)) % len(case.regions)
        assert out.tobytes() == want[0][idx].tobytes() and members.tobytes() == want[1][idx].tobytes()
    finally:
        c.close()


def test_refusals_launch_nothing_and_leave_queries_working(rcases):
    case = rcases["cornell"]
    rg, n, k = np.ascontiguousarray(case.regions[:65]), 65, 8
    want = (case.want(k)[0][:n], case.want(k)[1][:n])
    lib = capi.load()
    c = context()
    try:
        out, members = np.zeros(n, T.region_hits), np.zeros((n, k), T.region_member)
        p = lambda a: a.ctypes.data
        h = c.handle

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())

        refused(lib.rt_scene_overlap(h, p(rg), n, k, p(out), p(members)), "no scene")
        refused(lib.rt_scene_select(h, p(rg), 1, p(out), None, None, None), "no scene")
        c.upload_scene(case.scene)
        for rc, text in ((lambda: lib.rt_scene_overlap(h, None, n, k, p(out), p(members)), "regions is NULL"),
                         (lambda: lib.rt_scene_overlap(h, p(rg), n, k, None, p(members)), "out is NULL"),
                         (lambda: lib.rt_scene_overlap(h, p(rg), n, k + 1, p(out), p(members)), "RT_REGION_LIST_MAX"),
                         (lambda: lib.rt_scene_overlap(h, p(rg), n, 0, p(out), p(members)), "max_list == 0"),
                         (lambda: lib.rt_scene_select(h, p(rg), 0, p(out), None, None, None), "RT_SELECT_MAX_REGIONS"),
                         (lambda: lib.rt_scene_select(h, p(rg), 33, p(out), None, None, None), "RT_SELECT_MAX_REGIONS"),
                         (lambda: lib.rt_scene_select(h, None, 1, p(out), None, None, None), "regions is NULL"),
                         (lambda: lib.rt_scene_select(h, p(rg), 1, None, None, None, None), "no output")):
            refused(rc(), text)
            same(c.overlap(rg, k), want, "after a refusal")
        assert out.tobytes() == bytes(out.nbytes) and members.tobytes() == bytes(members.nbytes)      # nothing was written
        assert lib.rt_scene_overlap(h, p(rg), n, k, p(out), None) == 0                               # the host form with nowhere to list: the counting walk answers
        assert out.tobytes() == want[0].tobytes() and members.tobytes() == bytes(members.nbytes)
        assert lib.rt_scene_overlap(h, None, 0, 0, None, None) == 0                                  # n == 0: RT_OK, nothing done
    finally:
        c.close()


# ---- 5. the marquee

def test_pick_rect_marks_what_the_pixels_pick(golden_scenes, golden_radiance):
    sc = golden_scenes["cornell"]
    cam = golden_radiance["cornell_64_b4_s2/camera"]
    c = context()
    try:
        c.upload_scene(sc)
        fr = capi.Frame(c, 32, 32)
        fr.set_camera(cam)
        picked = np.full((32, 32), INVALID, np.uint32)
        for y in range(32):
            for x in range(32):
                picked[y, x] = fr.pick(x, y)[1]["primitive_id"]
        assert (picked != INVALID).sum() > 200
        g, touching, inside = fr.pick_rect(8, 8, 23, 23)
        cam32 = np.array(cam, T.camera).copy()
        assert g.tobytes() == capi.debug_rect_region(cam32, 32, 32, 8, 8, 23, 23).tobytes()
        mid = np.unique(picked[8:24, 8:24]); mid = mid[mid != INVALID]
        assert len(mid) >= 2 and (touching[mid] & 1).all() and not (inside & ~touching).any()
        g_all, t_all, _ = fr.pick_rect(0, 0, 31, 31)
        every = np.unique(picked); every = every[every != INVALID]
        assert (t_all[every] & 1).all() and (t_all & 1).sum() >= (touching & 1).sum() and not (touching & ~t_all).any()
        tw, iw = capi.debug_select(None, sc["triangles"], [g])
        assert tw.tobytes() == touching.tobytes() and iw.tobytes() == inside.tobytes()
        near = fr.pick_rect(8, 8, 23, 23, t_near=0.5, t_far=100.0)[0]
        assert near["num_planes"] == 6
        lib, h = c.lib, c.handle
        for args, text in (((9, 8, 8, 23), "x1 < x0"), ((8, 9, 23, 8), "y1 < y0"), ((8, 8, 32, 23), "outside the image"), ((8, 8, 23, 32), "outside the image")):
            assert lib.rt_frame_pick_rect(fr.handle, *args, 0.0, 1.0, None, touching.ctypes.data, None, None, None) != 0 and text in lib.rt_last_error(h).decode()
        assert lib.rt_frame_pick_rect(fr.handle, 8, 8, 23, 23, 0.0, 1.0, None, None, None, touching.ctypes.data, None) != 0 and "rt_scene_set_objects" in lib.rt_last_error(h).decode()
        assert fr.pick_rect(8, 8, 23, 23)[1].tobytes() == touching.tobytes()          # still usable
        fr.close()
        tile = capi.Frame(c, 32, 32, tile_rank=0, tile_count=2)
        assert lib.rt_frame_pick_rect(tile.handle, 0, 0, 1, 1, 0.0, 1.0, None, touching.ctypes.data, None, None, None) != 0 and "tile frame" in lib.rt_last_error(h).decode()
        tile.close()
    finally:
        c.close()


@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(rcases, ahead):
    case = rcases["cornell"]
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(4)
            fr.set_option(capi.OPT_SAMPLES_AHEAD, ahead)
            fr.integrate(1)
            if disturb:
                c.overlap(case.regions, 8)
                c.overlap(case.regions, 0)
                c.select(case.regions[:32])
                fr.pick_rect(3, 4, 40, 50)
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()
