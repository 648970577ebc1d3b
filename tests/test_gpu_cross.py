"""-m gpu: crossing queries (rt_scene_cross / rt_scene_cross_buffer / rt_scene_cross_self / rt_debug_cross / rt_debug_cross_self,
raytracing_amd/csrc/cross.hip) on the device.

The contract: per probe the scene triangles it crosses, counted, the lowest ids listed with their contact points -- a statement about the triangles alone, so
the device's answer is compared byte for byte with brute force on the host (rt_debug_cross(NULL, ...), which tests/test_cross.py compares with numpy and with
exact integer arithmetic), whichever tree is walked, whichever fold is in place, after a refit or a pose.  One process, each GPU step once, nothing retried;
nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_gpu_pose import scene_case
from tests.test_gpu_nearest import context
from tests.test_nearest import city, INVALID                                   # noqa: F401 (fixtures)
from tests.test_cross import ccases, same, cross, check_probes, corpus_probes, MAX_LISTS, SEARCHED, ANY_MODE      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 130]
ANY = capi.CROSS_ANY


# ---- 1. k_cross_brute: the rule on the device

def test_brute_kernel_equals_host_byte_for_byte(ccases):
    case = ccases["coverage"]
    tris = case.scene["triangles"]
    c = context()
    try:
        for max_list in MAX_LISTS:
            same(cross(capi.debug_cross, c, tris, case.probes, max_list=max_list), case.want(max_list), max_list)
            same(cross(capi.debug_cross, c, tris, case.probes[:1], max_list=max_list), cross(capi.debug_cross, None, tris, case.probes[:1], max_list=max_list), ("n = 1", max_list))
        same(cross(capi.debug_cross, c, tris, case.probes, max_list=0, options=ANY), case.want(0, ANY), "any")
    finally:
        c.close()


# ---- 2. the walk on the device equals brute force, whichever tree

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_cross_equals_brute_force(ccases, name, wide):
    case = ccases[name]
    check_probes(case.want(0)[0], len(case.scene["triangles"]))
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for max_list, options in [(m, 0) for m in MAX_LISTS] + [(0, ANY)]:
            want = case.want(max_list, options)
            same(cross(c.cross, case.probes, max_list=max_list, options=options), want, (name, wide, max_list, options, "all"))
            for n in COUNTS:                                               # the chunk edges: the first n probes (the not-searched ones included)
                same(cross(c.cross, case.probes[:n], max_list=max_list, options=options), (want[0][:n], want[1][:n]), (name, wide, max_list, options, n))
        c.finish()
    finally:
        c.close()


def test_corpus_trees_and_the_stack_status(env_map):
    """every BUILT tree of the corpus through rt_scene_upload, on the 4-wide records where the tree folds and with RT_CTX_OPT_WIDE_BVH = 0; a quarter of the
    probes span the whole scene, where a counting walk leaves the most entries pending: rt_finish would report a stack that ran over its bound."""
    from tests.test_gpu_tree_edges import finished
    for name in _trees.names("built"):
        c0 = _trees.case(name)
        sc = finished(c0.tris.copy(), _trees.MATS, env_map)
        probes = corpus_probes(sc["triangles"], 130)
        wants = {m: cross(capi.debug_cross, None, sc["triangles"], probes, max_list=m) for m in (0, 8)}
        for wide in (1, 0):
            c = context(wide=wide)
            try:
                c.upload_scene(sc)
                for max_list, want in wants.items():
                    same(cross(c.cross, probes, max_list=max_list), want, (name, wide, max_list))
                c.finish()                                                 # raises if the stack status word was set
            finally:
                c.close()


def test_adapted_fold_answers_the_same(ccases):
    case = ccases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the queries below walk
        for max_list in (0, 8):
            same(cross(c.cross, case.probes, max_list=max_list), case.want(max_list), ("adapted", max_list))
        fr.close()
    finally:
        c.close()


# ---- 3. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_cross_follows_pose_and_refit(ccases, name, golden_scenes, city):
    case = ccases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    probes = case.probes
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    want = capi.debug_cross(None, posed, probes, 8)
    assert want[0].tobytes() != case.want(8)[0].tobytes() or want[1].tobytes() != case.want(8)[1].tobytes()        # (the pose did move something)
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        same(a.cross(probes, 8), case.want(8), "before the pose")
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        same(a.cross(probes, 8), want, "pose")
    finally:
        a.close()
    b = context(refittable=True)
    try:
        b.upload_scene(sc)
        b.refit_scene(posed)
        same(b.cross(probes, 8), want, "refit")
    finally:
        b.close()


# ---- 4. the buffer form, the self forms, refusals

def test_buffer_and_self_forms(ccases, golden_scenes, city):
    case = ccases["coverage"]
    sc, ids, n_objects, _ = scene_case("cornell", golden_scenes, city)
    c, other = context(refittable=True), context()                        # (set_objects needs a refittable upload)
    try:
        c.upload_scene(case.scene)
        n, k = len(case.probes), 3
        b_pr, b_out, b_mem = c.create_buffer(case.probes), c.create_buffer(np.zeros(n, T.probe_hits)), c.create_buffer(np.zeros(n * k, T.cross_member))
        c.cross_buffer(b_pr, n, k, 0, b_out, b_mem)
        same((b_out.read(T.probe_hits, n), b_mem.read(T.cross_member, n * k).reshape(n, k)), case.want(k), "buffers")
        b_out2 = c.create_buffer(np.zeros(n, T.probe_hits))
        c.cross_buffer(b_pr, n, k, 0, b_out2)                                # nowhere to list: the counting walk answers
        assert b_out2.read(T.probe_hits, n).tobytes() == case.want(k)[0].tobytes()
        c.cross_buffer(b_pr, n, 0, ANY, b_out2)
        assert b_out2.read(T.probe_hits, n).tobytes() == case.want(0, ANY)[0].tobytes()
        # the self form on the scene's own triangles, host arrays and buffers, a range that starts inside a chunk
        tris = case.scene["triangles"]
        nt = len(tris)
        for first, m in ((0, nt), (5, min(nt - 5, 131))):
            want = capi.debug_cross_self(None, tris, first, m, 8)
            same(c.cross_self(first, m, 8), want, ("self", first, m))
            same(capi.debug_cross_self(c, tris, first, m, 8), want, ("self brute", first, m))
            same(cross(c.cross_self, first, m, max_list=0), cross(capi.debug_cross_self, None, tris, first, m, max_list=0), ("self count", first, m))
            same(cross(c.cross_self, first, m, max_list=0, options=ANY), cross(capi.debug_cross_self, None, tris, first, m, max_list=0, options=ANY), ("self any", first, m))
        s_out, s_mem = c.create_buffer(np.zeros(nt, T.probe_hits)), c.create_buffer(np.zeros(nt * 8, T.cross_member))
        c.cross_self_buffer(0, nt, 8, 0, s_out, s_mem)
        same((s_out.read(T.probe_hits, nt), s_mem.read(T.cross_member, nt * 8).reshape(nt, 8)), capi.debug_cross_self(None, tris, 0, nt, 8), "self buffers")
        # refusals of the buffer forms leave the context usable
        lib, h = c.lib, c.handle
        small, alien = c.create_buffer(np.zeros(n * k - 1, T.cross_member)), other.create_buffer(np.zeros(n * k, T.cross_member))
        B = lambda b: b.handle if b is not None else None

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())
            same(c.cross(case.probes[:65], k), (case.want(k)[0][:65], case.want(k)[1][:65]), "after a refusal")

        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, 0, B(b_out), B(small)), "the members buffer is smaller than n")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, 0, B(b_out), B(alien)), "another context")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n + 1, k, 0, B(b_out), None), "the probes buffer is smaller than n")
        refused(lib.rt_scene_cross_buffer(h, None, n, k, 0, B(b_out), None), "probes is NULL")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, 0, None, None), "out is NULL")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, 9, 0, B(b_out), None), "RT_CROSS_LIST_MAX")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, 0, 0, B(b_out), B(b_mem)), "max_list == 0")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, ANY, B(b_out), B(b_mem)), "RT_CROSS_ANY lists no members")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, 4, B(b_out), None), "unknown option bits")
        refused(lib.rt_scene_cross_buffer(h, B(b_pr), n, k, capi.CROSS_OTHER_OBJECTS, B(b_out), None), "self forms")
        refused(lib.rt_scene_cross_self_buffer(h, 0, nt, 8, capi.CROSS_OTHER_OBJECTS, B(s_out), B(s_mem)), "rt_scene_set_objects")
        refused(lib.rt_scene_cross_self_buffer(h, 1, nt, 8, 0, B(s_out), B(s_mem)), "beyond the scene")
        assert lib.rt_scene_cross_buffer(h, None, 0, 0, 0, None, None) == 0 and lib.rt_scene_cross_self(h, 0, 0, 0, 0, None, None) == 0
        for b in (b_pr, b_out, b_mem, b_out2, s_out, s_mem, small, alien):
            b.close()
        # RT_CROSS_OTHER_OBJECTS on a scene with objects
        c.upload_scene(sc)
        c.set_objects(ids, n_objects)
        nt = len(sc["triangles"])
        want = capi.debug_cross_self(None, sc["triangles"], 0, nt, 8, capi.CROSS_OTHER_OBJECTS, ids)
        same(c.cross_self(0, nt, 8, capi.CROSS_OTHER_OBJECTS), want, "other objects")
        same(capi.debug_cross_self(c, sc["triangles"], 0, nt, 8, capi.CROSS_OTHER_OBJECTS, ids), want, "other objects, brute")
        same(c.cross_self(0, nt, 8), capi.debug_cross_self(None, sc["triangles"], 0, nt, 8), "all pairs")
        c.finish()
    finally:
        c.close(); other.close()


def test_refusals_launch_nothing_and_leave_queries_working(ccases):
    case = ccases["cornell"]
    pr, n, k = np.ascontiguousarray(case.probes[:65]), 65, 8
    want = (case.want(k)[0][:n], case.want(k)[1][:n])
    lib = capi.load()
    c = context()
    try:
        out, members = np.zeros(n, T.probe_hits), np.zeros((n, k), T.cross_member)
        p = lambda a: a.ctypes.data
        h = c.handle

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())

        refused(lib.rt_scene_cross(h, p(pr), n, k, 0, p(out), p(members)), "no scene")
        refused(lib.rt_scene_cross_self(h, 0, 1, k, 0, p(out), p(members)), "no scene")
        c.upload_scene(case.scene)
        for rc, text in ((lambda: lib.rt_scene_cross(h, None, n, k, 0, p(out), p(members)), "probes is NULL"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, k, 0, None, p(members)), "out is NULL"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, k + 1, 0, p(out), p(members)), "RT_CROSS_LIST_MAX"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, 0, 0, p(out), p(members)), "max_list == 0"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, k, ANY, p(out), p(members)), "RT_CROSS_ANY lists no members"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, k, 8, p(out), p(members)), "unknown option bits"),
                         (lambda: lib.rt_scene_cross(h, p(pr), n, k, capi.CROSS_OTHER_OBJECTS, p(out), p(members)), "self forms"),
                         (lambda: lib.rt_scene_cross_self(h, 0, 1, k, capi.CROSS_OTHER_OBJECTS, p(out), p(members)), "rt_scene_set_objects"),
                         (lambda: lib.rt_scene_cross_self(h, len(case.scene["triangles"]), 1, k, 0, p(out), p(members)), "beyond the scene"),
                         (lambda: lib.rt_scene_cross_self(h, 0xFFFFFFFF, 2, k, 0, p(out), p(members)), "beyond the scene")):
            refused(rc(), text)
            same(c.cross(pr, k), want, "after a refusal")
        assert out.tobytes() == bytes(out.nbytes) and members.tobytes() == bytes(members.nbytes)      # nothing was written
        assert lib.rt_scene_cross(h, p(pr), n, k, 0, p(out), None) == 0                              # the host form with nowhere to list: the counting walk answers
        assert out.tobytes() == want[0].tobytes() and members.tobytes() == bytes(members.nbytes)
        assert lib.rt_scene_cross(h, None, 0, 0, 0, None, None) == 0                                 # n == 0: RT_OK, nothing done
    finally:
        c.close()


@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(ccases, ahead):
    case = ccases["cornell"]
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(4)
            fr.set_option(capi.OPT_SAMPLES_AHEAD, ahead)
            fr.integrate(1)
            if disturb:
                c.cross(case.probes, 8)
                c.cross(case.probes, 0, ANY)
                c.cross_self(0, len(case.scene["triangles"]), 8)
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()
