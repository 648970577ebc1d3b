"""-m gpu: separation queries (rt_scene_separation / rt_scene_separation_buffer / rt_scene_separation_self / rt_debug_separation /
rt_debug_separation_self, raytracing_amd/csrc/separation.hip) on the device.

The contract: per probe the nearest scene triangle within max_distance, the two closest points and their distance -- a statement about the triangles alone,
so the device's answer is compared byte for byte with brute force on the host (rt_debug_separation(NULL, ...), which tests/test_separation.py compares with
numpy and with exact arithmetic), whichever tree is walked, whichever fold is in place, after a refit or a pose.  One process, each GPU step once, nothing
retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_gpu_pose import scene_case
from tests.test_gpu_nearest import context
from tests.test_nearest import city, INVALID                                   # noqa: F401 (fixtures)
from tests.test_separation import scases, same, check_probes, corpus_probes, corpus_radius, np_none, INF, SEARCHED, FOUND, CROSSING      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 130]
OTHER = capi.SEPARATION_OTHER_OBJECTS


# ---- 1. k_separation_brute: the rule on the device

def test_brute_kernel_equals_host_byte_for_byte(scases):
    case = scases["coverage"]
    tris = case.scene["triangles"]
    c = context()
    try:
        for r in case.radii():
            same(capi.debug_separation(c, tris, case.probes, r), case.want(r), r)
        same(capi.debug_separation(c, tris, case.probes[:1]), capi.debug_separation(None, tris, case.probes[:1]), "n = 1")
    finally:
        c.close()


# ---- 2. the walk on the device equals brute force, whichever tree

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_separation_equals_brute_force(scases, name, wide):
    case = scases[name]
    check_probes(case)
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for r in case.radii():
            want = case.want(r)
            same(c.separation(case.probes, r), want, (name, wide, r, "all"))
            for n in COUNTS:                                               # the chunk edges: the first n probes (the not-searched ones included)
                same(c.separation(case.probes[:n], r), want[:n], (name, wide, r, n))
        c.finish()
    finally:
        c.close()


def test_corpus_trees_and_the_stack_status(env_map):
    """every BUILT tree of the corpus through rt_scene_upload, on the 4-wide records where the tree folds and with RT_CTX_OPT_WIDE_BVH = 0; a quarter of the
    probes span the whole scene: rt_finish would report a stack that ran over its bound."""
    from tests.test_gpu_tree_edges import finished
    for name in _trees.names("built"):
        c0 = _trees.case(name)
        sc = finished(c0.tris.copy(), _trees.MATS, env_map)
        probes = corpus_probes(sc["triangles"], 130)
        wants = {r: capi.debug_separation(None, sc["triangles"], probes, r) for r in (INF, corpus_radius(sc["triangles"]))}
        for wide in (1, 0):
            c = context(wide=wide)
            try:
                c.upload_scene(sc)
                for r, want in wants.items():
                    same(c.separation(probes, r), want, (name, wide, r))
                c.finish()                                                 # raises if the stack status word was set
            finally:
                c.close()


def test_adapted_fold_answers_the_same(scases):
    case = scases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the queries below walk
        for r in (INF, case.tight):
            same(c.separation(case.probes, r), case.want(r), ("adapted", r))
        fr.close()
    finally:
        c.close()


# ---- 3. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_separation_follows_pose_and_refit(scases, name, golden_scenes, city):
    case = scases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    probes = case.probes
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    want = capi.debug_separation(None, posed, probes)
    assert want.tobytes() != case.want(INF).tobytes()                     # (the pose did move something)
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        same(a.separation(probes), case.want(INF), "before the pose")
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        same(a.separation(probes), want, "pose")
    finally:
        a.close()
    b = context(refittable=True)
    try:
        b.upload_scene(sc)
        b.refit_scene(posed)
        same(b.separation(probes), want, "refit")
    finally:
        b.close()


# ---- 4. the buffer form, the self forms, refusals

def test_buffer_and_self_forms(scases, golden_scenes, city):
    case = scases["coverage"]
    sc, ids, n_objects, _ = scene_case("cornell", golden_scenes, city)
    c, other = context(refittable=True), context()                        # (set_objects needs a refittable upload)
    try:
        c.upload_scene(case.scene)
        n = len(case.probes)
        b_pr, b_out = c.create_buffer(case.probes), c.create_buffer(np.zeros(n, T.separation))
        for r in case.radii():
            c.separation_buffer(b_pr, n, r, 0, b_out)
            same(b_out.read(T.separation, n), case.want(r), ("buffers", r))
        # the self form on the scene's own triangles, host arrays and buffers, a range that starts inside a chunk
        tris = case.scene["triangles"]
        nt = len(tris)
        for first, m in ((0, nt), (5, min(nt - 5, 131))):
            for r in (INF, case.tight):
                want = capi.debug_separation_self(None, tris, first, m, r)
                same(c.separation_self(first, m, r), want, ("self", first, m, r))
                same(capi.debug_separation_self(c, tris, first, m, r), want, ("self brute", first, m, r))
        s_out = c.create_buffer(np.zeros(nt, T.separation))
        c.separation_self_buffer(0, nt, INF, 0, s_out)
        same(s_out.read(T.separation, nt), capi.debug_separation_self(None, tris, 0, nt), "self buffers")
        # refusals of the buffer forms leave the context usable
        lib, h = c.lib, c.handle
        small, alien = c.create_buffer(np.zeros(n - 1, T.separation)), other.create_buffer(np.zeros(n, T.separation))
        B = lambda b: b.handle if b is not None else None

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())
            same(c.separation(case.probes[:65]), case.want(INF)[:65], "after a refusal")

        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n, INF, 0, B(small)), "the out buffer is smaller than n")
        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n, INF, 0, B(alien)), "another context")
        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n + 1, INF, 0, B(b_out)), "the probes buffer is smaller than n")
        refused(lib.rt_scene_separation_buffer(h, None, n, INF, 0, B(b_out)), "probes is NULL")
        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n, INF, 0, None), "out is NULL")
        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n, INF, 4, B(b_out)), "unknown option bits")
        refused(lib.rt_scene_separation_buffer(h, B(b_pr), n, INF, OTHER, B(b_out)), "self forms")
        refused(lib.rt_scene_separation_self_buffer(h, 0, nt, INF, OTHER, B(s_out)), "rt_scene_set_objects")
        refused(lib.rt_scene_separation_self_buffer(h, 1, nt, INF, 0, B(s_out)), "beyond the scene")
        assert lib.rt_scene_separation_buffer(h, None, 0, INF, 0, None) == 0 and lib.rt_scene_separation_self(h, 0, 0, INF, 0, None) == 0
        for b in (b_pr, b_out, s_out, small, alien):
            b.close()
        # RT_SEPARATION_OTHER_OBJECTS on a scene with objects
        c.upload_scene(sc)
        c.set_objects(ids, n_objects)
        nt = len(sc["triangles"])
        want = capi.debug_separation_self(None, sc["triangles"], 0, nt, INF, OTHER, ids)
        assert (want["flags"] & FOUND != 0).any()
        same(c.separation_self(0, nt, INF, OTHER), want, "other objects")
        same(capi.debug_separation_self(c, sc["triangles"], 0, nt, INF, OTHER, ids), want, "other objects, brute")
        same(c.separation_self(0, nt), capi.debug_separation_self(None, sc["triangles"], 0, nt), "all pairs")
        c.finish()
    finally:
        c.close(); other.close()


def test_refusals_launch_nothing_and_leave_queries_working(scases):
    case = scases["cornell"]
    pr, n = np.ascontiguousarray(case.probes[:65]), 65
    want = case.want(INF)[:n]
    lib = capi.load()
    c = context()
    try:
        out = np.zeros(n, T.separation)
        p = lambda a: a.ctypes.data
        h = c.handle

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(h).decode(), (rc, lib.rt_last_error(h).decode())

        refused(lib.rt_scene_separation(h, p(pr), n, INF, 0, p(out)), "no scene")
        refused(lib.rt_scene_separation_self(h, 0, 1, INF, 0, p(out)), "no scene")
        c.upload_scene(case.scene)
        for rc, text in ((lambda: lib.rt_scene_separation(h, None, n, INF, 0, p(out)), "probes is NULL"),
                         (lambda: lib.rt_scene_separation(h, p(pr), n, INF, 0, None), "out is NULL"),
                         (lambda: lib.rt_scene_separation(h, p(pr), n, INF, 8, p(out)), "unknown option bits"),
                         (lambda: lib.rt_scene_separation(h, p(pr), n, INF, OTHER, p(out)), "self forms"),
                         (lambda: lib.rt_scene_separation_self(h, 0, 1, INF, OTHER, p(out)), "rt_scene_set_objects"),
                         (lambda: lib.rt_scene_separation_self(h, len(case.scene["triangles"]), 1, INF, 0, p(out)), "beyond the scene"),
                         (lambda: lib.rt_scene_separation_self(h, 0xFFFFFFFF, 2, INF, 0, p(out)), "beyond the scene")):
            refused(rc(), text)
            same(c.separation(pr), want, "after a refusal")
        assert out.tobytes() == bytes(out.nbytes)                                                     # nothing was written
        assert lib.rt_scene_separation(h, None, 0, INF, 0, None) == 0                                 # n == 0: RT_OK, nothing done
        # a max_distance that searches nothing is an answer, not a refusal
        for bad in (-1.0, float("nan")):
            assert c.separation(pr, bad).tobytes() == np_none(n).tobytes()
    finally:
        c.close()


@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(scases, ahead):
    case = scases["cornell"]
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(4)
            fr.set_option(capi.OPT_SAMPLES_AHEAD, ahead)
            fr.integrate(1)
            if disturb:
                c.separation(case.probes)
                c.separation(case.probes, case.tight)
                c.separation_self(0, len(case.scene["triangles"]))
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()
