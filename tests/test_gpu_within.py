"""-m gpu: within queries (rt_scene_within / rt_scene_within_buffer / rt_debug_within, raytracing_amd/csrc/within.hip) on the device.

The contract: per point every triangle with d2 <= max_distance^2, counted, the first max_near of them in ascending (d2, primitive_id) order -- a statement about
the triangles alone, so the device's answer is compared byte for byte with brute force on the host (rt_debug_within(NULL, ...), which tests/test_within.py
compares with numpy), whichever tree is walked, whichever fold is in place, after a refit or a pose, in counting and in k-nearest mode.  One process, each GPU
step once, nothing retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_refit import positions
from tests.test_gpu_pose import scene_case
from tests.test_gpu_nearest import context
from tests.test_nearest import city, points_of, CLASSES, NOT_SEARCHED, INVALID                 # noqa: F401 (fixtures)
from tests.test_within import wcases, within_header_case, triangles_of, same, check_classes, MAX_NEARS, SEARCHED, K_NEAREST      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = [1, 63, 64, 65, 130]
MODES = [(m, k) for m in MAX_NEARS for k in (False, True) if m or not k]


# ---- 1. k_within_brute: the rule on the device

def test_brute_kernel_equals_host_byte_for_byte():
    P, pts = within_header_case()[:2]
    tris = triangles_of(P)
    c = context()
    try:
        for max_near, knn in MODES:
            same(capi.debug_within(c, tris, pts, max_near, knn), capi.debug_within(None, tris, pts, max_near, knn), (max_near, knn))
        one = capi.debug_within(c, tris, pts[:1], 8)
        same(one, capi.debug_within(None, tris, pts[:1], 8), "n = 1")
    finally:
        c.close()


# ---- 2. the walk on the device equals brute force, whichever tree

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_within_equals_brute_force(wcases, name, wide):
    case = wcases[name]
    check_classes(case.want(0, False)[0])
    cls = np.arange(len(case.pts)) % CLASSES
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for max_near, knn in MODES:
            want = case.want(max_near, knn)
            got = c.within(case.pts, max_near, knn)
            same(got if max_near else (got, want[1]), want, (name, wide, max_near, knn, "all"))
            for n in COUNTS:                                               # the chunk edges: the first n points (every class, the not-searched ones included)
                got = c.within(case.pts[:n], max_near, knn)
                same(got if max_near else (got, want[1][:n]), (want[0][:n], want[1][:n]), (name, wide, max_near, knn, n))
        assert not case.want(8, False)[0]["flags"][cls == NOT_SEARCHED].any()
    finally:
        c.close()


def test_corpus_trees_and_the_stack_status(env_map):
    """every BUILT tree of the corpus (the ones with triangles: one triangle, two triangles, the extreme, SAH, refit and shadow soups, the grids) through
    rt_scene_upload, on the 4-wide records where the tree folds and with RT_CTX_OPT_WIDE_BVH = 0; half the points with radius +inf, where a counting walk
    leaves the most entries pending: rt_finish would report a stack that ran over its bound.  (The synthesised trees have no triangles to upload; their
    walks are tests/test_within.py's, on the host.)"""
    from tests.test_gpu_tree_edges import finished
    for name in _trees.names("built"):
        c0 = _trees.case(name)
        sc = finished(c0.tris.copy(), _trees.MATS, env_map)
        P = positions(sc["triangles"]).astype(np.float64).reshape(-1, 3)
        lo, hi = P.min(0), P.max(0)
        rng = np.random.default_rng(len(P))
        pos = (lo + rng.uniform(-0.1, 1.1, (130, 3)) * (hi - lo)).astype(f32)
        pts = points_of(pos, np.inf)
        pts["max_distance"][1::2] = f32(np.linalg.norm(hi - lo) * 0.2)
        for wide in (1, 0):
            c = context(wide=wide)
            try:
                c.upload_scene(sc)
                for max_near, knn in ((0, False), (8, False), (8, True)):
                    got = c.within(pts, max_near, knn)
                    want = capi.debug_within(None, sc["triangles"], pts, max_near, knn)
                    same(got if max_near else (got, want[1]), want, (name, wide, max_near, knn))
                c.finish()                                                 # raises if the stack status word was set
            finally:
                c.close()


def test_adapted_fold_answers_the_same(wcases):
    case = wcases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the queries below walk
        for max_near, knn in ((0, False), (8, False), (3, True)):
            want = case.want(max_near, knn)
            got = c.within(case.pts, max_near, knn)
            same(got if max_near else (got, want[1]), want, ("adapted", max_near, knn))
        fr.close()
    finally:
        c.close()


# ---- 3. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_within_follows_pose_and_refit(wcases, name, golden_scenes, city):
    case = wcases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    pts = case.pts
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    wants = {m: capi.debug_within(None, posed, pts, *m) for m in ((8, False), (3, True))}
    assert not np.array_equal(wants[(8, False)][0]["count"], case.want(8, False)[0]["count"])        # (the pose did move what the points are near to)
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        same(a.within(pts, 8), case.want(8, False), "before the pose")
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        for m, want in wants.items():
            same(a.within(pts, *m), want, ("pose", m))
        out, near, surf = a.within(pts, 8, surfaces=True)
        listed = near["primitive_id"] != INVALID
        assert np.array_equal(surf["object"][listed], ids[near["primitive_id"][listed]])
    finally:
        a.close()
    b = context(refittable=True)
    try:
        b.upload_scene(sc)
        b.refit_scene(posed)
        for m, want in wants.items():
            same(b.within(pts, *m), want, ("refit", m))
    finally:
        b.close()


# ---- 4. the buffer form, surfaces, and a bake at the members

def test_buffer_form_and_surfaces(wcases):
    case = wcases["coverage"]
    tris = case.scene["triangles"]
    pts, n, k = case.pts, len(case.pts), 3
    want = case.want(k, False)
    c = context()
    try:
        c.upload_scene(case.scene)
        out, near, surf = c.within(pts, k, surfaces=True)
        same((out, near), want, "host arrays")
        b_pts, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.point_hits))
        b_near, b_surf = c.create_buffer(np.zeros(n * k, T.nearest)), c.create_buffer(np.zeros(n * k, T.surface))
        c.within_buffer(b_pts, n, k, b_out, near=b_near, surfaces=b_surf)
        same((b_out.read(T.point_hits, n), b_near.read(T.nearest, n * k).reshape(n, k)), want, "buffers")
        assert b_surf.read(T.surface, n * k).tobytes() == surf.tobytes()
        b_only, b_out2 = c.create_buffer(np.zeros(n * k, T.surface)), c.create_buffer(np.zeros(n, T.point_hits))
        c.within_buffer(b_pts, n, k, b_out2, surfaces=b_only)                # surfaces alone: the records pass through the surface records themselves
        assert b_only.read(T.surface, n * k).tobytes() == surf.tobytes() and b_out2.read(T.point_hits, n).tobytes() == want[0].tobytes()
        b_k = c.create_buffer(np.zeros(n * k, T.nearest))
        c.within_buffer(b_pts, n, k, b_out2, near=b_k, k_nearest=True)
        same((b_out2.read(T.point_hits, n), b_k.read(T.nearest, n * k).reshape(n, k)), case.want(k, True), "buffers, k nearest")
        c.within_buffer(b_pts, n, k, b_out2)                                 # nowhere to list: the counting walk answers
        assert b_out2.read(T.point_hits, n).tobytes() == want[0].tobytes()
        # member 0's surface is k_nearest_surface's
        assert surf[:, 0].tobytes() == c.nearest(pts, surfaces=True)[1].tobytes()
        # every member's surface is query_surface's host restatement fed with its record: direction = q - p, t = distance
        rays, hits = np.zeros((n, k), T.ray), np.zeros((n, k), T.hit)
        d = (near["position"] - pts["position"][:, None, :]).astype(f32)
        for a, ax in enumerate("xyz"):
            rays["direction"][ax] = d[:, :, a]
        hits["bc"]["x"], hits["bc"]["y"] = near["bc"][:, :, 0], near["bc"][:, :, 1]
        hits["primitive_id"], hits["t"] = near["primitive_id"], near["distance"]
        host_surf = capi.debug_query_surface(None, tris, rays.reshape(-1), hits.reshape(-1)).reshape(n, k)
        assert surf.tobytes() == host_surf.tobytes(), [f for f in T.surface.names if surf[f].tobytes() != host_surf[f].tobytes()]
        listed = near["primitive_id"] != INVALID
        assert listed[:, 1:].any() and (~listed).any() and not surf[~listed]["flags"].any() and (surf["primitive_id"][~listed] == INVALID).all()
        # ... and they feed a bake without a trip to the host
        b_bake = c.create_buffer(np.zeros(n * k, T.bake_result))
        c.bake_buffer(b_surf, n * k, b_bake, 16, seed=1, bias=1e-3, radius=0.5, from_surfaces=True)
        baked = b_bake.read(T.bake_result, n * k).reshape(n, k)
        assert (baked["unoccluded"][~listed] == INVALID).all() and (baked["unoccluded"][listed] <= 16).any()
        assert "ray queries: " in c.tree_report()
        for b in (b_pts, b_out, b_near, b_surf, b_only, b_out2, b_k, b_bake):
            b.close()
    finally:
        c.close()


# ---- 5. no frame state; refusals that need a device

@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(wcases, ahead):
    case = wcases["cornell"]
    pts = case.pts[:257]
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(4)
            fr.set_option(capi.OPT_SAMPLES_AHEAD, ahead)
            fr.integrate(1)
            if disturb:
                c.within(pts, 8, surfaces=True)
                c.within(pts, 0)
                c.within(pts, 4, True)
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()


def test_refusals_launch_nothing_and_leave_queries_working(wcases):
    case = wcases["cornell"]
    pts, n, k = case.pts[:65], 65, 8
    want = (case.want(k, False)[0][:n], case.want(k, False)[1][:n])
    lib = capi.load()
    c, other = context(), context()
    try:
        out, near, surf = np.zeros(n, T.point_hits), np.zeros((n, k), T.nearest), np.zeros((n, k), T.surface)
        p = lambda a: a.ctypes.data

        def refused(rc, text, handle=None):
            assert rc != 0 and text in lib.rt_last_error(handle).decode(), (rc, lib.rt_last_error(handle).decode())

        refused(lib.rt_scene_within(c.handle, p(pts), n, k, 0, p(out), p(near), None), "no scene", c.handle)
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)

        def still_works():
            same(c.within(pts, k), want, "after a refusal")

        h = c.handle
        refused(lib.rt_scene_within(h, None, n, k, 0, p(out), p(near), None), "points is NULL", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, k, 0, None, p(near), None), "out is NULL", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, k + 1, 0, p(out), p(near), None), "RT_WITHIN_MAX", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, 0, 0, p(out), p(near), None), "max_near == 0", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, 0, 0, p(out), None, p(surf)), "max_near == 0", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, 0, 1, p(out), None, None), "max_near >= 1", h); still_works()
        refused(lib.rt_scene_within(h, p(pts), n, k, 6, p(out), p(near), None), "unknown option bits", h); still_works()
        assert out.tobytes() == bytes(out.nbytes) and near.tobytes() == bytes(near.nbytes) and surf.tobytes() == bytes(surf.nbytes)     # nothing was written
        assert lib.rt_scene_within(h, None, 0, 0, 0, None, None, None) == 0                      # n == 0: RT_OK, nothing done
        b_pts, b_out, b_small = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.point_hits)), c.create_buffer(np.zeros(n * k - 1, T.nearest))
        b_alien, b_surf = other.create_buffer(np.zeros(n * k, T.nearest)), c.create_buffer(np.zeros(n * k, T.surface))
        b_out_small = c.create_buffer(np.zeros(n - 1, T.point_hits))
        B = lambda b: b.handle
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, k, 0, B(b_out), B(b_small), None), "the near buffer is smaller than n", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, k, 0, B(b_out_small), None, None), "the out buffer is smaller than n", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n + 1, k, 0, B(b_out), None, None), "the points buffer is smaller than n", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, k, 0, B(b_out), B(b_alien), None), "another context", h); still_works()
        refused(lib.rt_scene_within_buffer(h, None, n, k, 0, B(b_out), None, None), "points is NULL", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, k, 0, None, None, B(b_surf)), "out is NULL", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, 0, 0, B(b_out), None, B(b_surf)), "max_near == 0", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, 0, 1, B(b_out), None, None), "max_near >= 1", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, 9, 0, B(b_out), None, None), "RT_WITHIN_MAX", h); still_works()
        refused(lib.rt_scene_within_buffer(h, B(b_pts), n, k, 2, B(b_out), None, None), "unknown option bits", h); still_works()
        assert b_out.read(T.point_hits, n).tobytes() == bytes(16 * n) and b_surf.read(T.surface, n * k).tobytes() == bytes(64 * n * k)
        assert b_small.read(T.nearest, n * k - 1).tobytes() == bytes(32 * (n * k - 1))
        assert lib.rt_scene_within_buffer(h, None, 0, 0, 0, None, None, None) == 0
        for b in (b_pts, b_out, b_small, b_alien, b_surf, b_out_small):
            b.close()
    finally:
        c.close(); other.close()


# ---- 6. layers

def test_layers_name_the_object_and_equal_capi():
    import os
    import subprocess
    from raytracing_amd import host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = host.Scene(os.path.join(root, "assets", "CornellBox.obj"), objects=True)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    render = host.Render(32, 24, scene)
    render.set_camera(host.default_camera(32, 24)); render.set_max_bounces(4)
    names, owner = scene.object_names(), scene.triangle_objects()
    tris = render.scene_arrays()["triangles"]
    flat = positions(tris).reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    rng = np.random.default_rng(19)
    pts = points_of((lo + rng.uniform(0.1, 0.9, (40, 3)) * (hi - lo)).astype(f32), f32(np.linalg.norm(hi - lo) * 0.25))
    pts["max_distance"][::5] = f32(1e-6)                                    # some have no member
    for k, knn in ((8, False), (3, True), (0, False)):
        want = capi.debug_within(None, tris, pts, k, knn)
        got = render.within(pts, k=k, k_nearest=knn)                       # Render::Within through rth_render_within
        assert [g["count"] for g in got] == list(want[0]["count"]) and [g["nearest_primitive"] for g in got] == list(want[0]["nearest_primitive"])
        for g, o, row in zip(got, want[0], want[1]):
            assert len(g["members"]) == o["stored"]
            for m, w in zip(g["members"], row):
                assert m["nearest"].tobytes() == w.tobytes() and m["object_name"] == names[owner[w["primitive_id"]]]
    want = capi.debug_within(None, tris, pts, 8)
    assert (want[0]["count"] > 8).any() and (want[0]["count"] == 0).any()
    assert len({names[owner[t]] for t in want[1]["primitive_id"][want[1]["primitive_id"] != INVALID]}) > 1        # more than one object was told apart
    # radius as an argument, rows of three columns
    got = render.within(pts["position"][1:3], radius=float(pts["max_distance"][1]), k=8)
    assert [g["count"] for g in got] == list(want[0]["count"][1:3])
    # objects_within names the objects of the nearest 8 members and says how many members there are
    i = int(np.argmax(want[0]["count"]))
    assert want[0]["count"][i] > 8
    got = render.objects_within(pts["position"][i], float(pts["max_distance"][i]))
    assert got == {"objects": sorted({names[owner[t]] for t in want[1]["primitive_id"][i]}), "count": int(want[0]["count"][i]), "complete": False}
    assert render.objects_within(pts["position"][0], 1e-6) == {"objects": [], "count": 0, "complete": True}
    c = capi.Context(0)
    try:
        c.upload_scene(render.scene_arrays())
        same(c.within(pts, 8), want, "capi")
    finally:
        c.close()
    j = int(np.flatnonzero(want[0]["count"] == 0)[0])
    r = subprocess.run([os.path.join(root, "raytracing_amd", "rt_render"), "-w", "32", "-h", "24", "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--within", "%.9g,%.9g,%.9g,%.9g" % (tuple(pts["position"][i]) + (pts["max_distance"][i],)),
                        "--within", "%.9g,%.9g,%.9g,%.9g,2" % (tuple(pts["position"][i]) + (pts["max_distance"][i],)),
                        "--within", "%.9g,%.9g,%.9g,1e-6" % tuple(pts["position"][j])], cwd=root, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("within ")]
    assert r.returncode == 0 and len(lines) == 3 + 8 + 2, (r.returncode, r.stdout[-600:], r.stderr[-400:])
    assert ("count %d " % want[0]["count"][i]) in lines[0] and ("nearest primitive %d" % want[0]["nearest_primitive"][i]) in lines[0]
    for m in range(8):
        assert ("primitive %d " % want[1]["primitive_id"][i, m]) in lines[1 + m] and lines[1 + m].rstrip().replace(" (back side)", "").endswith(
            names[owner[want[1]["primitive_id"][i, m]]]), lines[1 + m]
    assert "count 2 " in lines[9] and ("primitive %d " % want[1]["primitive_id"][i, 1]) in lines[11]
    assert lines[12].rstrip().endswith(": none"), lines[12]
