"""-m gpu: nearest-point queries (rt_scene_nearest / rt_scene_nearest_buffer / rt_debug_nearest, raytracing_amd/csrc/nearest.hip) on the device.

The contract: per point the smallest d2 <= max_distance^2 over all triangles, ties to the lowest index -- a statement about the triangles alone, so the device's
answer is compared byte for byte with brute force on the host (rt_debug_nearest(NULL, ...), which tests/test_nearest.py compares with numpy), whichever tree is
walked, whichever fold is in place, after a refit or a pose.  Every batch mixes points inside the bounds, on and near surfaces, far outside, 2^30 away, limits at
half and at twice the true distance, and points that are not searched.  One process, each GPU step once, nothing retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests.test_refit import positions
from tests.test_gpu_pose import scene_case
from tests.test_nearest import (city, cases, Case, header_case, triangles_of, points_of, same_records, check_batch, CLASSES, NOT_SEARCHED,       # noqa: F401 (fixtures)
                                INVALID, FOUND, BACK_SIDE, SHIFT, FACE)

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = [1, 63, 64, 65, 257, 4099]


def context(wide=1, adaptive=None, refittable=False):
    c = capi.Context(0)
    if wide != 1:
        c.set_wide_bvh(wide)
    if adaptive is not None:
        c.set_adaptive_fold(adaptive)
    if refittable:
        c.set_refittable(True)
    return c


# ---- 1. k_nearest_brute: the arithmetic on the device

def test_brute_kernel_equals_host_byte_for_byte():
    P, pts, _, _ = header_case()
    pts = pts[np.random.default_rng(3).permutation(len(pts))]              # every batch size gets a mix of the case's point kinds, not its first kind only
    tris = triangles_of(P)
    c = context()
    try:
        for n in COUNTS:
            batch = np.resize(pts, n) if n <= len(pts) else np.concatenate([pts, np.resize(pts[::-1], n - len(pts))])
            want = capi.debug_nearest(None, tris, batch)
            same_records(capi.debug_nearest(c, tris, batch), want, n)
            found = want["primitive_id"] != INVALID
            assert n < 64 or (found.any() and (~found).any())
    finally:
        c.close()


# ---- 2. the walk on the device equals brute force, whichever tree

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_nearest_equals_brute_force(cases, name, wide):
    case = cases[name]
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for n in COUNTS:
            pts, want = case.batch(n)
            check_batch(pts, want)
            same_records(c.nearest(pts), want, (name, wide, n))
    finally:
        c.close()


def test_adapted_fold_answers_the_same(cases):
    case = cases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the query below walks
        pts, want = case.batch(4099)
        same_records(c.nearest(pts), want, "adapted")
        fr.close()
    finally:
        c.close()


# ---- 3. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_nearest_follows_pose_and_refit(cases, name, golden_scenes, city):
    case = cases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    pts, unmoved = case.batch(4099)
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    want = capi.debug_nearest(None, posed, pts)
    assert not np.array_equal(want["distance"], unmoved["distance"])        # (the pose did move what the points are near to)
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        same_records(a.nearest(pts), unmoved, "before the pose")
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        got, surf = a.nearest(pts, surfaces=True)
        same_records(got, want, "pose")
        found = want["primitive_id"] != INVALID
        assert np.array_equal(surf["object"][found], ids[want["primitive_id"][found]])
    finally:
        a.close()
    b = context(refittable=True)
    try:
        b.upload_scene(sc)
        b.refit_scene(posed)
        same_records(b.nearest(pts), want, "refit")
    finally:
        b.close()


# ---- 4. the buffer form, surfaces, and a bake at the nearest points

def test_buffer_form_and_surfaces(cases):
    case = cases["coverage"]
    tris = case.scene["triangles"]
    c = context()
    try:
        c.upload_scene(case.scene)
        pts, want = case.batch(4099)
        n = len(pts)
        got, surf = c.nearest(pts, surfaces=True)
        same_records(got, want, "host arrays")
        b_pts, b_out, b_surf = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.nearest)), c.create_buffer(np.zeros(n, T.surface))
        c.nearest_buffer(b_pts, n, out=b_out, surfaces=b_surf)
        same_records(b_out.read(T.nearest, n), want, "buffers")
        assert b_surf.read(T.surface, n).tobytes() == surf.tobytes()
        b_only = c.create_buffer(np.zeros(n, T.surface))
        c.nearest_buffer(b_pts, n, surfaces=b_only)                          # surfaces alone: the records pass through the surface records themselves
        assert b_only.read(T.surface, n).tobytes() == surf.tobytes()
        # the surfaces are query_surface's host restatement fed with the nearest records: direction = q - p, t = distance
        rays, hits = np.zeros(n, T.ray), np.zeros(n, T.hit)
        d = (want["position"] - pts["position"]).astype(f32)
        for k, ax in enumerate("xyz"):
            rays["direction"][ax] = d[:, k]
        hits["bc"]["x"], hits["bc"]["y"] = want["bc"][:, 0], want["bc"][:, 1]
        hits["primitive_id"], hits["t"] = want["primitive_id"], want["distance"]
        host_surf = capi.debug_query_surface(None, tris, rays, hits)
        assert surf.tobytes() == host_surf.tobytes(), [k for k in T.surface.names if surf[k].tobytes() != host_surf[k].tobytes()]
        found = want["primitive_id"] != INVALID
        assert found.any() and (~found).any() and not surf[~found]["flags"].any() and (surf["primitive_id"][~found] == INVALID).all()
        # the back-face bit agrees with RT_NEAREST_BACK_SIDE where the direction is along the normal (the face region) and the point is off the surface
        flat = positions(tris).reshape(-1, 3)
        off = found & (((want["flags"] >> SHIFT) & 3) == FACE) & (want["distance"] > 1e-5 * np.linalg.norm(flat.max(0) - flat.min(0))) & \
            (np.abs(surf["geometric_normal"]).sum(1) > 0)
        assert off.sum() > n // 8
        assert np.array_equal((surf["flags"][off] & 2) != 0, (want["flags"][off] & BACK_SIDE) != 0)
        # ... and they feed a bake without a trip to the host
        b_bake = c.create_buffer(np.zeros(n, T.bake_result))
        c.bake_buffer(b_surf, n, b_bake, 16, seed=1, bias=1e-3, radius=0.5, from_surfaces=True)
        baked = b_bake.read(T.bake_result, n)
        assert (baked["unoccluded"][~found] == INVALID).all() and (baked["unoccluded"][found] <= 16).any()
        assert "ray queries: " in c.tree_report()
        for b in (b_pts, b_out, b_surf, b_only, b_bake):
            b.close()
    finally:
        c.close()


# ---- 5. no frame state; refusals that need a device

def test_frames_are_undisturbed(cases):
    case = cases["cornell"]
    pts = case.batch(257)[0]
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(T.default_camera(64, 64)); fr.set_max_bounces(4)
            fr.integrate(1)
            if disturb:
                c.nearest(pts, surfaces=True)
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()


def test_refusals_launch_nothing_and_leave_queries_working(cases):
    case = cases["cornell"]
    pts, want = case.batch(65)
    n = len(pts)
    lib = capi.load()
    c, other = context(), context()
    try:
        out, surf = np.zeros(n, T.nearest), np.zeros(n, T.surface)
        p = lambda a: a.ctypes.data

        def refused(rc, text, handle=None):
            assert rc != 0 and text in lib.rt_last_error(handle).decode(), (rc, lib.rt_last_error(handle).decode())

        refused(lib.rt_scene_nearest(c.handle, p(pts), n, p(out), None), "no scene", c.handle)
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)

        def still_works():
            same_records(c.nearest(pts), want, "after a refusal")

        refused(lib.rt_scene_nearest(c.handle, None, n, p(out), None), "points is NULL", c.handle); still_works()
        refused(lib.rt_scene_nearest(c.handle, p(pts), n, None, None), "no output", c.handle); still_works()
        assert out.tobytes() == bytes(out.nbytes) and surf.tobytes() == bytes(surf.nbytes)       # nothing was written by any of them
        assert lib.rt_scene_nearest(c.handle, None, 0, None, None) == 0                        # n == 0: RT_OK, nothing done
        b_pts, b_small, b_alien = c.create_buffer(pts), c.create_buffer(np.zeros(n - 1, T.nearest)), other.create_buffer(np.zeros(n, T.nearest))
        b_surf = c.create_buffer(np.zeros(n + 1, T.surface))
        refused(lib.rt_scene_nearest_buffer(c.handle, b_pts.handle, n, b_small.handle, None), "the out buffer is smaller than n", c.handle); still_works()
        refused(lib.rt_scene_nearest_buffer(c.handle, b_pts.handle, n + 1, None, b_surf.handle), "the points buffer is smaller than n", c.handle); still_works()
        refused(lib.rt_scene_nearest_buffer(c.handle, b_pts.handle, n, b_alien.handle, None), "another context", c.handle); still_works()
        refused(lib.rt_scene_nearest_buffer(c.handle, None, n, b_small.handle, None), "points is NULL", c.handle); still_works()
        refused(lib.rt_scene_nearest_buffer(c.handle, b_pts.handle, n, None, None), "no output", c.handle); still_works()
        assert b_small.read(T.nearest, n - 1).tobytes() == bytes(32 * (n - 1)) and b_surf.read(T.surface, n + 1).tobytes() == bytes(64 * (n + 1))
        assert lib.rt_scene_nearest_buffer(c.handle, None, 0, None, None) == 0
        for b in (b_pts, b_small, b_alien, b_surf):
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
    rng = np.random.default_rng(9)
    pts = points_of((lo + rng.uniform(0.1, 0.9, (40, 3)) * (hi - lo)).astype(f32))
    pts["max_distance"][::5] = f32(1e-6)                                    # some find nothing
    want = capi.debug_nearest(None, tris, pts)
    got = render.nearest(pts)                                              # Render::Nearest through rth_render_nearest
    same_records(np.array([g["nearest"] for g in got], T.nearest), want, "host.Render.nearest")
    seen = set()
    for g, w in zip(got, want):
        assert g["primitive_id"] == w["primitive_id"]
        if w["primitive_id"] == INVALID:
            assert g["object_name"] is None
        else:
            assert g["object_name"] == names[owner[w["primitive_id"]]] and g["t"] == w["distance"]
            seen.add(g["object_name"])
    assert len(seen) > 1 and (want["primitive_id"] == INVALID).any()        # more than one object was told apart; some points found nothing
    c = capi.Context(0)
    try:
        c.upload_scene(render.scene_arrays())
        same_records(c.nearest(pts), want, "capi")
    finally:
        c.close()
    i = int(np.flatnonzero(want["primitive_id"] != INVALID)[0])
    p = pts["position"][i]
    r = subprocess.run([os.path.join(root, "raytracing_amd", "rt_render"), "-w", "32", "-h", "24", "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--nearest", "%.9g,%.9g,%.9g" % tuple(p), "--nearest", "%.9g,%.9g,%.9g,1e-6" % tuple(pts["position"][0])], cwd=root, capture_output=True, text=True,
                       timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("nearest ")]
    assert r.returncode == 0 and len(lines) == 2, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    assert ("primitive %d " % want["primitive_id"][i]) in lines[0] and lines[0].rstrip().replace(" (back side)", "").endswith(got[i]["object_name"]), lines[0]
    assert lines[1].rstrip().endswith(": none"), lines[1]
