"""All hits on the device: rt_scene_trace_all / rt_scene_trace_all_buffer / rt_frame_pick_all against rt_debug_trace_all's host brute
force over the leaves, byte for byte, whichever tree or fold is walked, after a refit and a pose; the forms, the surfaces, the frames left alone, the
refusals, and the layers above the C-ABI.  tests/test_all_hits.py ties the brute force itself to numpy and to the independent oracle."""
import os
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T
from tests.test_gpu_query import make_batch, context, INVALID, MAX_DIST, Case as QueryCase
from tests.test_gpu_pose import city, scene_case          # noqa: F401 (city is a fixture)
from tests.test_all_hits import sheets_scene, sheet_directions, ray_rows, SHEET_X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
COUNTS = [1, 63, 64, 65, 257, 4099]


class Case(QueryCase):
    """a scene, its rays and the host brute force's answers (computed once, shared, never changed)"""

    def __init__(self, name, scene, cam, rays=None):
        super().__init__(name, scene, cam)
        self.fixed_rays, self.brute = rays, {}

    def rays(self, n):
        if self.fixed_rays is not None:
            return self.fixed_rays[np.arange(n) % len(self.fixed_rays)]
        if n not in self.batches:
            self.batches[n] = make_batch(self.scene, self.cam, self.orc, self.wide, self.entry, n, 1000 + n)
        return self.batches[n]

    def want(self, n, scene=None, key=None):
        k = (n, key)
        if k not in self.brute:
            sc = scene or self.scene
            self.brute[k] = capi.debug_trace_all(None, sc["nodes"], sc["triangles"], self.rays(n), 8)
        return self.brute[k]


def sheet_rays():
    """rays about the stack of sheets: through all twelve (count > 8), from inside and outside the box, an axis-parallel one (the child-pair walk), one not walked"""
    rng = np.random.default_rng(11)
    rows = [ray_rows([[1.5, 0.3, -0.2]], [np.array([1.0, 0.05, 0.02]) / np.linalg.norm([1.0, 0.05, 0.02])]), ray_rows([[1.5, 0.25, -0.5]], [[1.0, 0.0, 0.0]])]
    for origin in ((0.1, -0.2, 0.3), (0.3, 0.2, 5.0), (-3.0, 0.4, -0.1)):
        rows.append(ray_rows(np.tile(np.array(origin, f32), (20, 1)), sheet_directions(rng, origin, 20, towards=8)))
    bad = ray_rows([[0.0, np.nan, 0.0]], [[1.0, 0.0, 0.0]])
    return np.concatenate(rows + [bad]).view(T.ray).reshape(-1)


@pytest.fixture(scope="module")
def cases(golden_scenes, golden_radiance, city):
    sheets = sheets_scene()
    a = {k: np.array(v) for k, v in sheets.arrays().items()}
    return {"cornell": Case("cornell", golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]),
            "coverage": Case("coverage", golden_scenes["coverage"], golden_radiance["coverage_64_b6_s2/camera"]),
            "city": Case("city", city, T.default_camera(64, 64)),
            "sheets": Case("sheets", a, T.default_camera(64, 64), sheet_rays())}


def check(got, want, k, what):
    """a query with max_hits = k against the brute force's 8-list: the records, and the list's prefix"""
    rec, hits = (got, None) if k == 0 else got[:2]
    wrec, whits = want
    assert np.array_equal(rec["count"], wrec["count"]) and np.array_equal(rec["entering"], wrec["entering"]), (what, np.flatnonzero(rec["count"] != wrec["count"])[:8])
    assert np.array_equal(rec["stored"], np.minimum(wrec["count"], k)), what
    mask = (1 << (8 + k)) - 1
    assert np.array_equal(rec["flags"], wrec["flags"] & mask), what
    if k:
        assert hits.tobytes() == np.ascontiguousarray(whits[:, :k]).tobytes(), what


# ---- 1. the device equals the brute force

@pytest.mark.parametrize("tree", ["wide", "wide_off", "shared_shadow_tree"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city", "sheets"])
def test_the_device_equals_the_brute_force(cases, name, tree):
    case = cases[name]
    c = context(wide=0 if tree == "wide_off" else 1, shadow_tree=0 if tree == "shared_shadow_tree" else None)
    try:
        c.upload_scene(case.scene)
        for n in COUNTS:
            rays, want = case.rays(n), case.want(n)
            for k in (0, 3, 8):
                check(c.trace_all(rays, k), want, k, (name, tree, n, k))
        assert (case.want(4099)[0]["count"] >= 2).any()
    finally:
        c.close()


def test_the_device_brute_force_equals_the_hosts(cases):
    c = context()
    try:
        for name, n in (("cornell", 257), ("coverage", 65), ("sheets", 64), ("city", 63), ("cornell", 1)):
            case = cases[name]
            for k in (0, 8):
                rec, hits = capi.debug_trace_all(c, case.scene["nodes"], case.scene["triangles"], case.rays(n), k)
                wrec, whits = capi.debug_trace_all(None, case.scene["nodes"], case.scene["triangles"], case.rays(n), k)
                assert rec.tobytes() == wrec.tobytes() and hits.tobytes() == whits.tobytes(), (name, n, k)
    finally:
        c.close()


# ---- 2. adapted folds, refit, pose

def test_adapted_folds_answer_the_same(cases):
    case = cases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(case.cam); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report
        check(c.trace_all(case.rays(4099), 8), case.want(4099), 8, "adapted")
        fr.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["cornell", "city"])
def test_all_hits_follow_refit_and_pose(cases, name, golden_scenes, city):
    case = cases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    rays = case.rays(4099)
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    nodes, _, _ = capi.debug_refit(None, sc["nodes"], posed)
    want = capi.debug_trace_all(None, nodes, posed, rays, 8)             # brute force over the refitted leaves and the moved triangles
    assert not np.array_equal(want[1]["t"], case.want(4099)[1]["t"])      # (the pose did move what the rays see)
    a, b = context(refittable=True), context(refittable=True)
    try:
        a.upload_scene(sc); a.set_objects(ids, n_objects); a.pose_scene(mats)
        check(a.trace_all(rays, 8), want, 8, "pose")
        b.upload_scene(sc); b.refit_scene(posed)
        check(b.trace_all(rays, 8), want, 8, "refit")
    finally:
        a.close(); b.close()


# ---- 3. forms agree

def test_forms_and_outputs_agree(cases):
    case = cases["coverage"]
    c = context()
    try:
        c.upload_scene(case.scene)
        rays = case.rays(4099)
        n, k = len(rays), 3
        rec, hits, surf = c.trace_all(rays, k, surfaces=True)
        check((rec, hits), case.want(4099), k, "host arrays")
        b_rays, b_rec = c.create_buffer(rays), c.create_buffer(np.zeros(n, T.ray_hits))
        b_hits, b_surf, b_only = c.create_buffer(np.zeros(n * k, T.hit)), c.create_buffer(np.zeros(n * k, T.surface)), c.create_buffer(np.zeros(n * k, T.surface))
        c.trace_all_buffer(b_rays, n, k, b_rec, hits=b_hits, surfaces=b_surf)
        assert b_rec.read(T.ray_hits, n).tobytes() == rec.tobytes() and b_hits.read(T.hit, n * k).tobytes() == hits.tobytes()
        assert b_surf.read(T.surface, n * k).tobytes() == surf.tobytes()
        c.trace_all_buffer(b_rays, n, k, b_rec, surfaces=b_only)            # surfaces alone: the hits pass through the records themselves
        assert b_only.read(T.surface, n * k).tobytes() == surf.tobytes() and b_rec.read(T.ray_hits, n).tobytes() == rec.tobytes()
        c.trace_all_buffer(b_rays, n, 0, b_rec)
        check(b_rec.read(T.ray_hits, n), case.want(4099), 0, "buffers, counts alone")
        # the surfaces are the host restatement's of the stored hits
        host_surf = capi.debug_query_surface(None, case.scene["triangles"], np.repeat(rays, k), hits.reshape(-1))
        assert surf.reshape(-1).tobytes() == host_surf.tobytes()
        stored = hits["primitive_id"] != INVALID
        assert stored.any() and (~stored).any() and not surf[~stored]["flags"].any()
        exits = ((rec["flags"][:, None] >> (8 + np.arange(k))[None]) & 1).astype(bool)
        usable = stored & (np.abs(surf["geometric_normal"]).sum(-1) > 0)
        assert np.array_equal(((surf["flags"] & 2) != 0)[usable], exits[usable]) and exits[usable].any()      # an exit is a surface met from behind
        # ... and a bake takes them
        b_out = c.create_buffer(np.zeros(n * k, T.bake_result))
        c.bake_buffer(b_surf, n * k, b_out, 16, from_surfaces=True)
        baked = b_out.read(T.bake_result, n * k)
        assert (baked["unoccluded"][stored.reshape(-1)] <= 16).any() and (baked["unoccluded"][~stored.reshape(-1)] == INVALID).all()
        for b in (b_rays, b_rec, b_hits, b_surf, b_only, b_out):
            b.close()
    finally:
        c.close()


def test_pick_all_starts_with_the_pick(cases):
    case = cases["cornell"]
    w = h = 16
    c = context()
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, w, h)
        fr.set_camera(case.cam)
        deeper = 0
        for y in range(h):
            for x in range(w):
                ray, hit, surf = fr.pick(x, y)
                ray_a, rec, hits, surfs = fr.pick_all(x, y)
                assert ray_a.tobytes() == ray.tobytes()
                enter = [j for j in range(int(rec["stored"])) if not (int(rec["flags"]) >> (8 + j)) & 1]
                if hit["primitive_id"] == INVALID:
                    assert rec["entering"] == 0
                    continue
                first = enter[0]
                if len(enter) > 1 and hits["t"][enter[1]] == hits["t"][first]:
                    continue                                                # a tie in t: the reference's own order decides the pick
                assert hits[first].tobytes() == hit.tobytes() and surfs[first].tobytes() == surf.tobytes(), (x, y)
                deeper += int(rec["count"]) > 1
        assert deeper > 0
        fr.close()
    finally:
        c.close()


# ---- 4. frames are undisturbed

@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(cases, ahead):
    case = cases["cornell"]
    rays = case.rays(257)
    c = context()
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(case.cam); fr.set_max_bounces(4)
            fr.set_option(capi.OPT_SAMPLES_AHEAD, ahead)
            fr.guides()
            for k in range(4):
                fr.integrate(1)
                if disturb and k < 3:
                    c.trace_all(rays, 8, surfaces=True); c.trace_all(rays, 0); fr.pick_all(5, 7)
            st = fr.stats()
            out = (fr.radiance().tobytes(), (st.closest_rays, st.shadow_rays, st.samples, tuple(st.last_active), tuple(st.last_shadow), st.samples_ahead,
                   st.samples_from_banks, st.slow_rays), fr.guides()[3])
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    finally:
        c.close()


# ---- 5. refusals

def test_refusals_launch_nothing_and_leave_queries_working(cases):
    case = cases["cornell"]
    rays, n = case.rays(65), 65
    lib = capi.load()
    c, other = context(), context()
    try:
        rec, hits, surf = np.zeros(n, T.ray_hits), np.zeros((n, 8), T.hit), np.zeros((n, 8), T.surface)
        p = lambda a: a.ctypes.data

        def refused(rc, text, handle=None):
            assert rc != 0 and text in lib.rt_last_error(handle).decode(), (rc, lib.rt_last_error(handle).decode())

        refused(lib.rt_scene_trace_all(c.handle, p(rays), n, 8, p(rec), p(hits), None), "no scene", c.handle)
        fr0 = capi.Frame(c, 16, 12)
        refused(lib.rt_frame_pick_all(fr0.handle, 1, 1, 8, None, p(rec), p(hits), None), "no scene", c.handle)
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)

        def still_works():
            check(c.trace_all(rays, 8), case.want(65), 8, "after a refusal")

        refused(lib.rt_scene_trace_all(None, p(rays), n, 8, p(rec), p(hits), None), "ctx is NULL"); still_works()
        refused(lib.rt_scene_trace_all(c.handle, None, n, 8, p(rec), p(hits), None), "rays is NULL", c.handle); still_works()
        refused(lib.rt_scene_trace_all(c.handle, p(rays), n, 8, None, p(hits), None), "out is NULL", c.handle); still_works()
        refused(lib.rt_scene_trace_all(c.handle, p(rays), n, 9, p(rec), p(hits), None), "RT_ALL_HITS_MAX", c.handle); still_works()
        refused(lib.rt_scene_trace_all(c.handle, p(rays), n, 0, p(rec), p(hits), None), "max_hits == 0", c.handle); still_works()
        refused(lib.rt_scene_trace_all(c.handle, p(rays), n, 0, p(rec), None, p(surf)), "max_hits == 0", c.handle); still_works()
        assert rec.tobytes() == bytes(rec.nbytes) and hits.tobytes() == bytes(hits.nbytes) and surf.tobytes() == bytes(surf.nbytes)      # nothing was written
        assert lib.rt_scene_trace_all(c.handle, None, 0, 8, None, None, None) == 0           # n == 0: RT_OK, nothing done
        b_rays, b_rec = c.create_buffer(rays), c.create_buffer(np.zeros(n, T.ray_hits))
        b_small, b_alien = c.create_buffer(np.zeros(n * 8 - 1, T.hit)), other.create_buffer(np.zeros(n * 8, T.hit))
        b_surf = c.create_buffer(np.zeros(n * 3, T.surface))
        refused(lib.rt_scene_trace_all_buffer(c.handle, b_rays.handle, n, 8, b_rec.handle, b_small.handle, None), "the hits buffer is smaller", c.handle); still_works()
        refused(lib.rt_scene_trace_all_buffer(c.handle, b_rays.handle, n, 4, b_rec.handle, None, b_surf.handle), "the surfaces buffer is smaller", c.handle); still_works()
        refused(lib.rt_scene_trace_all_buffer(c.handle, b_rays.handle, n + 1, 0, b_rec.handle, None, None), "the rays buffer is smaller", c.handle); still_works()
        refused(lib.rt_scene_trace_all_buffer(c.handle, b_rays.handle, n, 8, b_rec.handle, b_alien.handle, None), "another context", c.handle); still_works()
        refused(lib.rt_scene_trace_all_buffer(c.handle, None, n, 8, b_rec.handle, None, None), "rays is NULL", c.handle); still_works()
        refused(lib.rt_scene_trace_all_buffer(c.handle, b_rays.handle, n, 8, None, None, None), "out is NULL", c.handle); still_works()
        assert b_rec.read(T.ray_hits, n).tobytes() == bytes(16 * n) and b_surf.read(T.surface, n * 3).tobytes() == bytes(64 * n * 3)
        refused(lib.rt_frame_pick_all(None, 0, 0, 8, None, p(rec), None, None), "frame is NULL"); still_works()
        refused(lib.rt_frame_pick_all(fr0.handle, 16, 0, 8, None, p(rec), p(hits), None), "outside the image", c.handle); still_works()
        refused(lib.rt_frame_pick_all(fr0.handle, 1, 1, 9, None, p(rec), p(hits), None), "RT_ALL_HITS_MAX", c.handle); still_works()
        tile = capi.Frame(c, 16, 12, tile_rank=0, tile_count=2, band_height=4)
        refused(lib.rt_frame_pick_all(tile.handle, 1, 1, 8, None, p(rec), p(hits), None), "tile frame", c.handle); still_works()
        assert rec.tobytes() == bytes(rec.nbytes) and hits.tobytes() == bytes(hits.nbytes)
        for b in (b_rays, b_rec, b_small, b_alien, b_surf):
            b.close()
        tile.close(); fr0.close()
    finally:
        c.close(); other.close()


# ---- 6. layers

def test_layers_pick_all_names_objects_and_equals_capi():
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"), objects=True)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    w, h = 32, 24
    render = host.Render(w, h, scene)
    cam = host.default_camera(w, h)
    render.set_camera(cam); render.set_max_bounces(4)
    names, owner = scene.object_names(), scene.triangle_objects()
    c = capi.Context(0)
    try:
        c.upload_scene(render.scene_arrays())
        fr = capi.Frame(c, w, h)
        fr.set_camera(cam)
        layered = 0
        for x, y in ((16, 12), (4, 20), (27, 5), (10, 3), (22, 18)):
            got = render.pick_all(x, y)                                     # Render::PickAll through rth_render_pick_all: the camera is still pending
            ray, rec, hits, surfs = fr.pick_all(x, y)
            assert len(got) == rec["stored"] and len(got) >= 1
            first = render.pick(x, y)
            assert got[0]["primitive_id"] == first["primitive_id"] and got[0]["object_name"] == first["object_name"]
            for j, g in enumerate(got):
                assert g["hit"].tobytes() == hits[j].tobytes() and g["ray"].tobytes() == ray.tobytes()
                assert g["object_name"] == names[owner[g["primitive_id"]]] and g["exit"] == bool((int(rec["flags"]) >> (8 + j)) & 1)
            layered += len(got) > 1
        assert layered > 0                                                  # something lies behind the first surface
        rays = np.array([fr.pick(x, 12)[0] for x in range(w)], T.ray)
        got, want = render.trace_all(rays, 8, surfaces=True), c.trace_all(rays, 8, surfaces=True)      # HIPPathTraceIntegrator::TraceAllHits through rth_render_trace_all
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert all(got[2][k].tobytes() == want[2][k].tobytes() for k in T.surface.names if k != "object")
        assert render.trace_all(rays, 0).tobytes() == c.trace_all(rays, 0).tobytes()
        fr.close()
    finally:
        c.close()


def test_inside_and_signed_distances_on_the_sheets_box():
    scene = sheets_scene()
    render = host.Render(16, 16, scene)
    render.set_camera(host.default_camera(16, 16))
    rng = np.random.default_rng(5)
    # x <= 0: along the default direction (0.36, 0.48, 0.8) such a ray is above the sheets (z > 2) before it reaches their planes, so only the box counts
    inner = (rng.uniform(-0.9, 0.9, (40, 3)) * [0.5, 1.0, 1.0] - [0.45, 0.0, 0.0]).astype(f32)
    # outside: above the box, and behind it so that the ray runs through the box (one entry, one exit)
    outer = np.concatenate([rng.uniform(-0.9, 0.9, (20, 3)) + [0.0, 0.0, 3.0], inner[:20].astype(np.float64) - 3.0 * np.array(host.Render.INSIDE_DIRECTION)]).astype(f32)
    points = np.concatenate([inner, outer])
    want = np.arange(len(points)) < len(inner)
    assert np.array_equal(render.inside(points), want)
    found = render.nearest(points, signed=True)
    for i, f in enumerate(found):
        assert f["inside"] == bool(want[i]) and (f["signed_distance"] < 0) == bool(want[i])
        assert abs(f["signed_distance"]) == float(f["nearest"]["distance"])
    wall = 1.0 - np.abs(inner).max(1)                                       # inside the box the nearest surface is the nearest wall
    got = np.array([-f["signed_distance"] for f in found[:len(inner)]])
    assert np.allclose(got, wall, atol=1e-6)
