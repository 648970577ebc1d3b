"""-m gpu: ray queries (rt_scene_trace / rt_scene_trace_buffer / rt_frame_pick, raytracing_amd/csrc/query.hip) on the device.

The contract: a closest-hit query returns bc, primitive_id and t bit for bit as the reference's IntersectRays would, an any-hit query the reference's verdict,
whichever tree is walked.  The reference's answer is the CPU oracle's walk (tests/_oracle.py: wide_trace over rt_debug_wide_bvh's records; it takes the
reference's own loop whenever t_min != 0).  Every batch mixes camera rays, random rays from inside the scene, axis-parallel directions and origins beyond 2^29
(the child-pair walk), t_min just past the first surface, t_max short of it, t_min > t_max, and rays that are not walked (NaN, Inf, a zero direction).
One process, each GPU step once, nothing retried; nothing here provokes a fault."""
import ctypes as C
import os
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests import _oracle
from tests.test_wide_bvh import wide_of
from tests.test_refit import positions
from tests.test_pose import IDENTITY, translation, rotation
from tests.test_gpu_pose import city, cornell_objects, city_objects, scene_case          # noqa: F401 (city is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INVALID = 0xFFFFFFFF
MAX_DIST = f32(20000.0)
OPT_WIDE_BVH, OPT_SHADOW_TREE, OPT_ADAPTIVE_FOLD = 1, 2, 4
COUNTS = [1, 63, 64, 65, 257, 4099]
CLASSES = 12          # a batch's ray i is of class i % CLASSES (below)
NOT_WALKED = 10


def camera_rays(cam, n, rng):
    """n pinhole rays of `cam` through random image points (numpy; any ray serves, the device's own generation is not under test)"""
    fr = np.array([cam["front"][k] for k in "xyz"], np.float64)
    up = np.array([cam["up"][k] for k in "xyz"], np.float64)
    right = np.cross(fr, up)
    tan_half = np.tan(0.5 * float(cam["fov"]))
    x = rng.uniform(-1, 1, n) * tan_half * float(cam["aspect_ratio"])
    y = rng.uniform(-1, 1, n) * tan_half
    d = right[None] * x[:, None] + up[None] * y[:, None] + fr[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, T.ray)
    for c, k in enumerate("xyz"):
        rays["origin"][k] = f32(cam["position"][k])
        rays["direction"][k] = d[:, c].astype(f32)
    rays["direction"]["w"] = MAX_DIST
    return rays


def make_batch(scene, cam, orc, wide, entry, n, seed):
    """the mixed batch: class of ray i = i % 12 -- 0, 4, 7, 11 camera rays; 1, 9 random origin inside the bounds, random direction; 2 a camera ray with t_min
    just past its first surface (the second surface is found); 3 an axis-parallel direction from inside (zero components: 1/dir is not finite); 5 an origin
    beyond 2^29 looking at the scene; 6 a camera ray with t_max short of its first surface; 8 t_min > t_max; 10 not walked (NaN / Inf component, zero direction)"""
    rng = np.random.default_rng(seed)
    p = positions(scene["triangles"]).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    rays = camera_rays(cam, n, rng)
    first = orc.wide_trace(wide, entry, rays, False)                       # the camera rays' first surfaces
    t1 = np.where(first["primitive_id"] != INVALID, first["t"], f32(1.0)).astype(f32)
    cls = np.arange(n) % CLASSES
    inside = (lo[None] + rng.uniform(0.05, 0.95, (n, 3)) * (hi - lo)[None]).astype(f32)
    rnd = rng.normal(size=(n, 3))
    rnd = (rnd / np.linalg.norm(rnd, axis=1, keepdims=True)).astype(f32)
    axis = np.zeros((n, 3), f32)
    axis[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)

    def put(mask, origin=None, direction=None, t_min=None, t_max=None):
        for c, k in enumerate("xyz"):
            if origin is not None:
                rays["origin"][k][mask] = origin[mask, c]
            if direction is not None:
                rays["direction"][k][mask] = direction[mask, c]
        if t_min is not None:
            rays["origin"]["w"][mask] = t_min[mask] if np.ndim(t_min) else t_min
        if t_max is not None:
            rays["direction"]["w"][mask] = t_max[mask] if np.ndim(t_max) else t_max

    put((cls == 1) | (cls == 9), origin=inside, direction=rnd)
    put(cls == 2, t_min=(t1 * f32(1.0001) + f32(1e-4)).astype(f32))
    put(cls == 3, origin=inside, direction=axis)
    centre = ((lo + hi) / 2).astype(f32)
    put(cls == 5, origin=(centre[None] - rnd * f32(2.0 ** 30)).astype(f32), direction=rnd, t_max=f32(2.0 ** 31))
    put(cls == 6, t_max=(t1 * f32(0.9)).astype(f32))
    put(cls == 8, t_min=(t1 * f32(2.0)).astype(f32), t_max=(t1 * f32(1.5)).astype(f32))
    bad = np.flatnonzero(cls == NOT_WALKED)
    for k, i in enumerate(bad):
        kind = k % 6
        if kind == 0: rays["origin"]["y"][i] = np.nan
        elif kind == 1: rays["direction"]["x"][i] = np.inf
        elif kind == 2: rays["origin"]["w"][i] = np.nan
        elif kind == 3: rays["direction"]["w"][i] = np.inf
        elif kind == 4: rays["direction"]["x"][i] = rays["direction"]["y"][i] = rays["direction"]["z"][i] = 0.0
        else: rays["origin"]["z"][i] = -np.inf
    return rays


def expected(orc, wide, entry, rays):
    """(closest hits, any-hit verdicts) of the oracle; a ray that is not walked is a miss by the contract (decided before any walk)"""
    hits = orc.wide_trace(wide, entry, rays, False).copy()
    occ = (orc.wide_trace(wide, entry, rays, True) != INVALID).astype(np.uint32)
    comp = np.stack([rays["origin"][k] for k in "xyzw"] + [rays["direction"][k] for k in "xyzw"], -1)
    zero_dir = (comp[:, 4:7] == 0).all(1)
    skipped = ~np.isfinite(comp).all(1) | zero_dir
    hits["primitive_id"][skipped] = INVALID
    occ[skipped] = 0
    return hits, occ, skipped


def check_closest(got, want, what=""):
    assert np.array_equal(got["primitive_id"], want["primitive_id"]), (what, int((got["primitive_id"] != want["primitive_id"]).sum()))
    hit = want["primitive_id"] != INVALID
    assert got["bc"][hit].tobytes() == want["bc"][hit].tobytes() and got["t"][hit].tobytes() == want["t"][hit].tobytes(), what
    assert 2 * hit.sum() >= len(want), (what, "fewer than half of the batch's rays hit", int(hit.sum()), len(want))


class Case:
    """a scene, its camera, its oracle and the batches' expected answers (computed once, shared, never changed)"""

    def __init__(self, name, scene, cam):
        self.name, self.scene, self.cam = name, scene, cam
        self.orc = _oracle.Oracle(16, 16, scene)
        self.wide, self.entry = wide_of(scene["nodes"], 1)
        self.batches = {}

    def batch(self, n):
        if n not in self.batches:
            rays = make_batch(self.scene, self.cam, self.orc, self.wide, self.entry, n, 1000 + n)
            self.batches[n] = (rays,) + expected(self.orc, self.wide, self.entry, rays)
        return self.batches[n]


@pytest.fixture(scope="module")
def cases(golden_scenes, golden_radiance, city):
    return {"cornell": Case("cornell", golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]),
            "coverage": Case("coverage", golden_scenes["coverage"], golden_radiance["coverage_64_b6_s2/camera"]),
            "city": Case("city", city, T.default_camera(64, 64))}


def context(wide=1, shadow_tree=None, adaptive=None, refittable=False):
    c = capi.Context(0)
    if wide != 1:
        c.set_wide_bvh(wide)
    if shadow_tree is not None:
        c.set_shadow_tree(shadow_tree)
    if adaptive is not None:
        c.set_adaptive_fold(adaptive)
    if refittable:
        c.set_refittable(True)
    return c


# ---- 1. closest hits equal the oracle's

@pytest.mark.parametrize("wide", [1, 0], ids=["wide_trees", "wide_trees_off"])
@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_closest_hits_equal_the_oracle(cases, name, wide):
    case = cases[name]
    c = context(wide=wide)
    try:
        c.upload_scene(case.scene)
        for n in COUNTS:
            rays, want, _, skipped = case.batch(n)
            got = c.trace(rays)
            check_closest(got, want, (name, wide, n))
            assert (got["primitive_id"][skipped] == INVALID).all()
    finally:
        c.close()


# ---- 2. any-hit verdicts equal the oracle's

@pytest.mark.parametrize("shadow_tree", [1, 0], ids=["own_shadow_tree", "shared_tree"])
def test_any_hit_verdicts_equal_the_oracle(cases, shadow_tree):
    case = cases["city"]                                                   # a directional light over a city: the upload measures an own shadow tree and chooses it
    c = context(shadow_tree=shadow_tree)
    try:
        c.upload_scene(case.scene)
        report = c.tree_report()
        if shadow_tree:
            line = [ln for ln in report.splitlines() if ln.startswith("shadow tree: ")]
            assert line and line[-1].endswith("-> own"), report              # the own tree is the one the any-hit queries walk
        for n in COUNTS:
            rays, want, occ, _ = case.batch(n)
            got = c.trace(rays, any_hit=True)
            assert np.array_equal(got, occ), (n, int((got != occ).sum()))
            assert np.array_equal(occ != 0, want["primitive_id"] != INVALID)      # (with t_max fixed a ray is occluded exactly when it has a closest hit)
    finally:
        c.close()


# ---- 3. adapted folds

def test_adapted_folds_answer_the_same(cases):
    case = cases["city"]
    c = context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)               # wait for the fold; small trees too
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(case.cam); fr.set_max_bounces(3)
        fr.integrate(1)
        report = c.tree_report()
        assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report     # adapted records are what the queries below walk
        rays, want, occ, _ = case.batch(4099)
        check_closest(c.trace(rays), want, "adapted")
        assert np.array_equal(c.trace(rays, any_hit=True), occ)
        fr.close()
    finally:
        c.close()


# ---- 4. moving geometry

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_queries_follow_refit_and_pose(cases, name, golden_scenes, golden_radiance, city):
    case = cases[name]
    sc, ids, n_objects, mats = scene_case(name, golden_scenes, city)
    rays = case.batch(4099)[0]
    a = context(refittable=True)
    try:
        a.upload_scene(sc)
        _, surf = a.trace(rays, surfaces=True)
        hit = surf["primitive_id"] != INVALID
        assert hit.any() and (surf["object"][hit] == INVALID).all()         # no objects set yet
        a.set_objects(ids, n_objects)
        a.pose_scene(mats)
        posed = capi.debug_pose(None, sc["triangles"], ids, mats)
        moved = dict(sc); moved["triangles"] = posed
        hits_a, surf_a = a.trace(rays, surfaces=True)
        occ_a = a.trace(rays, any_hit=True)
        hit = surf_a["primitive_id"] != INVALID
        assert np.array_equal(surf_a["object"][hit], ids[surf_a["primitive_id"][hit]])
        b = context(refittable=True)
        try:
            b.upload_scene(sc)
            b.refit_scene(posed)                                            # after a refit ...
            hits_b, surf_b = b.trace(rays, surfaces=True)
            occ_b = b.trace(rays, any_hit=True)
        finally:
            b.close()
        # ... and both against a fresh context's answer: the refit's node bounds are the refitted ones, so the fresh upload gets those nodes
        nodes, _, _ = capi.debug_refit(None, sc["nodes"], posed)
        moved["nodes"] = nodes
        f = context()
        try:
            f.upload_scene(moved)
            hits_f, surf_f = f.trace(rays, surfaces=True)
            occ_f = f.trace(rays, any_hit=True)
        finally:
            f.close()
        for got_h, got_s, got_o, who in ((hits_a, surf_a, occ_a, "pose"), (hits_b, surf_b, occ_b, "refit")):
            assert np.array_equal(got_h["primitive_id"], hits_f["primitive_id"]), who
            h = hits_f["primitive_id"] != INVALID
            assert got_h[h].tobytes() == hits_f[h].tobytes(), who
            for k in T.surface.names:
                if k != "object":
                    assert got_s[k].tobytes() == surf_f[k].tobytes(), (who, k)
            assert np.array_equal(got_o, occ_f), who
        assert not np.array_equal(hits_f["t"], case.batch(4099)[1]["t"])     # (the pose did move what the rays see)
    finally:
        a.close()


# ---- 5. forms and outputs

def test_forms_and_outputs_agree(cases):
    case = cases["coverage"]
    c = context()
    try:
        c.upload_scene(case.scene)
        rays, want, occ, _ = case.batch(4099)
        n = len(rays)
        hits, surf = c.trace(rays, surfaces=True)
        check_closest(hits, want, "host arrays")
        assert c.trace(rays.view(f32).reshape(-1, 8)).tobytes() == hits.tobytes()        # float rows: the same rule
        b_rays = c.create_buffer(rays)
        b_hits, b_occ, b_surf = c.create_buffer(np.zeros(n, T.hit)), c.create_buffer(np.zeros(n, np.uint32)), c.create_buffer(np.zeros(n, T.surface))
        c.trace_buffer(b_rays, n, hits=b_hits, occluded=b_occ, surfaces=b_surf)
        assert b_hits.read(T.hit, n).tobytes() == hits.tobytes()
        assert b_surf.read(T.surface, n).tobytes() == surf.tobytes()
        assert np.array_equal(b_occ.read(np.uint32, n), (hits["primitive_id"] != INVALID).astype(np.uint32))
        b_only = c.create_buffer(np.zeros(n, T.surface))
        c.trace_buffer(b_rays, n, surfaces=b_only)                          # surfaces alone: the hits pass through the records themselves
        assert b_only.read(T.surface, n).tobytes() == surf.tobytes()
        c.trace_buffer(b_rays, n, any_hit=True, occluded=b_occ)
        assert np.array_equal(b_occ.read(np.uint32, n), occ)
        # the surfaces are the host restatement's of the same rays and hits, and so are the kernel's on caller triangles
        host_surf = capi.debug_query_surface(None, case.scene["triangles"], rays, hits)
        assert surf.tobytes() == host_surf.tobytes(), [k for k in T.surface.names if surf[k].tobytes() != host_surf[k].tobytes()]
        ids = (np.arange(len(case.scene["triangles"])) % 5).astype(np.uint32)
        for objects in (None, ids):
            assert capi.debug_query_surface(c, case.scene["triangles"], rays, hits, objects).tobytes() == \
                   capi.debug_query_surface(None, case.scene["triangles"], rays, hits, objects).tobytes()
        miss = hits["primitive_id"] == INVALID
        assert miss.any() and not surf[miss]["flags"].any() and not surf[miss]["position"].any()
        assert "ray queries: " in c.tree_report()
        for b in (b_rays, b_hits, b_occ, b_surf, b_only):
            b.close()
    finally:
        c.close()


# ---- 6. pick

@pytest.mark.parametrize("name", ["cornell", "city"])
def test_pick_every_pixel(cases, name):
    case = cases[name]
    w, h = 16, 12
    c = context()
    try:
        c.upload_scene(case.scene)
        fr = capi.Frame(c, w, h)
        cam = case.cam.copy(); cam["aspect_ratio"] = f32(w) / f32(h)
        fr.set_camera(cam)
        picks = [fr.pick(x, y) for y in range(h) for x in range(w)]
        rays = np.array([p[0] for p in picks], T.ray)
        hits = np.array([p[1] for p in picks], T.hit)
        surf = np.array([p[2] for p in picks], T.surface)
        want = case.orc.wide_trace(case.wide, case.entry, rays, False)
        assert np.array_equal(hits["primitive_id"], want["primitive_id"])
        hit = want["primitive_id"] != INVALID
        assert hits[hit].tobytes() == want[hit].tobytes()
        assert (rays["origin"]["w"] == 0).all() and (rays["direction"]["w"] == MAX_DIST).all()
        _, nrm, dep, _ = fr.guides()
        g_hit = (dep < MAX_DIST).ravel()
        assert np.array_equal(g_hit, hit) and hit.any()                      # misses agree on both sides
        assert surf["shading_normal"][hit].tobytes() == nrm.reshape(-1, 4)[hit][:, :3].tobytes()
        o = np.stack([rays["origin"][k] for k in "xyz"], -1)
        dlt = o - surf["position"]
        depth = np.sqrt((dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]).astype(f32)     # length3, binary32, summed left to right
        assert depth[hit].tobytes() == dep.ravel()[hit].tobytes()
        fr.close()
    finally:
        c.close()


# ---- 7. frames are undisturbed

@pytest.mark.parametrize("ahead", [1, 0], ids=["samples_ahead", "samples_ahead_off"])
def test_frames_are_undisturbed(cases, ahead):
    case = cases["cornell"]
    rays = case.batch(257)[0]
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
                    c.trace(rays); c.trace(rays, any_hit=True); fr.pick(5, 7)
            st = fr.stats()
            out = (fr.radiance().tobytes(), (st.closest_rays, st.shadow_rays, st.samples, tuple(st.last_active), tuple(st.last_shadow), st.samples_ahead,
                   st.samples_from_banks, st.slow_rays), fr.guides()[3])
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    finally:
        c.close()


# ---- 8. refusals

def test_refusals_launch_nothing_and_leave_queries_working(cases):
    case = cases["cornell"]
    rays, want, occ, _ = case.batch(65)
    n = len(rays)
    lib = capi.load()
    c, other = context(), context()
    try:
        hits, o, surf = np.zeros(n, T.hit), np.zeros(n, np.uint32), np.zeros(n, T.surface)
        p = lambda a: a.ctypes.data

        def refused(rc, text, handle=None):
            assert rc != 0 and text in lib.rt_last_error(handle).decode(), (rc, lib.rt_last_error(handle).decode())

        refused(lib.rt_scene_trace(c.handle, p(rays), n, 0, p(hits), None, None), "no scene", c.handle)
        fr0 = capi.Frame(c, 16, 12)
        refused(lib.rt_frame_pick(fr0.handle, 1, 1, None, p(hits), None), "no scene", c.handle)
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)

        def still_works():
            check_closest(c.trace(rays), want, "after a refusal")
            assert np.array_equal(c.trace(rays, any_hit=True), occ)

        refused(lib.rt_scene_trace(None, p(rays), n, 0, p(hits), None, None), "ctx is NULL"); still_works()
        refused(lib.rt_scene_trace(c.handle, None, n, 0, p(hits), None, None), "rays is NULL", c.handle); still_works()
        refused(lib.rt_scene_trace(c.handle, p(rays), n, 2, p(hits), None, None), "unknown mode", c.handle); still_works()
        refused(lib.rt_scene_trace(c.handle, p(rays), n, 0, None, None, None), "no output", c.handle); still_works()
        refused(lib.rt_scene_trace(c.handle, p(rays), n, 1, p(hits), p(o), None), "RT_QUERY_ANY_HIT", c.handle); still_works()
        refused(lib.rt_scene_trace(c.handle, p(rays), n, 1, None, p(o), p(surf)), "RT_QUERY_ANY_HIT", c.handle); still_works()
        assert hits.tobytes() == bytes(hits.nbytes) and not o.any() and surf.tobytes() == bytes(surf.nbytes)                          # nothing was written by any of them
        assert lib.rt_scene_trace(c.handle, None, 0, 0, None, None, None) == 0               # n == 0: RT_OK, nothing done
        b_rays, b_small, b_alien = c.create_buffer(rays), c.create_buffer(np.zeros(n - 1, T.hit)), other.create_buffer(np.zeros(n, T.hit))
        b_surf = c.create_buffer(np.zeros(n + 1, T.surface))
        refused(lib.rt_scene_trace_buffer(c.handle, b_rays.handle, n, 0, b_small.handle, None, None), "smaller than n", c.handle); still_works()
        refused(lib.rt_scene_trace_buffer(c.handle, b_rays.handle, n + 1, 0, None, None, b_surf.handle), "the rays buffer is smaller than n", c.handle); still_works()
        refused(lib.rt_scene_trace_buffer(c.handle, b_rays.handle, n, 0, b_alien.handle, None, None), "another context", c.handle); still_works()
        refused(lib.rt_scene_trace_buffer(c.handle, None, n, 0, b_small.handle, None, None), "rays is NULL", c.handle); still_works()
        refused(lib.rt_scene_trace_buffer(c.handle, b_rays.handle, n, 0, None, None, None), "no output", c.handle); still_works()
        assert b_small.read(T.hit, n - 1).tobytes() == bytes(16 * (n - 1)) and b_surf.read(T.surface, n + 1).tobytes() == bytes(64 * (n + 1))
        refused(lib.rt_frame_pick(None, 0, 0, None, None, None), "frame is NULL"); still_works()
        refused(lib.rt_frame_pick(fr0.handle, 16, 0, None, p(hits), None), "outside the image", c.handle); still_works()
        refused(lib.rt_frame_pick(fr0.handle, 0, 12, None, p(hits), None), "outside the image", c.handle); still_works()
        tile = capi.Frame(c, 16, 12, tile_rank=0, tile_count=2, band_height=4)
        refused(lib.rt_frame_pick(tile.handle, 1, 1, None, p(hits), None), "tile frame", c.handle); still_works()
        assert hits.tobytes() == bytes(hits.nbytes)
        for b in (b_rays, b_small, b_alien, b_surf):
            b.close()
        fr0.set_camera(case.cam)
        ray, hit, s = fr0.pick(8, 6)
        assert hit["primitive_id"] == case.orc.wide_trace(case.wide, case.entry, np.array([ray], T.ray), False)["primitive_id"][0]
        tile.close(); fr0.close()
    finally:
        c.close(); other.close()


# ---- 9. layers

def test_layers_pick_names_the_object_and_equals_capi():
    import subprocess
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"), objects=True)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    w, h = 32, 24
    render = host.Render(w, h, scene)
    cam = host.default_camera(w, h)
    render.set_camera(cam); render.set_max_bounces(4)
    names, owner = scene.object_names(), scene.triangle_objects()
    assert len(names) > 1 and len(owner) == len(render.scene_arrays()["triangles"])
    c = capi.Context(0)
    try:
        c.upload_scene(render.scene_arrays())
        fr = capi.Frame(c, w, h)
        fr.set_camera(cam); fr.set_max_bounces(4)
        seen = set()
        for x, y in ((16, 12), (4, 20), (27, 5), (10, 3), (22, 18)):
            got = render.pick(x, y)                                             # Render::Pick through rth_render_pick: the camera is still pending
            ray, hit, surf = fr.pick(x, y)
            assert got["ray"].tobytes() == ray.tobytes() and got["hit"].tobytes() == hit.tobytes()
            for k in T.surface.names:
                if k != "object":
                    assert np.asarray(got[k], surf[k].dtype).tobytes() == np.asarray(surf[k]).tobytes(), k     # (pick() hands scalars out as Python numbers)
            assert got["primitive_id"] != INVALID                               # (the start-up camera looks into the box)
            assert got["object_name"] == names[owner[got["primitive_id"]]]
            seen.add(got["object_name"])
        assert len(seen) > 1                                                    # more than one object was told apart
        # HIPPathTraceIntegrator::Pick itself (rt_frame_pick on the integrator's frame) once a frame has handed the camera over, and a frame that had picks
        # before it equals one that had none
        render.render_samples(2)
        ray, hit, surf = np.zeros(1, T.ray), np.zeros(1, T.hit), np.zeros(1, T.surface)
        assert render.lib.rth_render_integrator_pick(render.handle, 16, 12, ray.ctypes.data, hit.ctypes.data, surf.ctypes.data) == 0
        want = fr.pick(16, 12)
        assert ray[0].tobytes() == want[0].tobytes() and hit[0].tobytes() == want[1].tobytes()
        assert all(surf[0][k].tobytes() == want[2][k].tobytes() for k in T.surface.names if k != "object")
        fr.integrate(2)
        assert render.radiance().tobytes() == fr.radiance().tobytes()
        rays = np.array([fr.pick(x, 12)[0] for x in range(w)], T.ray)
        assert render.trace(rays).tobytes() == c.trace(rays).tobytes()          # HIPPathTraceIntegrator::TraceRays through rth_render_trace
        assert np.array_equal(render.trace(rays, any_hit=True), c.trace(rays, any_hit=True))
        fr.close()
    finally:
        c.close()
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", str(w), "-h", str(h), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--pick", "16,12", "--pick", "4,20"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("pick ")]
    assert r.returncode == 0 and len(lines) == 2, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    first = render.pick(16, 12)
    assert ("primitive %d " % first["primitive_id"]) in lines[0] and lines[0].rstrip().replace(" (back face)", "").endswith(first["object_name"]), lines[0]
