"""-m gpu: light bakes (rt_scene_light_bake / rt_scene_light_bake_buffer / rt_scene_atlas_bake_light, raytracing_amd/csrc/light_bake.hip)
on the device.

The contract: a light bake's result is rt_debug_light_bake_reduce of the host restatement's items (which tests/test_light_bake.py compares with numpy bit for
bit) and any-hit verdicts of their rays, byte for byte, whichever tree is walked and however the points are grouped into waves.  The scenes are the golden
Cornell and coverage scenes with scenes.make_lights' lights (a directional one, a point light inside, one behind the walls, one on a baked point) and
gradient_env; tests/test_light_bake.py::test_non_vacuity pins with the CPU walk that the verdicts are not all alike.  One process, each GPU step once,
nothing retried; nothing here provokes a fault."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes, types as T
from tests.test_bake import bake_cases, back_faced, random_points, np_points, INVALID, BakeCase     # noqa: F401 (a fixture)
from tests.test_light_bake import LightCase, GPU_SHAPES, GPU_LIGHTS, random_lights
from tests.test_gpu_pose import city, scene_case          # noqa: F401 (city is a fixture)
from tests.test_gpu_query import context

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def same(got, want, what=""):
    for k in T.light_bake_result.names:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:4], want[k][:4])


def device_expected(c, case, points, samples, **kw):
    """rt_debug_light_bake_reduce of the host's rays and of Context.trace(ANY_HIT)'s verdicts for them"""
    kw = dict(dict(bias=case.bias, sky_distance=case.sky_distance), **kw)
    rays = capi.debug_light_bake_rays(None, points, samples, case.lights, **kw)
    occ = c.trace(rays.reshape(-1), any_hit=True).reshape(rays.shape)
    return capi.debug_light_bake_reduce(points, samples, occ, case.lights, case.env, **kw), rays


def bake(c, case, points, samples, **kw):
    return c.bake_light(points, samples, **dict(dict(bias=case.bias, sky_distance=case.sky_distance), **kw))


# ---- 1. parity, 2. rays

@pytest.mark.parametrize("M", GPU_LIGHTS)
@pytest.mark.parametrize("name", ["cornell", "coverage"])
def test_light_bake_equals_reduced_verdicts(bake_cases, name, M):
    c = context()
    try:
        partial = lit = 0
        uploaded = None
        for samples, counts in GPU_SHAPES:
            for n in counts:
                case = LightCase(bake_cases[name], M, n)
                if uploaded is None or uploaded.tobytes() != case.lights.tobytes():     # (the coincident light follows the batch's first walked point)
                    c.upload_scene(case.scene)
                    uploaded = case.lights
                want, rays = device_expected(c, case, case.pts, samples, seed=n)
                cpu, _ = case.expected(case.pts, samples, seed=n)
                same(want, cpu, ("device verdicts against the CPU walk's", name, M, samples, n))
                same(bake(c, case, case.pts, samples, seed=n), want, (name, M, samples, n))
                assert capi.debug_light_bake_rays(c, case.pts, samples, case.lights, seed=n, bias=case.bias, sky_distance=case.sky_distance).tobytes() == rays.tobytes()
                walked = want["sky_unoccluded"] != INVALID
                if samples == 16 and n >= 7:                                   # a skipped point between two walked ones of the same wave (four points per wave)
                    assert any(not walked[i] and walked[i - 1] and walked[i + 1] and (i - 1) // 4 == (i + 1) // 4 for i in range(1, n - 1)), walked
                partial += int((walked & (want["sky_unoccluded"] > 0) & (want["sky_unoccluded"] < samples)).sum())
                lit += int(want["lights_unshadowed"][walked].sum())
                for kw in (dict(sky=False), dict(lights=False)):
                    hw = dict(sky=kw.get("sky", True), use_lights=kw.get("lights", True))
                    same(bake(c, case, case.pts, samples, seed=n, **kw), device_expected(c, case, case.pts, samples, seed=n, **hw)[0], (name, M, samples, n, kw))
        assert partial > 0 and (M == 0 or lit > 0)
    finally:
        c.close()


def test_device_rays_equal_host_rays(bake_cases):
    case = bake_cases["cornell"]
    c = context()
    try:
        rng = np.random.default_rng(2)
        for samples, n, first, M in ((16, 67, 0, 3), (64, 5, 0xFFFFFFFE, 70), (256, 33, 1000, 0), (4096, 3, 7, 1)):
            pts, lg = random_points(rng, n), random_lights(rng, M)
            for kw in (dict(), dict(sky=False), dict(use_lights=False)):
                kw = dict(kw, seed=11, bias=0.25, sky_distance=3.0, first_index=first)
                assert capi.debug_light_bake_rays(c, pts, samples, lg, **kw).tobytes() == capi.debug_light_bake_rays(None, pts, samples, lg, **kw).tobytes(), (samples, n, M)
        s = back_faced(case.surfaces(65))
        lg = random_lights(rng, 5)
        kw = dict(seed=1, bias=case.bias, sky_distance=case.radius, from_surfaces=True)
        assert capi.debug_light_bake_rays(c, s, 64, lg, **kw).tobytes() == capi.debug_light_bake_rays(None, s, 64, lg, **kw).tobytes()
    finally:
        c.close()


# ---- 3. forms: buffers, surfaces, chunks

def test_buffers_from_surfaces_and_chunks(bake_cases):
    base = bake_cases["coverage"]
    case = LightCase(base, 3, 65)
    c = context()
    try:
        c.upload_scene(case.scene)
        n, samples = 65, 64
        rays = base.mixed_rays(n, 77)                                      # (tests/test_bake.py pins that their first hits hold miss records)
        b_rays, b_surf, b_out = c.create_buffer(rays), c.create_buffer(np.zeros(n, T.surface)), c.create_buffer(np.zeros(n, T.light_bake_result))
        c.trace_buffer(b_rays, n, surfaces=b_surf)
        c.bake_light_buffer(b_surf, n, b_out, samples, seed=3, bias=case.bias, sky_distance=case.sky_distance, from_surfaces=True)     # no trip to the host in between
        got = b_out.read(T.light_bake_result, n)
        surf = b_surf.read(T.surface, n)
        want, _ = device_expected(c, case, surf, samples, seed=3, from_surfaces=True)
        same(got, want, "buffers")
        miss = surf["primitive_id"] == INVALID
        assert miss.any() and not miss.all() and (got["sky_unoccluded"][miss] == INVALID).all() and (got["lights_unshadowed"][miss] == INVALID).all()
        same(bake(c, case, surf, samples, seed=3, from_surfaces=True), got, "host arrays, surfaces")
        flipped = back_faced(surf)
        same(bake(c, case, flipped, samples, seed=3, from_surfaces=True), device_expected(c, case, flipped, samples, seed=3, from_surfaces=True)[0], "back faces")
        pos, nrm, ok = np_points(surf, True)
        rows = np.zeros((n, 8), f32)
        rows[:, 0:3], rows[:, 4:7] = pos, np.where(ok[:, None], nrm, f32(0.0))
        whole = bake(c, case, rows, samples, seed=3)
        same(whole, got, "point rows")
        c.set_bake_chunk_points(3)                                         # 22 chunks: each carries the index of its first point
        same(bake(c, case, rows, samples, seed=3), whole, "chunked")
        c.set_bake_chunk_points(0)
        assert len(bake(c, case, rows[:0], samples)) == 0                  # n == 0
        for b in (b_rays, b_surf, b_out):
            b.close()
    finally:
        c.close()


# ---- 4. whichever tree is walked

@pytest.mark.parametrize("how", ["wide_trees_off", "shared_tree", "adapted_fold"])
def test_every_tree_gives_the_same_result(bake_cases, how):
    base = bake_cases["coverage"]
    c = context(wide=0) if how == "wide_trees_off" else context(shadow_tree=0) if how == "shared_tree" else context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)
    try:
        uploaded = None
        for samples, n in ((16, 33), (256, 9)):
            case = LightCase(base, 3, n)
            if uploaded is None or uploaded.tobytes() != case.lights.tobytes():
                c.upload_scene(case.scene)
                uploaded = case.lights
                if how == "adapted_fold":
                    fr = capi.Frame(c, 64, 64)
                    fr.set_camera(base.cam); fr.set_max_bounces(3)
                    fr.integrate(1)
                    report = c.tree_report()
                    assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report
                    fr.close()
            same(bake(c, case, case.pts, samples, seed=n), case.expected(case.pts, samples, seed=n)[0], (how, samples))
    finally:
        c.close()


# ---- 5. moving geometry

def test_light_bake_follows_pose(bake_cases, golden_scenes, city):
    sc, ids, n_objects, mats = scene_case("cornell", golden_scenes, city)
    posed = capi.debug_pose(None, sc["triangles"], ids, mats)
    nodes, _, _ = capi.debug_refit(None, sc["nodes"], posed)
    moved = dict(sc); moved["triangles"] = posed; moved["nodes"] = nodes
    after = LightCase(BakeCase("cornell", moved, bake_cases["cornell"].cam), 3, 33)
    c, fresh = context(refittable=True), context()
    try:
        rest = dict(sc); rest["lights"] = after.lights; rest["env"] = after.env
        c.upload_scene(rest)
        before = bake(c, after, after.pts, 64, seed=1)
        c.set_objects(ids, n_objects)
        c.pose_scene(mats)
        fresh.upload_scene(after.scene)
        got = bake(c, after, after.pts, 64, seed=1)
        same(got, bake(fresh, after, after.pts, 64, seed=1), "posed against a fresh upload of the posed triangles")
        same(got, after.expected(after.pts, 64, seed=1)[0], "posed against the CPU walk")
        assert before.tobytes() != got.tobytes()                           # (the pose did move what the rays meet)
    finally:
        c.close(); fresh.close()


# ---- 6. the atlas

def test_atlas_light_bake_equals_bake_of_its_surfaces(bake_cases):
    base = bake_cases["cornell"]
    case = LightCase(base, 3, 33)
    c = context()
    try:
        c.upload_scene(case.scene)
        w = h = 16
        uv = scenes.synthetic_atlas(case.scene["triangles"], w, h) * f32(0.75)           # (the charts leave a margin: uncovered texels)
        kw = dict(seed=4, bias=case.bias, sky_distance=case.sky_distance)
        got, texels, stats = c.bake_light_atlas(w, h, 64, uv=uv, **kw)
        tx, _ = c.atlas(w, h, uv=uv)
        assert texels.tobytes() == tx.tobytes()
        surf = c.atlas_surfaces(tx)
        same(got, c.bake_light(surf, 64, from_surfaces=True, **kw), "atlas")
        same(got, device_expected(c, case, surf, 64, seed=4, from_surfaces=True)[0], "atlas against the host's reduction")
        uncovered = tx["primitive_id"] == INVALID
        assert uncovered.any() and not uncovered.all() and stats["covered"] == (~uncovered).sum()
        assert (got["sky_unoccluded"][uncovered] == INVALID).all() and (got["lights_unshadowed"][uncovered] == INVALID).all() and not got["sky"][uncovered].any()
        ao, _, _ = c.bake_atlas(w, h, 64, seed=4, bias=case.bias, radius=case.sky_distance, uv=uv)
        assert np.array_equal(ao["unoccluded"], got["sky_unoccluded"])
        c.set_bake_chunk_points(50)
        same(c.bake_light_atlas(w, h, 64, uv=uv, **kw)[0], got, "chunked atlas")
        with pytest.raises(capi.RtError, match="flags must be 0"):
            c.bake_light_atlas(w, h, 64, uv=uv, flags=capi.LIGHT_BAKE_NO_SKY, **kw)
        same(c.bake_light_atlas(w, h, 64, uv=uv, **kw)[0], got, "after a refusal")
    finally:
        c.close()


# ---- 7. nothing else moves

def test_frames_and_occlusion_bakes_are_undisturbed(bake_cases):
    base = bake_cases["cornell"]
    case = LightCase(base, 3, 33)
    c = context(adaptive=0)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(base.cam); fr.set_max_bounces(4)
            fr.integrate(1)
            ao = [c.bake(case.pts, 64, bias=case.bias, radius=base.radius)]
            if disturb:
                bake(c, case, case.pts, 64)
            ao.append(c.bake(case.pts, 64, bias=case.bias, radius=base.radius))
            fr.integrate(1)
            out = (fr.radiance().tobytes(), bytes(fr.stats()), ao[0].tobytes(), ao[1].tobytes())
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a == b and a[2] == a[3]
    finally:
        c.close()


# ---- 8. refusals

def test_refusals_launch_nothing_and_leave_bakes_working(bake_cases):
    case = LightCase(bake_cases["cornell"], 3, 33)
    n, samples, pts = 33, 16, case.pts
    lib = capi.load()
    c, other = context(), context()
    try:
        out = np.zeros(n, T.light_bake_result)
        p = lambda a: a.ctypes.data
        d = lambda **kw: C.byref(capi.light_bake_desc(**dict(dict(samples=samples, bias=case.bias, sky_distance=case.sky_distance), **kw)))

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(c.handle).decode(), (rc, lib.rt_last_error(c.handle).decode())

        refused(lib.rt_scene_light_bake(c.handle, p(pts), n, d(), p(out)), "no scene")
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)
        want = case.expected(pts, samples)[0]
        works = lambda: same(bake(c, case, pts, samples), want, "after a refusal")
        refused(lib.rt_scene_light_bake(c.handle, None, n, d(), p(out)), "points is NULL"); works()
        refused(lib.rt_scene_light_bake(c.handle, p(pts), n, None, p(out)), "desc is NULL")
        refused(lib.rt_scene_light_bake(c.handle, p(pts), n, d(), None), "out is NULL")
        for kw, text in ((dict(samples=0), "power of two"), (dict(samples=8), "power of two"), (dict(samples=24), "power of two"), (dict(samples=8192), "power of two"),
                         (dict(bias=np.nan), "bias"), (dict(bias=-np.inf), "bias"), (dict(sky_distance=0.0), "sky_distance"), (dict(sky_distance=-1.0), "sky_distance"),
                         (dict(sky_distance=np.inf), "sky_distance"), (dict(sky_distance=np.nan), "sky_distance"), (dict(flags=8), "unknown flag")):
            refused(lib.rt_scene_light_bake(c.handle, p(pts), n, d(**kw), p(out)), text)
        works()
        atlas = capi.atlas_desc(8, 8)
        refused(lib.rt_scene_atlas_bake_light(c.handle, C.byref(atlas), None, d(flags=1), p(out), None, None), "flags must be 0")
        refused(lib.rt_scene_atlas_bake_light(c.handle, C.byref(atlas), None, d(samples=3), p(out), None, None), "power of two")
        refused(lib.rt_scene_atlas_bake_light(c.handle, C.byref(atlas), None, None, p(out), None, None), "desc is NULL")
        refused(lib.rt_scene_atlas_bake_light(c.handle, C.byref(atlas), None, d(), None, None, None), "out is NULL")
        refused(lib.rt_scene_atlas_bake_light(c.handle, C.byref(capi.atlas_desc(0, 8)), None, d(), p(out), None, None), "")
        assert out.tobytes() == bytes(out.nbytes)                           # nothing was written by any of them
        assert lib.rt_scene_light_bake(c.handle, None, 0, None, None) == 0  # n == 0: RT_OK, nothing done
        b_pts, b_out, b_small, b_alien = c.create_buffer(pts), c.create_buffer(out), c.create_buffer(out[:-1]), other.create_buffer(out)
        refused(lib.rt_scene_light_bake_buffer(c.handle, b_pts.handle, n, d(), b_small.handle), "the out buffer is smaller than n")
        refused(lib.rt_scene_light_bake_buffer(c.handle, b_pts.handle, n + 1, d(), b_out.handle), "the points buffer is smaller than n")
        refused(lib.rt_scene_light_bake_buffer(c.handle, b_pts.handle, n, d(flags=1), b_out.handle), "the points buffer is smaller than n")      # surfaces are 64 bytes each
        refused(lib.rt_scene_light_bake_buffer(c.handle, b_pts.handle, n, d(), b_alien.handle), "another context")
        refused(lib.rt_scene_light_bake_buffer(c.handle, None, n, d(), b_out.handle), "points is NULL")
        refused(lib.rt_scene_light_bake_buffer(c.handle, b_pts.handle, n, d(), None), "out is NULL")
        assert b_out.read(T.light_bake_result, n).tobytes() == bytes(out.nbytes)
        works()
        for b in (b_pts, b_out, b_small, b_alien):
            b.close()
    finally:
        c.close(); other.close()


# ---- 9. layers

def test_layers_irradiance_atlas_equals_the_capi_path(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = host.Scene(os.path.join(root, "assets", "CornellBox.obj"))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    w = h = 16
    render = host.Render(w, h, scene)
    render.set_camera(host.default_camera(w, h)); render.set_max_bounces(4)
    arrays = render.scene_arrays()
    uv = scenes.synthetic_atlas(arrays["triangles"], w, h) * f32(0.75)
    samples, bias, dist = 64, 1e-3, 2.5
    img, stats = render.irradiance_atlas(w, h, samples, sky_distance=dist, bias=bias, seed=5, uv=uv)
    assert img.shape == (h, w, 3) and img.dtype == f32
    c = context()
    try:
        c.upload_scene({k: v for k, v in arrays.items()})
        got, texels, cstats = c.bake_light_atlas(w, h, samples, seed=5, bias=bias, sky_distance=dist, uv=uv)
        assert bytes(stats) == bytes(cstats)
        covered = got["sky_unoccluded"] != INVALID
        want = np.where(covered[:, None], got["sky"] + got["lights"], f32(np.nan)).astype(f32).reshape(h, w, 3)
        assert img.tobytes() == want.tobytes()
        assert covered.any() and not covered.all() and np.isnan(img[~covered.reshape(h, w)]).all()
        assert (got["lights_unshadowed"][covered] > 0).any() and (got["lights"][covered] > 0).any() and (got["sky"][covered] > 0).any()
        # the point form and the image: every pixel picked, then baked
        surf = c.atlas_surfaces(texels)
        assert render.bake_light(surf, samples, seed=5, bias=bias, sky_distance=dist, from_surfaces=True).tobytes() == got.tobytes()
        for kw in (dict(sky=False), dict(lights=False)):
            assert render.bake_light(surf, samples, seed=5, bias=bias, sky_distance=dist, from_surfaces=True, **kw).tobytes() == \
                   c.bake_light(surf, samples, seed=5, bias=bias, sky_distance=dist, from_surfaces=True, **kw).tobytes()
        picture = render.irradiance_image(samples, sky_distance=dist, bias=bias, seed=5)
        assert picture.shape == (h, w, 3)
        picks = np.zeros(w * h, T.surface)
        for i, pk in enumerate(render.pick(x, y) for y in range(h) for x in range(w)):
            for k in T.surface.names:
                picks[i][k] = pk[k] if k != "object" else INVALID
        baked = c.bake_light(picks, samples, seed=5, bias=bias, sky_distance=dist, from_surfaces=True)
        assert picture.tobytes() == (baked["sky"] + baked["lights"]).astype(f32).reshape(h, w, 3).tobytes()
        assert (picture > 0).any()
    finally:
        c.close()
    # rt_render --lightmap writes that atlas (row 0 = v 0 first; seed 0, the bias and sky distance of the command line)
    out = tmp_path / "lightmap.pfm"
    r = subprocess.run([os.path.join(root, "raytracing_amd", "rt_render"), "-w", str(w), "-h", str(h), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--lightmap", str(out), "--atlas_size", "%d,%d" % (w, h), "--atlas_uv", "synthetic", "--ao_samples", str(samples)], cwd=root, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "lightmap" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    raw = out.read_bytes()
    head = ("PF\n%d %d\n-1.0\n" % (w, h)).encode()
    assert raw.startswith(head)
    pfm = np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)
    cli = render.irradiance_atlas(w, h, samples, uv=scenes.synthetic_atlas(arrays["triangles"], w, h))[0]      # the command line's defaults: seed 0, bias 1e-3
    assert pfm.tobytes() == cli.tobytes() and np.isfinite(pfm).any()
