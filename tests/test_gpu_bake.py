"""-m gpu: occlusion bakes (rt_scene_bake / rt_scene_bake_buffer, raytracing_amd/csrc/bake.hip) on the device.

The contract: a bake's result is rt_debug_bake_reduce of the host restatement's rays (which tests/test_bake.py compares with numpy bit for bit) and the
reference's any-hit verdicts of those rays -- the CPU oracle's walk (tests/_oracle.py) -- exact in `unoccluded` and in the bytes of `bent_normal`, whichever tree
is walked and however the points are grouped into waves.  The points are first hits under the scene's camera with skipped points of every kind mixed in;
tests/test_bake.py::test_non_vacuity pins that the expected counts are neither all zero nor all full.  One process, each GPU step once, nothing retried;
nothing here provokes a fault."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T
from tests import _oracle
from tests.test_bake import BakeCase, bake_cases, back_faced, random_points, np_points, INVALID, RADIUS_FRACTION, BIAS_FRACTION, bounds_diagonal     # noqa: F401 (a fixture)
from tests.test_gpu_pose import city, scene_case          # noqa: F401 (city is a fixture)
from tests.test_gpu_query import context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(16, (1, 3, 4, 5, 65)), (64, (1, 2, 65)), (256, (1, 33)), (4096, (1,))]      # partial point groups in a wave; lane refill over 4 and 64 rays


def same(got, want, what=""):
    assert np.array_equal(got["unoccluded"], want["unoccluded"]), (what, got["unoccluded"][:8], want["unoccluded"][:8])
    assert got["bent_normal"].tobytes() == want["bent_normal"].tobytes(), what


def half_walked(want, n):
    walked = want["unoccluded"] != INVALID
    assert 2 * walked.sum() >= n, (int(walked.sum()), n)
    return walked


# ---- 1. the main comparison

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_bake_equals_reduced_oracle_verdicts(bake_cases, name):
    case = bake_cases[name]
    c = context()
    try:
        c.upload_scene(case.scene)
        partial = 0
        for samples, counts in SHAPES:
            for n in counts:
                pts = case.points(n)
                want = case.expected(pts, samples, seed=n)
                got = c.bake(pts, samples, seed=n, bias=case.bias, radius=case.radius)
                same(got, want, (name, samples, n))
                walked = half_walked(want, n)
                assert n < 3 or not walked.all()                           # skipped points are in the batch
                partial += int((walked & (want["unoccluded"] > 0) & (want["unoccluded"] < samples)).sum())
        assert partial > 0
    finally:
        c.close()


# ---- 2. ray generation on the device

def test_device_rays_equal_host_rays(bake_cases):
    case = bake_cases["cornell"]
    c = context()
    try:
        rng = np.random.default_rng(2)
        for samples, n, first in ((16, 67, 0), (64, 5, 0xFFFFFFFE), (256, 33, 1000), (4096, 3, 7)):
            pts = random_points(rng, n)
            assert capi.debug_bake_rays(c, pts, samples, 11, 0.25, 3.0, first_index=first).tobytes() == \
                   capi.debug_bake_rays(None, pts, samples, 11, 0.25, 3.0, first_index=first).tobytes(), (samples, n)
        s = back_faced(case.surfaces(65))                                  # hits, a third of them marked as met from behind
        assert capi.debug_bake_rays(c, s, 64, 1, case.bias, case.radius, from_surfaces=True).tobytes() == \
               capi.debug_bake_rays(None, s, 64, 1, case.bias, case.radius, from_surfaces=True).tobytes()
    finally:
        c.close()


# ---- 3. forms: buffers, surfaces, chunks

def test_buffers_from_surfaces_and_chunks(bake_cases):
    case = bake_cases["coverage"]
    c = context()
    try:
        c.upload_scene(case.scene)
        n, samples = 257, 64
        rays = case.mixed_rays(n, 77)                                      # (tests/test_bake.py pins that their first hits hold miss records)
        b_rays, b_surf, b_out = c.create_buffer(rays), c.create_buffer(np.zeros(n, T.surface)), c.create_buffer(np.zeros(n, T.bake_result))
        c.trace_buffer(b_rays, n, surfaces=b_surf)
        c.bake_buffer(b_surf, n, b_out, samples, seed=3, bias=case.bias, radius=case.radius, from_surfaces=True)     # no trip to the host in between
        got = b_out.read(T.bake_result, n)
        surf = b_surf.read(T.surface, n)
        want = case.expected(surf, samples, seed=3, from_surfaces=True)
        same(got, want, "buffers")
        half_walked(want, n)
        miss = surf["primitive_id"] == INVALID
        assert miss.any() and (got["unoccluded"][miss] == INVALID).all()   # miss records are among them, and are skipped
        same(c.bake(surf, samples, seed=3, bias=case.bias, radius=case.radius, from_surfaces=True), got, "host arrays, surfaces")
        flipped = back_faced(surf)                                         # the walk culls back faces, so no traced record has the bit: the caller's own
        assert (flipped["flags"] & 2).any() and not (surf["flags"] & 2).any()
        want_flipped = case.expected(flipped, samples, seed=3, from_surfaces=True)
        same(c.bake(flipped, samples, seed=3, bias=case.bias, radius=case.radius, from_surfaces=True), want_flipped, "host arrays, back faces")
        b_surf.write(flipped)
        c.bake_buffer(b_surf, n, b_out, samples, seed=3, bias=case.bias, radius=case.radius, from_surfaces=True)
        same(b_out.read(T.bake_result, n), want_flipped, "buffers, back faces")
        assert not np.array_equal(want_flipped["unoccluded"], want["unoccluded"])
        pos, nrm, ok = np_points(surf, True)
        rows = np.zeros((n, 8), f32)
        rows[:, 0:3], rows[:, 4:7] = pos, np.where(ok[:, None], nrm, f32(0.0))
        whole = c.bake(rows, samples, seed=3, bias=case.bias, radius=case.radius)
        same(whole, got, "point rows")
        b_rows = c.create_buffer(rows)
        c.bake_buffer(b_rows, n, b_out, samples, seed=3, bias=case.bias, radius=case.radius)
        same(b_out.read(T.bake_result, n), got, "buffers, point rows")
        c.set_bake_chunk_points(50)                                        # six chunks: each carries the index of its first point
        same(c.bake(rows, samples, seed=3, bias=case.bias, radius=case.radius), whole, "chunked")
        c.set_bake_chunk_points(0)
        assert "of that the bakes'" in c.tree_report()
        assert len(c.bake(rows[:0], samples)) == 0                          # n == 0
        for b in (b_rays, b_surf, b_out, b_rows):
            b.close()
    finally:
        c.close()


# ---- 4. moving geometry

def test_bake_follows_pose(bake_cases, golden_scenes, city):
    case = bake_cases["cornell"]
    sc, ids, n_objects, mats = scene_case("cornell", golden_scenes, city)
    c = context(refittable=True)
    try:
        c.upload_scene(sc)
        c.set_objects(ids, n_objects)
        c.pose_scene(mats)
        posed = capi.debug_pose(None, sc["triangles"], ids, mats)
        nodes, _, _ = capi.debug_refit(None, sc["nodes"], posed)
        moved = dict(sc); moved["triangles"] = posed; moved["nodes"] = nodes
        after = BakeCase("cornell", moved, case.cam)
        pts = after.points(65)
        want = after.expected(pts, 64, seed=1)
        same(c.bake(pts, 64, seed=1, bias=after.bias, radius=after.radius), want, "posed")
        half_walked(want, 65)
        before = case.expected(pts, 64, seed=1)
        assert not np.array_equal(before["unoccluded"], want["unoccluded"])       # (the pose did move what the rays meet)
    finally:
        c.close()


# ---- 5. whichever tree is walked

@pytest.mark.parametrize("how", ["wide_trees_off", "shared_tree", "adapted_fold"])
def test_every_tree_gives_the_same_result(bake_cases, how):
    case = bake_cases["city"]
    c = context(wide=0) if how == "wide_trees_off" else context(shadow_tree=0) if how == "shared_tree" else context(adaptive=capi.ADAPTIVE_FOLD_DEFAULT | 2 | 4)
    try:
        c.upload_scene(case.scene)
        if how == "adapted_fold":
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(case.cam); fr.set_max_bounces(3)
            fr.integrate(1)
            report = c.tree_report()
            assert "adaptive fold" in report and "(adopted)" in report.split("adaptive fold")[-1], report
            fr.close()
        for samples, n in ((16, 65), (256, 33)):
            pts = case.points(n)
            same(c.bake(pts, samples, seed=n, bias=case.bias, radius=case.radius), case.expected(pts, samples, seed=n), (how, samples))
    finally:
        c.close()


# ---- 6. frames are undisturbed

def test_frames_are_undisturbed(bake_cases):
    case = bake_cases["cornell"]
    pts = case.points(65)
    c = context(adaptive=0)                                                # (no fold adopted at a moment of its own choosing: both runs walk the same records)
    try:
        c.upload_scene(case.scene)

        def run(disturb):
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(case.cam); fr.set_max_bounces(4)
            fr.integrate(1)
            if disturb:
                c.bake(pts, 64, bias=case.bias, radius=case.radius)
            fr.integrate(1)
            st = fr.stats()
            out = (fr.radiance().tobytes(), bytes(st))
            fr.close()
            return out

        a, b = run(False), run(True)
        assert a[0] == b[0] and a[1] == b[1]
    finally:
        c.close()


# ---- 7. refusals

def test_refusals_launch_nothing_and_leave_bakes_working(bake_cases):
    import ctypes as C
    case = bake_cases["cornell"]
    n, samples = 65, 16
    pts = case.points(n)
    want = case.expected(pts, samples)
    lib = capi.load()
    c, other = context(), context()
    try:
        out = np.zeros(n, T.bake_result)
        p = lambda a: a.ctypes.data
        d = lambda **kw: C.byref(capi.bake_desc(**dict(dict(samples=samples, bias=case.bias, radius=case.radius), **kw)))

        def refused(rc, text):
            assert rc != 0 and text in lib.rt_last_error(c.handle).decode(), (rc, lib.rt_last_error(c.handle).decode())

        refused(lib.rt_scene_bake(c.handle, p(pts), n, d(), p(out)), "no scene")
        c.upload_scene(case.scene)
        other.upload_scene(case.scene)
        works = lambda: same(c.bake(pts, samples, bias=case.bias, radius=case.radius), want, "after a refusal")
        refused(lib.rt_scene_bake(c.handle, None, n, d(), p(out)), "points is NULL"); works()
        refused(lib.rt_scene_bake(c.handle, p(pts), n, None, p(out)), "desc is NULL")
        refused(lib.rt_scene_bake(c.handle, p(pts), n, d(), None), "out is NULL")
        for kw, text in ((dict(samples=0), "power of two"), (dict(samples=8), "power of two"), (dict(samples=24), "power of two"), (dict(samples=8192), "power of two"),
                         (dict(bias=np.nan), "bias"), (dict(bias=-np.inf), "bias"), (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"),
                         (dict(radius=np.inf), "radius"), (dict(radius=np.nan), "radius"), (dict(flags=2), "unknown flag")):
            refused(lib.rt_scene_bake(c.handle, p(pts), n, d(**kw), p(out)), text)
        works()
        assert out.tobytes() == bytes(out.nbytes)                           # nothing was written by any of them
        assert lib.rt_scene_bake(c.handle, None, 0, None, None) == 0        # n == 0: RT_OK, nothing done
        b_pts, b_out, b_small, b_alien = c.create_buffer(pts), c.create_buffer(out), c.create_buffer(out[:-1]), other.create_buffer(out)
        refused(lib.rt_scene_bake_buffer(c.handle, b_pts.handle, n, d(), b_small.handle), "the out buffer is smaller than n")
        refused(lib.rt_scene_bake_buffer(c.handle, b_pts.handle, n + 1, d(), b_out.handle), "the points buffer is smaller than n")
        refused(lib.rt_scene_bake_buffer(c.handle, b_pts.handle, n, d(flags=1), b_out.handle), "the points buffer is smaller than n")      # surfaces are 64 bytes each
        refused(lib.rt_scene_bake_buffer(c.handle, b_pts.handle, n, d(), b_alien.handle), "another context")
        refused(lib.rt_scene_bake_buffer(c.handle, None, n, d(), b_out.handle), "points is NULL")
        refused(lib.rt_scene_bake_buffer(c.handle, b_pts.handle, n, d(), None), "out is NULL")
        assert b_out.read(T.bake_result, n).tobytes() == bytes(out.nbytes) and b_small.read(T.bake_result, n - 1).tobytes() == bytes(16 * (n - 1))
        works()
        for b in (b_pts, b_out, b_small, b_alien):
            b.close()
    finally:
        c.close(); other.close()


# ---- 8. layers

def test_layers_occlusion_image_equals_pick_then_bake(tmp_path):
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    w = h = 16
    render = host.Render(w, h, scene)
    render.set_camera(host.default_camera(w, h)); render.set_max_bounces(4)
    diag = bounds_diagonal(render.scene_arrays())
    samples, radius, bias = 64, float(f32(0.25 * diag)), float(f32(BIAS_FRACTION * diag))
    img = render.occlusion_image(samples, radius, bias=bias, seed=5)
    assert img.shape == (h, w) and img.dtype == f32
    picks = [render.pick(x, y) for y in range(h) for x in range(w)]
    surf = np.zeros(w * h, T.surface)
    for i, pk in enumerate(picks):
        for k in T.surface.names:
            surf[i][k] = pk[k] if k != "object" else INVALID
    got = render.bake(surf, samples, seed=5, bias=bias, radius=radius, from_surfaces=True)
    want = np.where(got["unoccluded"] == INVALID, f32(1.0), got["unoccluded"].astype(f32) / f32(samples)).astype(f32)
    assert img.tobytes() == want.reshape(h, w).tobytes()
    miss = surf["primitive_id"] == INVALID
    assert (want[miss] == 1).all() and ((want > 0) & (want < 1)).sum() * 4 >= (~miss).sum() and (~miss).sum() * 2 >= w * h
    rows = np.zeros((w * h, 8), f32)
    pos, nrm, ok = np_points(surf, True)
    rows[:, 0:3], rows[:, 4:7] = pos, np.where(ok[:, None], nrm, f32(0.0))
    assert render.bake(rows, samples, seed=5, bias=bias, radius=radius).tobytes() == got.tobytes()
    # rt_render --ao writes that image (bottom row first, grey)
    out = tmp_path / "ao.pfm"
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", str(w), "-h", str(h), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--ao", str(out), "--ao_samples", str(samples), "--ao_radius", repr(radius), "--ao_bias", repr(bias)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ambient occlusion" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    raw = out.read_bytes()
    head = ("PF\n%d %d\n-1.0\n" % (w, h)).encode()
    assert raw.startswith(head)
    pfm = np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1]
    seed0 = render.occlusion_image(samples, radius, bias=bias, seed=0)
    assert (pfm[:, :, 0] == pfm[:, :, 1]).all() and pfm[:, :, 0].tobytes() == seed0.tobytes()
