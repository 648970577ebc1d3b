"""-m gpu: the layers above rt_scene_set_objects / rt_scene_pose: HIPPathTraceIntegrator::SetObjects / PoseObjects through rt::Render,
rth_render_set_objects / rth_render_pose and host.Render.set_objects() / .pose().  A plain Render and two tile Renders on one device give the image of the C-ABI
path (upload, rt_scene_refit of the restatement's triangles: tests/test_gpu_pose.py shows that this equals rt_scene_pose); a refusal arrives as the library's
message.  One process, each GPU step once; nothing here provokes a fault."""
import os
import numpy as np
import pytest
from raytracing_amd import capi, host
from tests.test_pose import IDENTITY, translation, rotation
from tests.test_gpu_pose import cornell_objects

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BOUNCES = 64, 64, 2, 4
MATS = np.stack([IDENTITY, translation(0.05, 0.02, -0.03), rotation((0, 1, 0), 0.02)])


def scene_of():
    s = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    return s


@pytest.mark.parametrize("tiles", [1, 2])
def test_render_pose_equals_the_c_abi_path(tiles):
    cam = host.default_camera(W, H)
    renders = [host.Render(W, H, scene_of(), tile_rank=r, tile_count=tiles) for r in range(tiles)]
    arrays = dict(renders[0].scene_arrays())
    tris = arrays["triangles"].copy()
    ids, n = cornell_objects(tris)
    got = []
    for r in renders:
        r.set_refittable(True)
        r.set_camera(cam); r.set_max_bounces(BOUNCES)
        r.set_objects(ids, n)
        assert "posed objects: %d objects" % n in r.tree_report()
        r.render_samples(1)
        r.pose(MATS)
        r.render_samples(SPP)
        assert r.sample_count() == SPP                                # the pose requested a reset
        got.append((r.radiance().copy(), r.stats()))
    c = capi.Context(0)
    try:
        c.set_refittable(True)
        c.upload_scene(arrays)
        c.refit_scene(capi.debug_pose(None, tris, ids, MATS))
        for rank in range(tiles):
            fr = capi.Frame(c, W, H, tile_rank=rank, tile_count=tiles)
            fr.set_camera(cam); fr.set_max_bounces(BOUNCES)
            fr.integrate(SPP)
            assert fr.radiance().tobytes() == got[rank][0].tobytes()
            st = fr.stats()
            assert (st.closest_rays, st.shadow_rays) == (got[rank][1].closest_rays, got[rank][1].shadow_rays)
            fr.close()
    finally:
        c.close()


def test_a_refusal_arrives_as_the_librarys_message():
    r = host.Render(W, H, scene_of())
    ids, n = cornell_objects(r.scene_arrays()["triangles"])
    with pytest.raises(host.RtError, match="rt_scene_set_objects: RT_CTX_OPT_REFITTABLE was off when the scene was uploaded"):
        r.set_objects(ids, n)
    r.set_refittable(True)
    with pytest.raises(host.RtError, match="rt_scene_pose: no objects"):
        r.pose(MATS)
    r.set_objects(ids, n)
    with pytest.raises(host.RtError, match="rt_scene_pose: the object count differs"):
        r.pose(MATS[:2])
    bad = MATS.copy()
    bad[2, 1, 1] = np.inf
    with pytest.raises(host.RtError, match="rt_scene_pose: a matrix entry is not finite"):
        r.pose(bad)
    r.pose(MATS)
    r.set_refittable(True)                                            # uploads again: the objects are dropped
    with pytest.raises(host.RtError, match="rt_scene_pose: no objects"):
        r.pose(MATS)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0                                # little-endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]  # PFM stores the bottom row first


def test_rt_render_lists_and_steps_objects(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "raytracing_amd", "rt_render")
    obj = os.path.join(ROOT, "assets", "CornellBox.obj")
    listed = subprocess.run([exe, "--scene", obj, "--list_objects", "1"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert listed.returncode == 0, listed.stderr
    assert listed.stdout.split() == ["0", "ceiling", "1", "backWall", "2", "rightWall", "3", "leftWall", "4", "tallBox", "5", "light", "6", "floor", "7", "shortBox"]
    out = str(tmp_path / "stepped.pfm")
    frames, steps = 3, {7: (0.02, 0.0, 0.01), 4: (0.0, -0.015, 0.0)}
    cmd = [exe, "-w", str(W), "-h", str(H), "--scene", obj, "--bounces", str(BOUNCES), "--frames", str(frames), "--out", out]
    for i, d in steps.items():
        cmd += ["--object_step", "%d,%r,%r,%r" % ((i,) + d)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "3 posed-object frames" in run.stdout, run.stdout
    # the same sequence driven from Python
    s = host.Scene(obj, objects=True)
    s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    r = host.Render(W, H, s)
    r.set_refittable(True)
    r.set_camera(host.default_camera(W, H)); r.set_max_bounces(BOUNCES)
    r.set_resolve_every_frame(True)
    r.set_objects(s.triangle_objects(), len(s.object_names()))
    for k in range(frames):
        mats = np.stack([IDENTITY] * 8)
        for i, d in steps.items():
            mats[i, :, 3] = np.float32(k) * np.array(d, np.float32)
        r.pose(mats)
        r.render_frame()
        assert r.sample_count() == 1
    assert read_pfm(out).tobytes() == r.resolved()[..., :3].tobytes()
    r.close()
