"""-m gpu: the temporal filter's history across a refit of moving geometry (RT_CTX_OPT_REFIT_MOTION).  The snapshot and
guide-motion kernels and the accumulation with motion images equal their host restatements bit for bit; a frame's refit-per-frame sequence equals the
host restatement fed with each call's inputs; the history survives the refits where it must and drops where it must; nothing else moves with the
option.  One process, each GPU step once, nothing retried; nothing here provokes a fault."""
import os
import numpy as np
import pytest

from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_refit import smooth
from tests.test_temporal_filter import random_case, guide_dirs, vec
from tests.test_gpu_temporal_filter import bits, same, tonemap, moving_cameras, check_fresh_history, tonemapped_mse, MAX_DIST
from tests.test_motion_filter import random_triangles, hits_of, moving_triangles, pose, stable_pixels, STEP, INVALID

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM_STEP = (0.005, 0.0, 0.0)       # tests/test_gpu_temporal_filter.py's camera step: a fifth of a pixel at the back wall, 128 x 128
DESC = dict(iterations=3, flags=capi.FILTER_DEMODULATE, alpha_color=0.2, alpha_moments=0.3, sigma_luminance=4.0, sigma_normal=0.1, sigma_depth=0.2)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def context(motion=True, refittable=True):
    c = capi.Context(0)
    if refittable:
        c.set_refittable(True)
    if motion is not None:
        c.set_refit_motion(motion)
    return c


# ---- 4. the kernels against the host restatement

@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (23, 41), (1080, 1920)])
def test_kernels_equal_host_restatement_bit_for_bit(ctx, shape):
    rng = np.random.default_rng(shape[0] + 13 * shape[1])
    H, W = shape
    tris = random_triangles(rng, 500)
    u = rng.uniform(0, 1, shape)
    v = rng.uniform(0, 1, shape) * (1 - u)
    prim = rng.integers(0, 500, shape).astype(np.uint32)
    prim[rng.random(shape) < 0.05] = INVALID
    hits = hits_of(u.astype(f32), v.astype(f32), prim)
    dev, ref = capi.debug_guide_motion(ctx, hits, tris), capi.debug_guide_motion(None, hits, tris)
    for d, r in zip(dev, ref):
        assert np.array_equal(bits(d), bits(r))
    assert (ref[0][..., 3] == (prim < 500)).all()

    args = list(random_case(rng, H, W))
    cam, dep, nrm = args[0], args[5], args[4]
    d = guide_dirs(cam, W, H)
    X = np.stack([f32(cam["position"][k]) + dep * d[i] for i, k in enumerate("xyz")], -1)
    prev_pos = np.zeros((H, W, 4), f32)
    moves = rng.random(shape) < 0.5
    prev_pos[..., :3] = X + np.where(moves[..., None], rng.normal(size=(H, W, 3)) * 0.02, 0.0)
    prev_pos[..., 3] = rng.random(shape) < 0.9                       # a tenth of the pixels know no motion
    prev_n = nrm.copy()
    turn = rng.random(shape) < 0.2
    prev_n[turn, :3] += rng.normal(size=(int(turn.sum()), 3)).astype(f32) * f32(0.3)
    prev_n[..., :3] /= np.maximum(np.linalg.norm(prev_n[..., :3], axis=-1, keepdims=True), 1e-6)
    prev_n[..., 3] = 0
    big = H > 100
    lengths = []
    for it in ((0, 5) if big else (0, 1, 4, 8)):
        for demod in (0, 1):
            for standing in (False, True):               # geometry moved under a moving and under a standing camera
                a = list(args)
                if standing:
                    a[1] = None
                desc = dict(iterations=it, flags=demod, alpha_color=float(rng.uniform(0.0, 0.5)), alpha_moments=float(rng.uniform(0.0, 0.5)),
                            sigma_luminance=float(rng.uniform(0.5, 8.0)), sigma_normal=float(rng.uniform(0.05, 1.0)),
                            sigma_depth=float(rng.uniform(0.05, 1.0)))
                dev = capi.debug_filter_temporal_motion(ctx, *a, prev_pos, prev_n, desc)
                ref = capi.debug_filter_temporal_motion(None, *a, prev_pos, prev_n, desc)
                for dd, r, what in zip(dev, ref, ("image", "colour history", "moments")):
                    assert np.array_equal(bits(dd), bits(r)), (it, demod, standing, what, int((bits(dd) != bits(r)).sum()))
                lengths.append(ref[2][..., 2])
    if shape == (23, 41):
        assert any((L > 1).sum() > 100 for L in lengths) and any((L == 1).sum() > 20 for L in lengths)      # hits and misses


# ---- 5 - 7. a frame's sequence: one refit, one reset, one sample, one filter call per frame

def run_sequence(c, scene, poses, cams, w, h, desc, bounces=4):
    """Uploads poses[0], refits to poses[1] BEFORE the first frame (so that every frame, the first included, has a kept pose to show its motion
    against) and to poses[k + 1] before frame k.  Per frame: (camera, hdr = radiance / spp, guides, guide_motion(), the history before, the
    output, the history after)."""
    first = dict(scene)
    first["triangles"] = poses[0]
    c.upload_scene(first)
    fr = capi.Frame(c, w, h)
    fr.set_max_bounces(bounces)
    rec = []
    for k, cam in enumerate(cams):
        c.refit_scene(poses[k + 1])
        fr.set_camera(cam)
        fr.reset()
        fr.integrate(1)
        hdr = fr.radiance() / f32(fr.sample_count())
        alb, nrm, dep, _ = fr.guides()
        ppos, pn = fr.guide_motion()
        before = fr.filter_history()
        out = fr.filter_temporal(desc)
        rec.append(dict(cam=cam, hdr=hdr, alb=alb, nrm=nrm, dep=dep, ppos=ppos, pn=pn, before=before, out=out, after=fr.filter_history()))
    fr.close()
    return rec


def check_replay(rec, desc, motion=True):
    """every frame's output and history from the host restatement fed with that frame's inputs, byte for byte"""
    prev = None
    for k, r in enumerate(rec):
        hc, hm = r["before"]
        if prev is None:
            want = capi.debug_filter_temporal_motion(None, r["cam"], None, r["hdr"], r["alb"], r["nrm"], r["dep"], r["nrm"], r["dep"], hc, np.zeros_like(hm),
                                                     None, None, desc)
        elif motion:
            want = capi.debug_filter_temporal_motion(None, r["cam"], prev["cam"], r["hdr"], r["alb"], r["nrm"], r["dep"], prev["nrm"], prev["dep"], hc, hm,
                                                     r["ppos"], r["pn"], desc)
        else:                                               # the history was dropped: as the first frame
            want = capi.debug_filter_temporal_motion(None, r["cam"], None, r["hdr"], r["alb"], r["nrm"], r["dep"], r["nrm"], r["dep"], hc, np.zeros_like(hm),
                                                     None, None, desc)
        assert same(r["out"], tonemap(want[0])), k
        assert np.array_equal(bits(r["after"][0]), bits(want[1])) and np.array_equal(bits(r["after"][1]), bits(want[2])), k
        prev = r


def cornell_poses(scene, n, step=STEP):
    tris = scene["triangles"]
    sel = moving_triangles(tris)
    assert sel.sum() > 0
    return [pose(tris, sel, k - 1, step) for k in range(n + 1)]


@pytest.mark.parametrize("camera", ["standing", "moving"])
def test_the_frame_equals_the_replay(golden_scenes, golden_radiance, camera):
    scene, cam = golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]
    n = 8
    cams = moving_cameras(cam, n, CAM_STEP if camera == "moving" else (0.0, 0.0, 0.0))
    c = context()
    try:
        rec = run_sequence(c, scene, cornell_poses(scene, n), cams, 64, 64, DESC)
        report = c.tree_report()
        assert "previous pose: RT_CTX_OPT_REFIT_MOTION keeps 96 bytes per triangle" in report
        assert "refit %d:" % n in report and "for the previous pose, 96 bytes per triangle" in report
    finally:
        c.close()
    check_replay(rec, DESC)
    L = rec[-1]["after"][1][..., 2]
    assert L.max() == n                                      # histories that lived through every refit
    assert (rec[-1]["ppos"][..., 3] == (rec[-1]["dep"] < MAX_DIST)).all()


def classes(rec, step):
    """per frame (valid, moving, normal): moving = the first hit lay more than |step| / 2 from where it lies now"""
    out = []
    half = 0.5 * float(np.linalg.norm(np.array(step, np.float64)))
    for r in rec:
        h, w = r["dep"].shape
        d = guide_dirs(r["cam"], w, h)
        X = np.stack([f32(r["cam"]["position"][k]) + r["dep"] * d[i] for i, k in enumerate("xyz")], -1).astype(np.float64)
        valid = (r["dep"] < MAX_DIST) & np.isfinite(r["hdr"][..., :3]).all(-1) & (r["ppos"][..., 3] != 0)
        moving = np.linalg.norm(X - r["ppos"][..., :3], axis=-1) > half
        out.append((valid, moving & valid, r["nrm"][..., :3].astype(np.float64)))
    return out


def test_the_history_survives_the_refits(golden_scenes, golden_radiance):
    """THE test that fails without the feature.  128 x 128, the short block moves STEP per frame, the camera stands, N = 8 frames.  On the stable
    pixels S (tests/test_motion_filter.py: stable_pixels; its numpy trace of the same sequence finds 0.875 of the image stable, 1318 pixels of them on
    the block) the history is N long after frame N -- static and moving pixels alike."""
    scene, cam = golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]
    n, w, h = 8, 128, 128
    cams = moving_cameras(cam, n, (0.0, 0.0, 0.0))
    poses = cornell_poses(scene, n)
    c = context()
    try:
        rec = run_sequence(c, scene, poses, cams, w, h, None)
    finally:
        c.close()
    cl = classes(rec, STEP)
    stable = stable_pixels(cl)
    moving = stable & cl[-1][1]
    print("stable pixels on the device's guides: %.3f of the image, %d of them on the moving block" % (stable.mean(), moving.sum()))
    assert stable.mean() >= 0.25 and moving.sum() > 0
    for k, r in enumerate(rec):
        L = r["after"][1][..., 2]
        short = stable & (L != k + 1)
        assert not short.any(), (k, int(short.sum()), np.argwhere(short)[:8].tolist(), L[short][:8].tolist())
    off = context(motion=False)
    try:
        rec_off = run_sequence(off, scene, poses, cams, w, h, None)
    finally:
        off.close()
    for r in rec_off:                                        # today's behaviour: every refit drops the history
        valid = (r["dep"] < MAX_DIST) & np.isfinite(r["hdr"][..., :3]).all(-1)
        L = r["after"][1][..., 2]
        assert (L[valid] == 1).all() and (L[~valid] == 0).all()
        assert (r["ppos"] == 0).all() and (r["pn"] == 0).all()


@pytest.fixture(scope="module")
def city():
    scene = host.Scene(arrays=S.city_block(40_000))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}


def test_a_deformation_not_only_a_rigid_move(city):
    n, w, h = 6, 96, 64
    cam = T.default_camera(w, h)
    poses = [smooth(city["triangles"], 0.001 * k, 0.5) for k in range(n + 1)]
    cams = [cam] * n
    share = {}
    for motion in (True, False):
        c = context(motion=motion)
        try:
            rec = run_sequence(c, city, poses, cams, w, h, DESC)
        finally:
            c.close()
        check_replay(rec, DESC, motion)
        hit = rec[-1]["dep"] < MAX_DIST
        share[motion] = float((rec[-1]["after"][1][..., 2][hit] == n).mean())
    print("deformation: %.3f of the first-hit pixels hold a history of %d after %d frames (option off: %.3f)" % (share[True], n, n, share[False]))
    assert share[True] > 0 and share[False] == 0


# ---- 8. where the history must still drop

def test_two_refits_an_upload_a_reset_and_the_option_off_give_a_fresh_history(golden_scenes, golden_radiance):
    scene, cam = golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]
    poses = cornell_poses(scene, 8)

    def shot(fr):
        fr.reset(); fr.integrate(1)
        return fr.filter_temporal()

    c = context()
    try:
        c.upload_scene(scene)
        fr = capi.Frame(c, 64, 64)
        fr.set_camera(cam); fr.set_max_bounces(4)
        assert (np.array(fr.guide_motion()) == 0).all()      # no refit yet: no pose kept
        shot(fr)
        c.refit_scene(poses[2]); shot(fr)
        assert fr.filter_history()[1][..., 2].max() == 2     # one refit: followed
        c.refit_scene(poses[3]); c.refit_scene(poses[4]); shot(fr)
        check_fresh_history(fr)                              # two refits: the kept pose is one deep
        c.refit_scene(poses[5]); shot(fr)
        assert fr.filter_history()[1][..., 2].max() == 2
        fr.filter_history_reset()
        c.refit_scene(poses[6]); shot(fr)
        check_fresh_history(fr)
        c.refit_scene(poses[7]); shot(fr)
        c.upload_scene(scene); shot(fr)
        check_fresh_history(fr)                              # an upload: another epoch (and no pose kept until its first refit)
        assert (np.array(fr.guide_motion()) == 0).all()
        shot(fr)
        assert fr.filter_history()[1][..., 2].max() == 2     # nothing moved: as ever
        fr.close()
    finally:
        c.close()
    # the option off, against a context that never heard of it: byte for byte, and fresh after every refit
    outs = []
    for motion in (False, None):
        c = context(motion=motion)
        try:
            c.upload_scene(scene)
            assert "previous pose" not in c.tree_report()
            fr = capi.Frame(c, 64, 64)
            fr.set_camera(cam); fr.set_max_bounces(4)
            seq = []
            for k in range(1, 4):
                c.refit_scene(poses[k])
                seq.append(shot(fr).tobytes())
                check_fresh_history(fr)
                seq += [a.tobytes() for a in fr.filter_history()]
            seq.append(shot(fr).tobytes())                   # and a standing step
            seq += [a.tobytes() for a in fr.filter_history()]
            assert "previous pose" not in c.tree_report()
            fr.close()
            outs.append(seq)
        finally:
            c.close()
    assert outs[0] == outs[1]
    # the option without RT_CTX_OPT_REFITTABLE: nothing kept, the refit refused as ever
    c = context(motion=True, refittable=False)
    try:
        c.upload_scene(scene)
        assert "previous pose" not in c.tree_report()
        with pytest.raises(capi.RtError, match="RT_CTX_OPT_REFITTABLE"):
            c.refit_scene(poses[2])
    finally:
        c.close()


# ---- 9. the refit's own results do not move with the option

def test_refit_results_are_untouched_by_the_option(golden_scenes, golden_radiance):
    scene, cam = golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]
    poses = cornell_poses(scene, 3)
    shots = []
    for motion in (True, False):
        c = context(motion=motion)
        try:
            c.upload_scene(scene)
            fr = capi.Frame(c, 96, 64)
            fr.set_camera(cam); fr.set_max_bounces(4)
            fr.integrate(2)
            c.refit_scene(poses[3])
            fr.reset(); fr.integrate(3)
            st = fr.stats()
            alb, nrm, dep, _ = fr.guides()
            shots.append((fr.radiance().tobytes(), fr.resolve().tobytes(), (st.closest_rays, st.shadow_rays), alb.tobytes(), nrm.tobytes(), dep.tobytes()))
            fr.close()
        finally:
            c.close()
    assert shots[0] == shots[1]


# ---- 10. quality

# Tone-mapped MSE against 1024 spp of the last pose at the last camera, 16 frames of 1 spp at 128 x 128, 4 bounces, the header's defaults; the short block
# moves along one of three paths and the camera moves CAM_STEP per frame.  (The camera moves because the random sampler's seed is a function of pixel and
# sample index alone: under a standing camera every reset frame repeats a static pixel's noise, and time adds nothing there with either setting.)
# Measured on an MI355X: QUALITY_MEASURED; the parent commit's rt_frame_filter_temporal over the same frames -- every refit drops
# its history -- gave the same figures as this build with the option off.
QUALITY_PATHS = {"along_x": (0.004, 0.0, 0.0), "along_y": (0.0, 0.004, 0.0), "up": (0.0, 0.0, 0.004)}
QUALITY_MEASURED = {"along_x": (1.2911e-03, 5.8745e-03, 0.2198), "along_y": (1.5883e-03, 5.9652e-03, 0.2663), "up": (1.2788e-03, 5.7994e-03, 0.2205)}
# (followed, dropped, ratio); the parent commit measured 5.8745e-03, 5.9652e-03, 5.7994e-03: the dropped column to every printed digit
QUALITY_BOUND = 0.633       # halfway between the largest measured ratio (0.2663) and 1: a filter that stopped following has ratio 1 by construction


def quality_sequence(c, scene, cam, step, n=16, w=128, h=128):
    tris = scene["triangles"]
    sel = moving_triangles(tris)
    poses = [pose(tris, sel, k, step) for k in range(n)]
    cams = moving_cameras(cam, n, CAM_STEP)
    first = dict(scene)
    first["triangles"] = poses[0]
    c.upload_scene(first)
    fr = capi.Frame(c, w, h)
    fr.set_max_bounces(4)
    for k in range(n):
        if k:
            c.refit_scene(poses[k])
        fr.set_camera(cams[k])
        fr.reset()
        fr.integrate(1)
        out = fr.filter_temporal()
    fr.reset()
    fr.integrate(1024)
    ref = fr.resolve()
    fr.close()
    return out, ref


@pytest.mark.parametrize("path", list(QUALITY_PATHS))
def test_quality_against_the_dropped_history(golden_scenes, golden_radiance, path):
    scene, cam = golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]
    res = {}
    for motion in (True, False):
        c = context(motion=motion)
        try:
            res[motion] = quality_sequence(c, scene, cam, QUALITY_PATHS[path])
        finally:
            c.close()
    assert res[True][1].tobytes() == res[False][1].tobytes()
    ref = res[True][1]
    ok = np.isfinite(ref).all(-1) & np.isfinite(res[True][0]).all(-1) & np.isfinite(res[False][0]).all(-1)
    on, off = tonemapped_mse(res[True][0], ref, ok), tonemapped_mse(res[False][0], ref, ok)
    print("quality %s: tone-mapped MSE against 1024 spp: followed %.4e, dropped %.4e, ratio %.4f" % (path, on, off, on / off))
    assert on < off
    assert on / off <= QUALITY_BOUND


# ---- the layers above the C-ABI

def test_render_set_refit_motion_equals_the_frame_sequence():
    """host.Render (HIPPathTraceIntegrator::SetRefitMotion, RefitGeometry, SetTemporalFilter): a refit requests the reset, the next resolve filters with
    the followed history -- the images a capi.Frame gives for the same refits, byte for byte; and the option is refused without set_refittable."""
    w, h, n = 96, 64, 5
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    render = host.Render(w, h, scene)
    render.set_max_bounces(4)
    with pytest.raises(RuntimeError, match="SetRefittable"):
        render.set_refit_motion()
    render.set_refittable()
    render.set_refit_motion()
    assert "previous pose" in render.tree_report()
    render.set_temporal_filter(DESC)
    cam = host.default_camera(w, h)
    render.set_camera(cam)
    arrays = render.scene_arrays()
    tris = np.array(arrays["triangles"])
    poses = [smooth(tris, 0.002 * k, 0.5) for k in range(n)]
    via_render = []
    for k in range(n):
        if k:
            render.refit(poses[k])
        render.render_samples(1)
        via_render.append(render.resolve_now())
    render.close() if hasattr(render, "close") else None
    c = context()
    try:
        c.upload_scene(arrays)
        fr = capi.Frame(c, w, h)
        fr.set_max_bounces(4); fr.set_camera(cam)
        for k in range(n):
            if k:
                c.refit_scene(poses[k])
            fr.reset(); fr.integrate(1)
            assert np.array_equal(bits(fr.filter_temporal(DESC)), bits(via_render[k])), k
        assert fr.filter_history()[1][..., 2].max() == n
        fr.close()
    finally:
        c.close()
