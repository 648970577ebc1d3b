"""-m gpu: the layers above rt_scene_set_morph / rt_scene_morph / rt_scene_morph_skin on one small scene: host.Render.set_morph() /
.morph() / .morph_skin(), HIPPathTraceIntegrator::SetMorph / MorphTargets / MorphAndSkin through rth_render_*, and capi.Context.set_morph() / morph_scene() /
morph_skin_scene().  All give the same image bits as the refit of the restatement's triangles, each raises the library's message on a wrong target count, and
the tree report keeps its line.  One process, each GPU step once; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_gpu_skin_layers import scene_of, shot, W, H, SPP, BOUNCES, BONES

pytestmark = pytest.mark.gpu
f32 = np.float32
TARGETS = 4


def test_the_layers_give_the_same_images_and_the_report_keeps_its_line(golden_scenes):
    cam = host.default_camera(W, H)
    r1 = host.Render(W, H, scene_of(golden_scenes, True))
    r1.set_refittable(True)
    r1.set_camera(cam); r1.set_max_bounces(BOUNCES)
    arrays = dict(r1.scene_arrays())
    tris = arrays["triangles"].copy()
    infl = r1.scene.triangle_skin()
    deltas, offsets = T.morph_targets(S.synthetic_morph(tris, TARGETS, radius=0.25, amplitude=0.04))     # the BVH order of scene_arrays()['triangles']
    w = np.array([0.9, -0.5, 0.7, 0.3], f32)
    axis, lo, hi = S.skin_extent(tris)
    bend = S.bend_palette(BONES, 0.08, axis, lo, hi)
    rest_image = shot(r1)[0]
    # 1. host.Render
    r1.set_morph(deltas, offsets)
    line = "morph targets: %d targets, %d deltas, " % (TARGETS, len(deltas))
    assert line in r1.tree_report() and "rest pose 160 + staging area 160 + row 4 bytes per triangle, 32 per delta" in r1.tree_report(), r1.tree_report()
    r1.morph(w)
    report = r1.tree_report()
    assert report.count("morph targets: ") == 1 and report.index(line) < report.index("refit 1:"), report      # kept across the refit, before its line
    img1, rays1 = shot(r1)
    with pytest.raises(host.RtError, match="rt_scene_morph: the target count differs"):
        r1.morph(w[:-1])
    with pytest.raises(host.RtError, match="rt_scene_morph_skin: no skin"):
        r1.morph_skin(w, bend)
    r1.set_skin()
    r1.morph_skin(w, bend)
    fused1, frays1 = shot(r1)
    assert r1.tree_report().count("morph targets: ") == 1 and "skinned triangles: " in r1.tree_report()
    # 2. the C++ layer through the flat C API
    r2 = host.Render(W, H, scene_of(golden_scenes, False))
    r2.set_refittable(True)
    r2.set_camera(cam); r2.set_max_bounces(BOUNCES)
    assert r2.scene_arrays()["triangles"].tobytes() == tris.tobytes()
    lib = host.load()
    flat = np.ascontiguousarray(infl).reshape(-1)
    assert lib.rth_render_set_morph(r2.handle, deltas.ctypes.data, offsets.ctypes.data, TARGETS, len(tris)) == 0, lib.rth_last_error()
    assert lib.rth_render_morph(r2.handle, w.ctypes.data, TARGETS - 1) != 0 and b"rt_scene_morph: the target count differs" in lib.rth_last_error()
    assert lib.rth_render_morph(r2.handle, w.ctypes.data, TARGETS) == 0, lib.rth_last_error()
    img2, rays2 = shot(r2)
    assert lib.rth_render_set_skin(r2.handle, flat.ctypes.data, len(tris), BONES) == 0, lib.rth_last_error()
    assert lib.rth_render_morph_skin(r2.handle, w.ctypes.data, TARGETS, bend.ctypes.data, BONES) == 0, lib.rth_last_error()
    fused2, frays2 = shot(r2)
    # 3. the C ABI's binding, and what all must equal: the refit of the restatement's triangles
    c = capi.Context(0)
    try:
        c.set_refittable(True)
        c.upload_scene(arrays)

        def image():
            fr = capi.Frame(c, W, H)
            fr.set_camera(cam); fr.set_max_bounces(BOUNCES)
            fr.integrate(SPP)
            st = fr.stats()
            out = fr.radiance().copy(), (st.closest_rays, st.shadow_rays)
            fr.close()
            return out

        c.set_morph(deltas, offsets, len(tris))
        with pytest.raises(capi.RtError, match="rt_scene_morph: the target count differs"):
            c.morph_scene(w[1:])
        c.morph_scene(w)
        img3, rays3 = image()
        c.set_skin(infl, BONES)
        c.morph_skin_scene(w, bend)
        fused3, frays3 = image()
        morphed = capi.debug_morph(None, tris, deltas, offsets, w)
        c.refit_scene(morphed)
        want = image()[0]
        c.refit_scene(capi.debug_skin(None, morphed, infl, bend))
        fused_want = image()[0]
    finally:
        c.close()
    assert img1.tobytes() == img2.tobytes() == img3.tobytes() == want.tobytes()
    assert fused1.tobytes() == fused2.tobytes() == fused3.tobytes() == fused_want.tobytes()
    assert rays1 == rays2 == rays3 and frays1 == frays2 == frays3
    assert img1.tobytes() != rest_image.tobytes() and fused1.tobytes() != img1.tobytes()       # both move what the camera sees
    r1.set_refittable(True)                                           # uploads again: the morph is dropped
    with pytest.raises(host.RtError, match="rt_scene_morph: no morph"):
        r1.morph(w)
    assert "morph targets" not in r1.tree_report()
    r1.close(); r2.close()
