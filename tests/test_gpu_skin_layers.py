"""-m gpu: the layers above rt_scene_set_skin / rt_scene_skin on one small scene: host.Render.set_skin() / .skin() with the scene's own
table, HIPPathTraceIntegrator::SetSkin / SkinBones through rth_render_set_skin / rth_render_skin with a caller's table, and capi.Context.set_skin() /
skin_scene().  All three give the same image bits, and each raises the library's message on a wrong bone count.  One process, each GPU step once; nothing here
provokes a fault."""
import os
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BOUNCES = 64, 64, 2, 4
BONES = 6


def scene_of(golden_scenes, with_skin):
    sc = golden_scenes["cornell"]
    arrays = {k: sc[k] for k in ("triangles", "materials", "textures", "texture_data")}
    n = len(arrays["triangles"])
    arrays["triangles"] = arrays["triangles"][np.random.default_rng(4).permutation(n)]          # so that the build reorders triangles and influences alike
    s = host.Scene(arrays=arrays, skin=S.synthetic_skin(arrays["triangles"], BONES) if with_skin else None)
    s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    s.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    return s


def shot(r):
    r.render_samples(SPP)
    assert r.sample_count() == SPP                                    # the skin requested a reset
    st = r.stats()
    return r.radiance().copy(), (st.closest_rays, st.shadow_rays)


def test_three_layers_give_the_same_image(golden_scenes):
    cam = host.default_camera(W, H)
    # 1. host.Render with the scene's own table
    r1 = host.Render(W, H, scene_of(golden_scenes, True))
    r1.set_refittable(True)
    r1.set_camera(cam); r1.set_max_bounces(BOUNCES)
    arrays = dict(r1.scene_arrays())
    tris = arrays["triangles"].copy()
    infl = r1.scene.triangle_skin()
    assert infl.shape == (len(tris), 3) and r1.scene.num_bones() == BONES
    assert infl.tobytes() == T.influences(*S.synthetic_skin(tris, BONES)).tobytes()          # the scene's table is in the uploaded order
    axis, lo, hi = S.skin_extent(tris)
    bend = S.bend_palette(BONES, 0.08, axis, lo, hi)
    r1.set_skin()
    assert "skinned triangles: %d bones" % BONES in r1.tree_report()
    r1.render_samples(1)
    r1.skin(bend)
    img1, rays1 = shot(r1)
    with pytest.raises(host.RtError, match="rt_scene_skin: the bone count differs"):
        r1.skin(bend[:-1])
    r1.skin(bend.reshape(BONES, 12))                                  # [n, 12] is taken too
    assert shot(r1)[0].tobytes() == img1.tobytes()
    # 2. the C++ layer through the flat C API, a table of the caller's own
    r2 = host.Render(W, H, scene_of(golden_scenes, False))
    r2.set_refittable(True)
    r2.set_camera(cam); r2.set_max_bounces(BOUNCES)
    assert r2.scene_arrays()["triangles"].tobytes() == tris.tobytes()
    rest_image = shot(r2)[0]
    lib = host.load()
    flat = np.ascontiguousarray(infl).reshape(-1)
    assert lib.rth_render_set_skin(r2.handle, flat.ctypes.data, len(tris), BONES) == 0, lib.rth_last_error()
    assert lib.rth_render_skin(r2.handle, bend.ctypes.data, BONES - 1) != 0 and b"rt_scene_skin: the bone count differs" in lib.rth_last_error()
    assert lib.rth_render_skin(r2.handle, bend.ctypes.data, BONES) == 0, lib.rth_last_error()
    img2, rays2 = shot(r2)
    with pytest.raises(host.RtError, match="set_skin: the scene carries no skin"):
        r2.set_skin()
    # 3. the C ABI's binding
    c = capi.Context(0)
    try:
        c.set_refittable(True)
        c.upload_scene(arrays)
        c.set_skin(infl, BONES)
        with pytest.raises(capi.RtError, match="rt_scene_skin: the bone count differs"):
            c.skin_scene(bend[1:])
        c.skin_scene(bend)
        fr = capi.Frame(c, W, H)
        fr.set_camera(cam); fr.set_max_bounces(BOUNCES)
        fr.integrate(SPP)
        st = fr.stats()
        img3, rays3 = fr.radiance().copy(), (st.closest_rays, st.shadow_rays)
        fr.close()
        # ... and what all three must equal: the refit of the restatement's triangles
        c.refit_scene(capi.debug_skin(None, tris, infl, bend))
        fr = capi.Frame(c, W, H)
        fr.set_camera(cam); fr.set_max_bounces(BOUNCES)
        fr.integrate(SPP)
        want = fr.radiance().copy()
        fr.close()
    finally:
        c.close()
    assert img1.tobytes() == img2.tobytes() == img3.tobytes() == want.tobytes()
    assert rays1 == rays2 == rays3
    assert img1.tobytes() != rest_image.tobytes()                     # the bend does move what the camera sees
    r1.close(); r2.close()


def test_a_refusal_arrives_as_the_librarys_message(golden_scenes):
    r = host.Render(W, H, scene_of(golden_scenes, True))
    with pytest.raises(host.RtError, match="rt_scene_set_skin: RT_CTX_OPT_REFITTABLE was off when the scene was uploaded"):
        r.set_skin()
    r.set_refittable(True)
    bend = np.stack([np.eye(3, 4, dtype=np.float32)] * BONES)
    with pytest.raises(host.RtError, match="rt_scene_skin: no skin"):
        r.skin(bend)
    with pytest.raises(host.RtError, match="rt_scene_set_skin: a bone index is not below num_bones"):
        r.set_skin(r.scene.triangle_skin(), BONES - 1)
    with pytest.raises(host.RtError, match="num_bones is needed"):
        r.set_skin(r.scene.triangle_skin())
    r.set_skin()
    bad = bend.copy()
    bad[2, 1, 1] = np.inf
    with pytest.raises(host.RtError, match="rt_scene_skin: a matrix entry is not finite"):
        r.skin(bad)
    with pytest.raises(host.RtError, match="matrices must be"):
        r.skin(bend[:, :2])
    r.skin(bend)
    r.set_refittable(True)                                            # uploads again: the skin is dropped
    with pytest.raises(host.RtError, match="rt_scene_skin: no skin"):
        r.skin(bend)
    r.close()
