"""-m gpu: the spatial filter (rt_frame_filter, rt_frame_read_guides, rt_debug_filter; raytracing_amd/csrc/spatial_filter.h).
The kernel equals the host restatement bit for bit, zero iterations are rt_frame_resolve bit for bit on every path that makes a frame, the
guides are the first hits of pixel-centre rays and are recomputed exactly when the camera or the scene changes, and the filter lowers the
error of a 4-spp frame against a 1024-spp one."""
import numpy as np
import pytest

from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_spatial_filter import random_inputs

pytestmark = pytest.mark.gpu
MAX_DIST = 20000.0


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (23, 41), (1080, 1920)])
def test_kernel_equals_host_restatement_bit_for_bit(ctx, shape):
    rng = np.random.default_rng(shape[0] + 7 * shape[1])
    hdr, alb, nrm, dep = random_inputs(rng, *shape)
    hdr[rng.random(shape) < 0.001, 0] = np.nan
    for it in ((1, 5, 8) if shape[0] > 100 else range(0, 9)):
        for demod in (0, 1):
            desc = dict(iterations=it, flags=demod, sigma_color=float(rng.uniform(0.2, 2.0)), sigma_normal=float(rng.uniform(0.05, 1.0)),
                        sigma_depth=float(rng.uniform(0.05, 1.0)))
            dev = capi.debug_filter(ctx, hdr, alb, nrm, dep, desc)
            ref = capi.debug_filter(None, hdr, alb, nrm, dep, desc)
            assert np.array_equal(bits(dev), bits(ref)), (it, demod, int((bits(dev) != bits(ref)).sum()))


def stage_sample(fr, bounces, aovs=False):
    fr.generate_rays()
    for b in range(bounces + 1):
        fr.intersect(b)
        if aovs and b == 0:
            fr.lib.rt_compute_aovs(fr.handle)
        fr.shade(b); fr.intersect_shadow(b)
    fr.advance_sample()
    if aovs:
        fr.lib.rt_denoise(fr.handle); fr.lib.rt_copy_history(fr.handle)


def check_identity(fr):
    rad = fr.radiance()
    assert np.array_equal(bits(fr.filter(dict(iterations=0))), bits(fr.resolve()))
    fr.filter()                                                  # the default filter leaves the frame's own state alone
    assert np.array_equal(bits(fr.radiance()), bits(rad))
    assert np.array_equal(bits(fr.filter(dict(iterations=0))), bits(fr.resolve()))


@pytest.mark.parametrize("path", ["integrate_in_flight", "samples_ahead", "frame_kernel", "denoiser", "after_reset"])
def test_zero_iterations_is_resolve_bit_for_bit(ctx, golden_scenes, golden_radiance, path):
    ctx.upload_scene(golden_scenes["coverage"])
    cam = golden_radiance["coverage_64_b6_s2/camera"]
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(cam); fr.set_max_bounces(4)
    if path == "integrate_in_flight":
        fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 4)
        fr.integrate(7)
    elif path == "samples_ahead":
        fr.set_option(capi.OPT_SAMPLES_AHEAD, 4)
        for _ in range(9):
            stage_sample(fr, 4)
        assert fr.stats().samples_from_banks > 0
    elif path == "frame_kernel":
        fr.set_option(capi.OPT_FRAME_KERNEL, 1)
        for _ in range(3):
            stage_sample(fr, 4)
        assert fr.stats().frame_kernel_samples > 0
    elif path == "denoiser":
        fr.set_option(capi.OPT_DENOISER, 1)
        for _ in range(3):
            stage_sample(fr, 4, aovs=True)
    else:
        fr.integrate(3)
        fr.reset()
        fr.integrate(2)
    check_identity(fr)
    fr.close()


def quad_scene(env, kd):
    mats = [S.make_material(kd=kd)]
    meshes = [S.quad((-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0)) + (0,)]
    s = host.Scene(arrays=dict(triangles=S.to_triangles(meshes), materials=np.array(mats, dtype=T.packed_material),
                               textures=np.zeros(0, T.texture), texture_data=np.zeros(0, np.uint32)))
    s.build_bvh()
    s.set_env_image(np.zeros_like(env))
    s.finalize()
    return s.arrays()


def down_camera(w, h, height, fov=1.0):
    cam = T.default_camera(w, h)
    for key, v in (("position", (0.1, -0.2, height)), ("front", (0.0, 0.0, -1.0)), ("up", (0.0, 1.0, 0.0))):
        for k, x in zip("xyz", v):
            cam[key][k] = np.float32(x)
    cam["fov"] = np.float32(fov)
    cam["aspect_ratio"] = np.float32(w / h)
    cam["aperture"] = np.float32(0.05)                       # guides ignore the lens
    return cam


def pixel_centre_dirs(cam, w, h):
    """the guide rays' directions (k_sf_guide_rays) in float64"""
    f = np.array([cam["front"][k] for k in "xyz"], np.float64).ravel()
    u = np.array([cam["up"][k] for k in "xyz"], np.float64).ravel()
    r = np.cross(f, u)
    t = np.tan(0.5 * float(cam["fov"]))
    ys, xs = np.mgrid[0:h, 0:w]
    x = ((xs + 0.5) / w * 2 - 1) * t * float(cam["aspect_ratio"])
    y = ((ys + 0.5) / h * 2 - 1) * t
    d = r * x[..., None] + u * y[..., None] + f
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_guides_on_an_analytic_quad(ctx, env_map):
    kd = (0.6, 0.3, 0.15)
    scene = quad_scene(env_map, kd)
    ctx.upload_scene(scene)
    w, h, D = 48, 32, 3.0
    cam = down_camera(w, h, D)
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(cam)
    alb, nrm, dep, passes = fr.guides()
    assert passes == 1
    assert (dep < MAX_DIST).all()
    packed = int(scene["materials"][0]["diffuse_albedo"])           # UnpackRGBTex: byte / 255 per channel
    want_alb = np.array([(packed >> s & 0xFF) for s in (0, 8, 16)], np.float32) / np.float32(255.0)
    assert np.array_equal(alb[..., :3], np.broadcast_to(want_alb, alb[..., :3].shape))
    assert np.array_equal(nrm[..., :3], np.broadcast_to(np.float32((0, 0, 1)), nrm[..., :3].shape))
    cos_t = -pixel_centre_dirs(cam, w, h)[..., 2]
    np.testing.assert_allclose(dep, D / cos_t, rtol=1e-5)
    fr.close()


def test_guides_are_recomputed_exactly_when_camera_or_scene_change(ctx, golden_scenes, golden_radiance):
    ctx.upload_scene(golden_scenes["coverage"])
    cam = golden_radiance["coverage_64_b6_s2/camera"].copy()
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(cam)
    g1 = fr.guides()
    assert g1[3] == 1
    fr.integrate(2)
    fr.filter()
    fr.set_camera(cam)                                       # the same bytes
    fr.filter()
    assert fr.guides()[3] == 1
    # the coverage scene: hits and misses, several materials and normals
    hit = g1[2] < MAX_DIST
    assert 0 < hit.sum() <= hit.size
    assert len(np.unique(g1[0][hit][:, :3], axis=0)) > 3 and len(np.unique(g1[1][hit][:, :3], axis=0)) > 10
    np.testing.assert_allclose(np.linalg.norm(g1[1][hit][:, :3], axis=-1), 1.0, rtol=1e-6)
    assert (g1[0][~hit] == 0).all() and (g1[1][~hit] == 0).all()
    cam2 = cam.copy()
    cam2["position"]["x"] = np.float32(cam2["position"]["x"] + np.float32(0.05))
    fr.set_camera(cam2)
    g2 = fr.guides()
    assert g2[3] == 2 and not np.array_equal(g2[2], g1[2])
    fr.set_camera(cam)
    assert fr.guides()[3] == 3
    ctx.upload_scene(golden_scenes["coverage"])
    g4 = fr.guides()
    assert g4[3] == 4
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(g1[:3], g4[:3]))   # same scene, same camera: same guides
    fr.close()


def test_refusals(ctx, golden_scenes, golden_radiance):
    ctx.upload_scene(golden_scenes["cornell"])
    cam = golden_radiance["cornell_64_b4_s2/camera"]
    tile = capi.Frame(ctx, 64, 64, tile_rank=0, tile_count=2, band_height=8)
    tile.set_camera(cam)
    tile.integrate(1)
    with pytest.raises(capi.RtError, match="whole image"):
        tile.filter()
    with pytest.raises(capi.RtError, match="whole image"):
        tile.guides()
    tile.close()
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(cam)
    fr.set_option(capi.OPT_AOV, 1)
    with pytest.raises(capi.RtError, match="RT_OPT_AOV"):
        fr.filter()
    fr.set_option(capi.OPT_AOV, 0)
    with pytest.raises(capi.RtError, match="iterations"):
        fr.filter(dict(iterations=9))
    fr.close()


def tonemapped_mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3]) ** 2))


@pytest.mark.parametrize("name", ["cornell_64_b4_s2", "coverage_64_b6_s2"])
def test_filtered_4spp_halves_the_error_against_1024spp(ctx, golden_scenes, golden_radiance, name):
    ctx.upload_scene(golden_scenes[name.split("_")[0]])
    cam = golden_radiance[name + "/camera"]
    fr = capi.Frame(ctx, 128, 128)
    fr.set_camera(cam); fr.set_max_bounces(4)
    fr.integrate(1024)
    ref = fr.resolve()
    fr.reset()
    fr.integrate(4)
    noisy, filtered = fr.resolve(), fr.filter()
    ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1)
    e0, e1 = tonemapped_mse(noisy[ok], ref[ok]), tonemapped_mse(filtered[ok], ref[ok])
    print("%s: tone-mapped MSE 4 spp %.3e, filtered %.3e, ratio %.3f" % (name, e0, e1, e1 / e0))
    assert e1 <= 0.5 * e0
    fr.close()
