"""-m gpu: the spatial filter above the C-ABI and against the CPU walk -- RT_OPT_DENOISER = 2 filters the image rt_frame_resolve returns,
HIPPathTraceIntegrator::SetSpatialFilter (host.Render.set_spatial_filter) equals Frame.filter, tiles and TiledRender refuse, and the coverage
scene's guides are the first hits tests/_oracle.py's wide walk finds for the same pixel-centre rays."""
import os
import subprocess

import numpy as np
import pytest

from raytracing_amd import capi, host, types as T
from tests import _oracle
from tests.test_wide_bvh import wide_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DIST = np.float32(20000.0)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_denoiser_mode_2_filters_the_resolved_image(ctx, golden_scenes, golden_radiance):
    """RT_OPT_DENOISER = 2: the radiance holds one sample while the sample count grows; k_resolve does not divide, nor may the filter.
    With a vanishing sigma_color only identical colours weigh, so the filtered image is the resolved one up to the remodulation's rounding."""
    ctx.upload_scene(golden_scenes["coverage"])
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(golden_radiance["coverage_64_b6_s2/camera"]); fr.set_max_bounces(4)
    fr.set_option(capi.OPT_DENOISER, 2)
    for _ in range(4):
        fr.integrate(1)
    assert fr.sample_count() == 4
    want = fr.resolve()
    got = fr.filter(dict(iterations=2, flags=capi.FILTER_DEMODULATE, sigma_color=1e-6, sigma_normal=0.1, sigma_depth=0.1))
    ok = np.isfinite(want).all(-1)
    # (dark pixels whose colours differ by less than ~1e-6 still blend: that is the filter, not the sample count)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5, atol=1e-5)
    fr.close()


def test_render_set_spatial_filter_equals_frame_filter(ctx):
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    w, h = 96, 64
    render = host.Render(w, h, scene)
    cam = host.default_camera(w, h)
    render.set_camera(cam); render.set_max_bounces(4)
    render.render_samples(4)
    desc = dict(iterations=3, flags=capi.FILTER_DEMODULATE, sigma_color=4.0, sigma_normal=0.1, sigma_depth=0.1)
    plain = render.resolve_now()
    render.set_spatial_filter(desc)
    via_render = render.resolve_now()
    render.set_spatial_filter(on=False)
    assert np.array_equal(bits(render.resolve_now()), bits(plain))

    ctx.upload_scene(render.scene_arrays())
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(cam); fr.set_max_bounces(4)
    fr.integrate(4)
    assert np.array_equal(bits(fr.radiance()), bits(render.radiance()))
    assert np.array_equal(bits(fr.filter(desc)), bits(via_render))
    assert not np.array_equal(bits(via_render), bits(plain))
    fr.close()


def test_a_tile_and_tiled_render_refuse():
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    tile = host.Render(64, 64, scene, tile_rank=0, tile_count=2)
    with pytest.raises(RuntimeError, match="whole image"):
        tile.set_spatial_filter()
    tile.set_spatial_filter(on=False)                        # off is always accepted
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "--tiled", "1", "--filter", "2", "-w", "64", "-h", "64", "--spp", "1",
                        "--scene", "assets/CornellBox.obj"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "TiledRender" in r.stderr and "whole image" in r.stderr, (r.returncode, r.stderr[-500:])


def guide_rays(ctx, cam, w, h):
    """k_sf_guide_rays restated in float32 in the kernel's order of operations (tan from the device's rt_tanf)"""
    f32 = np.float32
    tan_half = f32(ctx.debug_eval(2, np.array([f32(0.5) * f32(cam["fov"])], np.float32))[0])
    ys, xs = np.mgrid[0:h, 0:w]
    x = (xs.astype(f32) + f32(0.5)) * (f32(1.0) / f32(w))
    y = (ys.astype(f32) + f32(0.5)) * (f32(1.0) / f32(h))
    x = (x * f32(2.0) - f32(1.0)) * tan_half * f32(cam["aspect_ratio"])
    y = (y * f32(2.0) - f32(1.0)) * tan_half
    fr_ = [f32(cam["front"][k]) for k in "xyz"]
    up = [f32(cam["up"][k]) for k in "xyz"]
    right = [fr_[1] * up[2] - fr_[2] * up[1], fr_[2] * up[0] - fr_[0] * up[2], fr_[0] * up[1] - fr_[1] * up[0]]     # cross3(front, up)
    d = [right[c] * x + up[c] * y + fr_[c] for c in range(3)]
    ln = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    rays = np.zeros(w * h, T.ray)
    for c, k in enumerate("xyz"):
        rays["origin"][k] = f32(cam["position"][k])
        rays["direction"][k] = (d[c] / ln).ravel()
    rays["direction"]["w"] = MAX_DIST                 # the reference's Ray: t_max in direction.w, origin.w = 0
    return rays


def test_coverage_guides_match_the_cpu_walk(ctx, golden_scenes, golden_radiance):
    scene = golden_scenes["coverage"]
    cam = golden_radiance["coverage_64_b6_s2/camera"]
    w = h = 64
    ctx.upload_scene(scene)
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(cam)
    alb, nrm, dep, _ = fr.guides()
    fr.close()
    rays = guide_rays(ctx, cam, w, h)
    wide, entry = wide_of(scene["nodes"], 1)
    hits = _oracle.Oracle(w, h, scene).wide_trace(wide, entry, rays, False)
    prim = hits["primitive_id"].reshape(h, w)
    hit = prim != 0xFFFFFFFF
    assert np.array_equal(hit, dep < MAX_DIST)                          # the same pixels hit and miss
    assert hit.sum() > 0.5 * hit.size                                   # (the coverage camera looks into a closed box)
    # the per-primitive values: interpolated normal, the hit distance, and the albedo of untextured materials
    tri = scene["triangles"][prim[hit]]
    bu = hits["bc"][:, 0].reshape(h, w)[hit].astype(np.float64)
    bv = hits["bc"][:, 1].reshape(h, w)[hit].astype(np.float64)
    w0 = 1.0 - bu - bv
    n = sum(np.stack([tri[v]["normal"][k] for k in "xyz"], -1).astype(np.float64) * wt[:, None] for v, wt in (("v1", w0), ("v2", bu), ("v3", bv)))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    np.testing.assert_allclose(nrm[hit][:, :3], n, atol=2e-5)
    np.testing.assert_allclose(dep[hit], hits["t"].reshape(h, w)[hit], rtol=2e-5)
    mats = scene["materials"][tri["mtl_index"]]
    untextured = (mats["diffuse_albedo"] >> 24) == 0xFF
    want = np.stack([((mats["diffuse_albedo"] >> s) & 0xFF).astype(np.float32) / np.float32(255.0) for s in (0, 8, 16)], -1)
    assert untextured.sum() > 100
    assert np.array_equal(alb[hit][untextured, :3], want[untextured])
