"""-m gpu: the UV atlas through the layers above the C-ABI: HIPPathTraceIntegrator::AtlasCover / BakeAtlas behind host.Render.atlas() /
.occlusion_atlas(), and rt_render --ao_atlas, each against capi.Context on the same scene arrays.  One Render, one context, one run of the CLI."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_atlas import INVALID, f32, same_cover, refused as capi_refused

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SAMPLES, RADIUS = 24, 16, 16, 0.5


def test_render_atlas_occlusion_atlas_and_the_cli_equal_the_c_abi(tmp_path):
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    render = host.Render(16, 16, scene)
    arrays = {k: np.array(v) for k, v in render.scene_arrays().items() if k != "flags"}
    uv = S.synthetic_atlas(arrays["triangles"], W, H)
    c = capi.Context(0)
    try:
        c.upload_scene(arrays)
        for kw in (dict(uv=uv), dict(gutter=1), dict(uv=uv * f32(0.5), gutter=2)):
            same_cover(render.atlas(W, H, **kw), c.atlas(W, H, **kw), kw.keys())
        for kw in (dict(uv=uv * f32(0.5), gutter=1), dict(uv=uv)):
            img, stats = render.occlusion_atlas(W, H, SAMPLES, RADIUS, seed=0, **kw)
            out, texels, want_stats = c.bake_atlas(W, H, SAMPLES, seed=0, radius=RADIUS, **kw)
            want = np.where(out["unoccluded"] == INVALID, f32(np.nan), out["unoccluded"].astype(f32) / f32(SAMPLES)).astype(f32)
            assert img.shape == (H, W) and img.dtype == f32 and img.tobytes() == want.reshape(H, W).tobytes()
            assert stats.tobytes() == want_stats.tobytes() and int(np.isnan(img).sum()) == W * H - int(stats["covered"]) - int(stats["gutter"])
        assert ((img > 0) & (img < 1)).any()
        # rt_render --ao_atlas writes that image, the atlas's row 0 first, grey; NaN where no triangle covers a texel
        path = tmp_path / "ao_atlas.pfm"
        r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", "16", "-h", "16", "--spp", "1", "--scene", "assets/CornellBox.obj", "--ao_atlas", str(path),
                            "--atlas_size", "%d,%d" % (W, H), "--atlas_uv", "synthetic", "--ao_samples", str(SAMPLES), "--ao_radius", repr(RADIUS)],
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ambient occlusion atlas 24x16" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
        raw = path.read_bytes()
        head = ("PF\n%d %d\n-1.0\n" % (W, H)).encode()
        assert raw.startswith(head)
        pfm = np.frombuffer(raw[len(head):], f32).reshape(H, W, 3)
        assert pfm[:, :, 0].tobytes() == pfm[:, :, 1].tobytes() == img.tobytes()
        assert int(np.isnan(pfm[:, :, 0]).sum()) == W * H - int(stats["covered"])
        # the layers pass the library's refusals on
        for fn in (render.atlas, lambda w, h, **k: render.occlusion_atlas(w, h, SAMPLES, RADIUS, **k)):
            with pytest.raises(host.RtError, match="width and height must be 1 .. 16384"):
                fn(0, 8)
            with pytest.raises(host.RtError, match="gutter must be 0 .. 4"):
                fn(8, 8, gutter=5)
        with pytest.raises(host.RtError, match="samples must be a power of two"):
            render.occlusion_atlas(8, 8, 17, RADIUS)
    finally:
        c.close()
        render.close()
