"""The temporal filter at 1080p on the city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles) with the camera moving
every frame: each frame is reset, traced with one sample and passed through rt_frame_filter_temporal with the header's defaults
(RT_TEMPORAL_FILTER_DESC_DEFAULT), so every call runs the guide pass (pixel-centre rays, k_trace_v1<false>, guide values), the accumulation,
the variance estimate and the variance-guided passes.  Prints wall times; run under `rocprofv3 --kernel-trace --stats -- python
tools/temporal_filter_profile.py` for the per-kernel times (k_sf_guide_rays, k_trace_v1, k_sf_guide_values, k_tf_accumulate, k_tf_variance,
k_tf_pass)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host, scenes as S  # noqa: E402


def main():
    n_tris = int(sys.argv[1]) if len(sys.argv) > 1 else 2_800_000
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    w, h = 1920, 1080
    scene = host.Scene(arrays=S.city_block(n_tris))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    ctx = capi.Context(0)
    ctx.upload_scene(scene.arrays())
    fr = capi.Frame(ctx, w, h)
    fr.set_max_bounces(4)
    cam = host.default_camera(w, h)
    x0 = float(cam["position"]["x"])
    trace, filt, resolve = [], [], []
    for k in range(frames):
        cam["position"]["x"] = np.float32(x0 + 0.01 * k)
        fr.set_camera(cam)
        fr.reset()
        a = time.perf_counter()
        fr.integrate(1)
        fr.resolve()
        b = time.perf_counter()
        img = fr.filter_temporal()                      # guide pass (a new camera) + accumulation + variance + passes + read-back
        c = time.perf_counter()
        fr.resolve()
        d = time.perf_counter()
        trace.append(b - a); filt.append(c - b); resolve.append(d - c)
    L = fr.filter_history()[1][..., 2]
    print("temporal_filter_profile: %dx%d, %d triangles, %d moving-camera frames; 1 spp + resolve %.2f ms, filter_temporal %.2f ms, resolve %.2f ms "
          "(medians); history lengths of the last frame: L >= 4 %.1f %%, L = 1 %.1f %%, L = 0 %.1f %%; finite pixels %.1f %%" %
          (w, h, n_tris, frames, 1e3 * np.median(trace), 1e3 * np.median(filt), 1e3 * np.median(resolve), 100.0 * (L >= 4).mean(),
           100.0 * (L == 1).mean(), 100.0 * (L == 0).mean(), 100.0 * np.isfinite(img).all(-1).mean()))
    fr.close()
    ctx.close()


if __name__ == "__main__":
    main()
