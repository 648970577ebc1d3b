"""The spatial filter at 1080p on the city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles): one sample, then
rt_frame_filter with the header's defaults (RT_FILTER_DESC_DEFAULT) -- the first call runs the guide pass (pixel-centre rays, k_trace_v1<false>,
guide values), the next ones only the a-trous passes.  Prints wall times; run under `rocprofv3 --kernel-trace --stats -- python tools/filter_profile.py` for the
per-kernel times (k_sf_guide_rays, k_trace_v1, k_sf_guide_values, k_sf_pass)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host, scenes as S  # noqa: E402


def main():
    n_tris = int(sys.argv[1]) if len(sys.argv) > 1 else 2_800_000
    w, h = 1920, 1080
    scene = host.Scene(arrays=S.city_block(n_tris))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    ctx = capi.Context(0)
    ctx.upload_scene(scene.arrays())
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(host.default_camera(w, h))
    fr.set_max_bounces(4)
    fr.integrate(1)
    fr.resolve()
    t0 = time.perf_counter()
    img = fr.filter()                                   # guide pass + the default passes + read-back
    t1 = time.perf_counter()
    times = []
    for _ in range(10):
        a = time.perf_counter()
        fr.filter()
        times.append(time.perf_counter() - a)
    r = []
    for _ in range(10):
        a = time.perf_counter()
        fr.resolve()
        r.append(time.perf_counter() - a)
    hit = fr.guides()[2] < 20000.0
    print("filter_profile: %dx%d, %d triangles; first filter (with guide pass) %.2f ms, filter %.2f ms (median of 10), resolve %.2f ms; "
          "guide hits %.1f %%, finite pixels %.1f %%" % (w, h, n_tris, 1e3 * (t1 - t0), 1e3 * np.median(times), 1e3 * np.median(r),
                                                       100.0 * hit.mean(), 100.0 * np.isfinite(img).all(-1).mean()))
    fr.close()
    ctx.close()


if __name__ == "__main__":
    main()
