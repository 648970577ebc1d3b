"""The temporal filter across refits at 1080p on the city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles) with the
geometry deforming every frame under a standing camera: each frame refits the scene from a device buffer (rt_scene_refit_buffer), is reset, traced
with one sample and passed through rt_frame_filter_temporal with the header's defaults.  With RT_CTX_OPT_REFIT_MOTION (the default here; `off` as
the third argument runs the same frames without it) every refit first snapshots the pose it replaces (k_sf_snapshot_pose) and every filter call runs
the guide pass, the motion images (k_sf_guide_motion) and the accumulation with them.  Prints wall times; run under `rocprofv3 --kernel-trace --stats
-- python tools/motion_filter_profile.py` for the per-kernel times (k_sf_snapshot_pose, k_refit_*, k_sf_guide_values, k_sf_guide_motion,
k_tf_accumulate, k_tf_variance, k_tf_pass)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host, scenes as S  # noqa: E402


def deformed(tris, amplitude, phase=0.5):
    """every vertex displaced by a smooth field of its position (shared vertices stay shared), scaled to the scene"""
    P = np.stack([np.stack([tris[v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).astype(np.float64)
    size = float(np.ptp(P.reshape(-1, 3), axis=0).max()) or 1.0
    Q = P / size * 5.0 + phase
    D = np.stack([np.sin(Q[..., 1] * 1.3 + Q[..., 2]), np.cos(Q[..., 0] * 0.7 - Q[..., 2] * 1.1), np.sin(Q[..., 0] + Q[..., 1] * 0.9)], -1)
    P = (P + amplitude * size * D).astype(np.float32)
    out = tris.copy()
    for k, v in enumerate(("v1", "v2", "v3")):
        for a, c in enumerate("xyz"):
            out[v]["position"][c] = P[:, k, a]
    return out


def main():
    n_tris = int(sys.argv[1]) if len(sys.argv) > 1 else 2_800_000
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    motion = not (len(sys.argv) > 3 and sys.argv[3] == "off")
    w, h = 1920, 1080
    scene = host.Scene(arrays=S.city_block(n_tris))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    arrays = scene.arrays()
    tris = np.array(arrays["triangles"])
    ctx = capi.Context(0)
    ctx.set_refittable(True)
    if motion:
        ctx.set_refit_motion(True)
    ctx.upload_scene(arrays)
    fr = capi.Frame(ctx, w, h)
    fr.set_max_bounces(4)
    fr.set_camera(host.default_camera(w, h))
    poses = [ctx.create_buffer(deformed(tris, 0.0002 * (k % 2))) for k in range(2)]      # two poses on the device, alternating: no PCIe copy per frame
    refit, trace, filt = [], [], []
    for k in range(frames):
        a = time.perf_counter()
        if k:
            ctx.refit_scene(poses[k % 2])
            ctx.finish()
        b = time.perf_counter()
        fr.reset()
        fr.integrate(1)
        fr.resolve()
        c = time.perf_counter()
        img = fr.filter_temporal()                      # guide pass (a new scene) + motion images + accumulation + variance + passes + read-back
        d = time.perf_counter()
        refit.append(b - a); trace.append(c - b); filt.append(d - c)
    L = fr.filter_history()[1][..., 2]
    print("motion_filter_profile: %dx%d, %d triangles, %d frames, one refit each, RT_CTX_OPT_REFIT_MOTION %s; refit %.2f ms, 1 spp + resolve %.2f ms, "
          "filter_temporal %.2f ms (medians); history lengths of the last frame: L = %d %.1f %%, L >= 4 %.1f %%, L = 1 %.1f %%, L = 0 %.1f %%; "
          "finite pixels %.1f %%" %
          (w, h, n_tris, frames, "on" if motion else "off", 1e3 * np.median(refit[1:] or refit), 1e3 * np.median(trace), 1e3 * np.median(filt), frames,
           100.0 * (L == frames).mean(), 100.0 * (L >= 4).mean(), 100.0 * (L == 1).mean(), 100.0 * (L == 0).mean(),
           100.0 * np.isfinite(img).all(-1).mean()))
    print(ctx.tree_report().strip().splitlines()[-1])
    fr.close()
    for p in poses:
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
