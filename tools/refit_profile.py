"""What moving a scene's triangles costs: rt_scene_refit_buffer against rt_scene_upload of the same moved scene, on the city-block stand-in of bench.py's
config 4 (scenes.city_block, ~2.8 M triangles, default options), in one session on one device.

  * the yardstick: rt_scene_upload (RT_CTX_OPT_REFITTABLE off: the code path is the parent's) of the moved triangles with the refitted node array, a few times;
  * the refit: a warm-up, then --refits calls of rt_scene_refit_buffer alternating between two poses that are on the device already; host clock around the
    call + rt_finish; the median is what DESIGN quotes, and "done" is median refit <= upload / 10;
  * what a refitted tree costs to trace: per stated deformation (a smooth displacement field, amplitude as a fraction of the scene's largest extent), 1080p
    samples on the refitted context against a fresh upload of that pose with a BVH built for it -- no threshold, users need to know when to upload again.

Per-kernel times: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/refit_profile.py --refits 20 --no-trace` in a run of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host, scenes as S  # noqa: E402


def positions(tris):
    return np.stack([np.stack([tris[v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1)


def smooth(tris, amplitude, phase=0.0):
    """every vertex displaced by a smooth field of its position (shared vertices stay shared); amplitude = fraction of the scene's largest extent"""
    P = positions(tris).astype(np.float64)
    size = float(np.ptp(P.reshape(-1, 3), axis=0).max())
    Q = P / size * 40.0 + phase
    D = np.stack([np.sin(Q[..., 1] * 1.3 + Q[..., 2]), np.cos(Q[..., 0] * 0.7 - Q[..., 2] * 1.1), np.sin(Q[..., 0] + Q[..., 1] * 0.9)], -1)
    out = tris.copy()
    M = (P + amplitude * size * D).astype(np.float32)
    for k, v in enumerate(("v1", "v2", "v3")):
        for a, c in enumerate("xyz"):
            out[v]["position"][c] = M[:, k, a]
    return out


def built(arrays):
    scene = host.Scene(arrays=arrays)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items()}


def ms_per_sample(ctx, w, h, samples):
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(host.default_camera(w, h))
    fr.set_max_bounces(4)
    fr.integrate(samples)                                   # warm-up (and the fold adaptation's probe, where one is armed)
    ctx.finish()
    times = []
    for _ in range(3):
        fr.reset()
        t = time.perf_counter()
        fr.integrate(samples)
        ctx.finish()
        times.append((time.perf_counter() - t) / samples)
    fr.close()
    return 1e3 * float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=2_800_000)
    ap.add_argument("--refits", type=int, default=24)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--no-trace", action="store_true", help="skip the trace-time table")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    a = ap.parse_args()
    sc = built(S.city_block(a.triangles))
    tris, nodes = sc["triangles"], sc["nodes"]
    poses = [smooth(tris, 0.002, 0.0), smooth(tris, 0.002, 1.0)]
    result = {"triangles": int(len(tris)), "nodes": int(len(nodes))}

    # the yardstick: upload of a moved scene, option off
    moved_scene = dict(sc, triangles=poses[0], nodes=capi.debug_refit(None, nodes, poses[0])[0])
    ctx = capi.Context(0)
    up = []
    for _ in range(a.uploads):
        t = time.perf_counter()
        ctx.upload_scene(moved_scene)
        ctx.finish()
        up.append(time.perf_counter() - t)
    ctx.close()
    result["upload_s"] = [round(x, 4) for x in up]

    ctx = capi.Context(0)
    ctx.set_refittable(True)
    t = time.perf_counter()
    ctx.upload_scene(sc)
    ctx.finish()
    result["upload_refittable_s"] = round(time.perf_counter() - t, 4)
    bufs = [ctx.create_buffer(p) for p in poses]
    for b in bufs:                                          # warm-up
        ctx.refit_scene(b)
    ctx.finish()
    rf = []
    for k in range(a.refits):
        t = time.perf_counter()
        ctx.refit_scene(bufs[k & 1])
        ctx.finish()
        rf.append(time.perf_counter() - t)
    result["refit_ms"] = {"median": round(1e3 * float(np.median(rf)), 3), "min": round(1e3 * min(rf), 3), "max": round(1e3 * max(rf), 3), "calls": len(rf)}
    result["upload_over_refit"] = round(float(np.median(up)) / float(np.median(rf)), 1)
    result["report"] = ctx.tree_report().splitlines()[-1]
    for b in bufs:
        b.close()

    if not a.no_trace:
        w, h = 1920, 1080
        table = []
        for amplitude in (0.0, 0.002, 0.01, 0.05):
            pose = smooth(tris, amplitude, 0.5) if amplitude else tris
            ctx.refit_scene(pose)
            refitted = ms_per_sample(ctx, w, h, a.samples)
            fresh_scene = built({k: (pose if k == "triangles" else v) for k, v in sc.items() if k not in ("nodes", "env", "lights")})
            fresh = capi.Context(0)
            fresh.upload_scene(fresh_scene)
            rebuilt = ms_per_sample(fresh, w, h, a.samples)
            fresh.close()
            table.append({"amplitude": amplitude, "refitted_ms_per_sample": round(refitted, 3), "rebuilt_ms_per_sample": round(rebuilt, 3)})
        result["trace_1080p"] = table
    ctx.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
