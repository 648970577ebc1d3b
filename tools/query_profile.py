"""What a ray query costs: the frame's own bounce-0 (coherent) and bounce-2 (incoherent) closest-hit queues of the 2.8 M-triangle
stand-in at 1920 x 1080, read back with rt_frame_debug_read_queue and handed to rt_scene_trace_buffer -- the same rays through k_query_trace and through
the frame's own kernels: k_trace_w4 (the default variant) and k_trace_v1 (RT_OPT_TRACE_VARIANT = 0, the per-ray loop), timed by RT_OPT_PROFILE_KERNELS.
The query is timed with the host clock around the call plus rt_finish; medians over --calls calls after a warm-up.  Also rt_scene_trace (host arrays) for
1 ray and for 2 M rays, beside the PCIe bytes it moves.  Writes one JSON file.

  python tools/query_profile.py --out profiles/query_2p8M.json
  python tools/query_profile.py --kernel-stats profiles/query_2p8M_kernel_stats.csv

The second form gives every kernel's OWN time by one clock: per queue it starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/query_profile.py
--kernels-only BOUNCE` as a fresh child process -- which walks to the queue with k_trace2 (RT_OPT_TRACE_VARIANT = 8: other kernel names than the ones
measured), then launches the query, k_trace_w4 and k_trace_v1 --calls + 3 times each on that queue, no event brackets -- and keeps the rows of those
kernels (and of k_trace2: with a two-entry stack k_trace_w4's follow-up over its slow-ray list, otherwise the walk), with the queue in a first column."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import kernel_stats
from raytracing_amd import capi, codeobj, host, scenes as S, types as T

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=4)
ap.add_argument("--calls", type=int, default=21)
ap.add_argument("--out", default="profiles/query_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per queue and write the measured kernels' statistics here")
ap.add_argument("--kernels-only", type=int, default=None, help="(the child of --kernel-stats) launch the three kernels on this bounce's queue and leave")
a = ap.parse_args()
MEASURED = ("k_query_trace", "k_trace_w4", "k_trace_v1", "k_trace2")      # k_trace2<., 2>: k_trace_w4's follow-up launch over its slow-ray list; k_trace2<., 10 / 12>: the walk to the queue

if a.kernel_stats:
    rows, header = [], None
    for bounce in (0, 2):
        head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--kernels-only", bounce], lambda name: any(k in name for k in MEASURED),
                                             ROOT, "query_profile_")
        header = ["queue"] + head
        rows += [["bounce_%d" % bounce] + r for r in kept]
    kernel_stats.write(a.kernel_stats, header, rows)
    for r in rows:
        print(", ".join(r[:6]))
    sys.exit(0)

cfg = bench.CONFIGS[a.config]
w, h = cfg["width"], cfg["height"]
scene, n_tris = bench.build_scene(argparse.Namespace(config=a.config, blob_tris=871_200, ball_tris=20_000), host, S)
scene.build_bvh(); scene.finalize()
arrays = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
ctx = capi.Context(0)
ctx.set_adaptive_fold(0)          # the upload's fold for every kernel alike: no probe frame's launches among the measured ones, no exchange of records half way
ctx.upload_scene(arrays)
fr = capi.Frame(ctx, w, h)
fr.set_camera(host.default_camera(w, h)); fr.set_max_bounces(cfg["bounces"])
fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 1)
median = lambda v: float(np.median(np.asarray(v)))


def walk_to(bounce, variant=5):
    """the stage API up to the incoming queue of `bounce`"""
    fr.set_option(capi.OPT_TRACE_VARIANT, variant)
    fr.reset(); fr.generate_rays()
    for b in range(bounce):
        fr.intersect(b); fr.shade(b); fr.intersect_shadow(b)
    ctx.finish()
    fr.set_option(capi.OPT_TRACE_VARIANT, 5)


if a.kernels_only is not None:
    bounce = a.kernels_only
    walk_to(bounce, 8)
    rays, _, _ = fr.read_queue(0, bounce)
    n = len(rays)
    b_rays, b_hits = ctx.create_buffer(rays.copy()), ctx.create_buffer(np.zeros(n, T.hit))
    for _ in range(a.calls + 3):
        ctx.trace_buffer(b_rays, n, hits=b_hits); ctx.finish()
    for variant in (5, 0):
        fr.set_option(capi.OPT_TRACE_VARIANT, variant)
        for _ in range(a.calls + 3):
            fr.intersect(bounce); ctx.finish()
    b_rays.close(); b_hits.close(); fr.close(); ctx.close()
    sys.exit(0)

fr.set_option(capi.OPT_PROFILE, 1)


def frame_kernel_ms(bounce, variant):
    walk_to(bounce)
    fr.set_option(capi.OPT_TRACE_VARIANT, variant)
    for _ in range(3):
        fr.intersect(bounce)
    fr.profile()
    ms = []
    for _ in range(a.calls):
        fr.intersect(bounce)
        p = fr.profile()
        ms.append(p.ms_trace_closest)
    fr.set_option(capi.OPT_TRACE_VARIANT, 5)
    return median(ms)


out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "device": ctx.device_info()[0], "calls": a.calls,
       "code_object_sha256": codeobj.code_object_sha256(), "queues": {}}
for bounce in (0, 2):
    walk_to(bounce)
    rays, _, _ = fr.read_queue(0, bounce)
    rays = rays.copy()
    n = len(rays)
    fr.intersect(bounce)                                                     # the frame's own hits of this very queue (a later walk may fill it in another order)
    frame_hits = fr.read_hits(n).copy()
    b_rays, b_hits = ctx.create_buffer(rays), ctx.create_buffer(np.zeros(n, T.hit))
    for _ in range(3):
        ctx.trace_buffer(b_rays, n, hits=b_hits); ctx.finish()
    ms = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        ctx.trace_buffer(b_rays, n, hits=b_hits); ctx.finish()
        ms.append(1e3 * (time.perf_counter() - t0))
    got = b_hits.read(T.hit, n)
    hit = frame_hits["primitive_id"] != 0xFFFFFFFF
    same = got["primitive_id"].tobytes() == frame_hits["primitive_id"].tobytes() and got[hit].tobytes() == frame_hits[hit].tobytes()   # bc, primitive_id and t of every hit
    q_ms, w4_ms, v1_ms = median(ms), frame_kernel_ms(bounce, 5), frame_kernel_ms(bounce, 0)
    out["queues"]["bounce_%d" % bounce] = dict(rays=n, query_ms=q_ms, query_mrays_s=n / q_ms / 1e3, k_trace_w4_ms=w4_ms, k_trace_v1_ms=v1_ms,
                                               query_over_w4=q_ms / w4_ms, query_over_v1=q_ms / v1_ms, faster_than_v1=bool(q_ms < v1_ms),
                                               hits_equal_the_frames=bool(same))
    print("bounce %d: %d rays, query %.3f ms (%.0f Mrays/s), k_trace_w4 %.3f ms, k_trace_v1 %.3f ms, hits equal the frame's: %s" % (bounce, n, q_ms, n / q_ms / 1e3, w4_ms, v1_ms, same), flush=True)
    big = rays
    b_rays.close(); b_hits.close()
host_rows = {}
for n in (1, 2_000_000):
    r = np.resize(big, n)
    for _ in range(2):
        ctx.trace(r)
    ms = []
    for _ in range(a.calls):
        t0 = time.perf_counter(); ctx.trace(r); ms.append(1e3 * (time.perf_counter() - t0))
    host_rows[str(n)] = dict(ms=median(ms), bytes_to_device=32 * n, bytes_to_host=16 * n)
    print("rt_scene_trace, host arrays, %d rays: %.3f ms (%d bytes up, %d down)" % (n, median(ms), 32 * n, 16 * n), flush=True)
out["rt_scene_trace_host_arrays"] = host_rows
out["tree_report_line"] = [ln for ln in ctx.tree_report().splitlines() if ln.startswith("ray queries: ")]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
fr.close(); ctx.close()
