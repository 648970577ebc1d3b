"""What an all-hits query costs: the frame's own bounce-0 (coherent) and bounce-2 (incoherent) closest-hit queues of the 2.8 M-triangle
stand-in at 1920 x 1080, read back with rt_frame_debug_read_queue, their t_max set to RT_MAX_RENDER_DIST, and handed to rt_scene_trace_all_buffer -- with
max_hits 0 (k_all_hits<false>: the counts alone) and 8 (k_all_hits<true>: the sorted list), on the 4-wide records and on the child-pair records
(RT_CTX_OPT_WIDE_BVH = 0), beside rt_scene_trace_buffer's closest-hit and any-hit queries of the same rays.  Host clock around the call plus rt_finish; medians
over --calls calls after a warm-up.  The upload's fold (RT_CTX_OPT_ADAPTIVE_FOLD = 0).  Writes one JSON file.

  python tools/all_hits_profile.py --out profiles/all_hits_2p8M.json
  python tools/all_hits_profile.py --kernel-stats profiles/all_hits_2p8M_kernel_stats.csv

The second form gives every kernel's OWN time by one clock: per tree and queue it starts `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/all_hits_profile.py --kernels-only TREE,BOUNCE` as a fresh child process -- no counters in that run -- which launches the four kernels --calls + 3 times
each on that queue, and keeps their rows, with the tree and the queue in the first columns.

The condition the wide walk has to earn: k_all_hits on the 4-wide records faster than on the child-pair records, on both queues."""
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
ap.add_argument("--out", default="profiles/all_hits_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and queue and write the measured kernels' statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) TREE,BOUNCE: launch the kernels on this bounce's queue over this tree and leave")
a = ap.parse_args()
MEASURED = ("k_all_hits", "k_query_trace")
TREES = (("wide", 1), ("pairs", 0))

if a.kernel_stats:
    rows, header = [], None
    for tree, _ in TREES:
        for bounce in (0, 2):
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--kernels-only", "%s,%d" % (tree, bounce)],
                                                 lambda name: any(k in name for k in MEASURED) and "surface" not in name, ROOT, "all_hits_profile_")
            header = ["tree", "queue"] + head
            rows += [[tree, "bounce_%d" % bounce] + r for r in kept]
    kernel_stats.write(a.kernel_stats, header, rows)
    for r in rows:
        print(", ".join(r[:7]))
    sys.exit(0)

cfg = bench.CONFIGS[a.config]
w, h = cfg["width"], cfg["height"]
scene, n_tris = bench.build_scene(argparse.Namespace(config=a.config, blob_tris=871_200, ball_tris=20_000), host, S)
scene.build_bvh(); scene.finalize()
arrays = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
median = lambda v: float(np.median(np.asarray(v)))


def context(wide):
    c = capi.Context(0)
    c.set_adaptive_fold(0)            # the upload's fold for every kernel alike
    if not wide:
        c.set_wide_bvh(0)
    c.upload_scene(arrays)
    return c


def queues(ctx, bounces):
    """the frame's incoming closest-hit queue of each bounce, t_max = RT_MAX_RENDER_DIST"""
    fr = capi.Frame(ctx, w, h)
    fr.set_camera(host.default_camera(w, h)); fr.set_max_bounces(cfg["bounces"])
    fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 1)
    out = {}
    for bounce in bounces:
        fr.reset(); fr.generate_rays()
        for b in range(bounce):
            fr.intersect(b); fr.shade(b); fr.intersect_shadow(b)
        ctx.finish()
        rays = fr.read_queue(0, bounce)[0].copy()
        rays["direction"]["w"] = np.float32(20000.0)
        out[bounce] = rays
    fr.close()
    return out


def variants(ctx, rays):
    """name -> a call that enqueues that query over `rays`"""
    n = len(rays)
    b_rays, b_rec = ctx.create_buffer(rays), ctx.create_buffer(np.zeros(n, T.ray_hits))
    b_hits8, b_hits, b_occ = ctx.create_buffer(np.zeros(n * 8, T.hit)), ctx.create_buffer(np.zeros(n, T.hit)), ctx.create_buffer(np.zeros(n, np.uint32))
    return {"k_all_hits<false>": lambda: ctx.trace_all_buffer(b_rays, n, 0, b_rec),
            "k_all_hits<true>": lambda: ctx.trace_all_buffer(b_rays, n, 8, b_rec, hits=b_hits8),
            "k_query_trace<false>": lambda: ctx.trace_buffer(b_rays, n, hits=b_hits),
            "k_query_trace<true>": lambda: ctx.trace_buffer(b_rays, n, any_hit=True, occluded=b_occ)}, (b_rays, b_rec, b_hits8, b_hits, b_occ)


if a.kernels_only is not None:
    tree, bounce = a.kernels_only.split(",")
    ctx = context(dict(TREES)[tree])
    calls, bufs = variants(ctx, queues(ctx, [int(bounce)])[int(bounce)])
    for call in calls.values():
        for _ in range(a.calls + 3):
            call(); ctx.finish()
    for b in bufs:
        b.close()
    ctx.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "code_object_sha256": codeobj.code_object_sha256(), "queues": {}}
records, shared = {}, None
for tree, wide in TREES:
    ctx = context(wide)
    out["device"] = ctx.device_info()[0]
    shared = shared or queues(ctx, (0, 2))          # both trees get the very same arrays: a later frame may fill a shaded queue in another order
    for bounce, rays in shared.items():
        calls, bufs = variants(ctx, rays)
        row = out["queues"].setdefault("bounce_%d" % bounce, {"rays": len(rays)})
        for name, call in calls.items():
            for _ in range(3):
                call(); ctx.finish()
            ms = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                call(); ctx.finish()
                ms.append(1e3 * (time.perf_counter() - t0))
            row["%s_%s_ms" % (name, tree)] = median(ms)
        rec = bufs[1].read(T.ray_hits, len(rays))
        row.update(mean_count=float(rec["count"].mean()), max_count=int(rec["count"].max()), rays_above_8=int((rec["count"] > 8).sum()))
        same = records.setdefault(bounce, rec).tobytes() == rec.tobytes()       # the two trees give the same records
        row["records_equal_across_trees"] = bool(same and row.get("records_equal_across_trees", True))
        print("%s, bounce %d: %d rays, %s" % (tree, bounce, len(rays), ", ".join("%s %.3f ms" % (k, row["%s_%s_ms" % (k, tree)]) for k in calls)), flush=True)
        for b in bufs:
            b.close()
    ctx.close()
for row in out["queues"].values():
    for k in ("k_all_hits<false>", "k_all_hits<true>"):
        row[k + "_wide_over_pairs"] = row[k + "_wide_ms"] / row[k + "_pairs_ms"]
        row[k + "_over_k_query_trace<false>"] = row[k + "_wide_ms"] / row["k_query_trace<false>_wide_ms"]
    row["wide_faster_than_pairs"] = bool(row["k_all_hits<false>_wide_over_pairs"] < 1 and row["k_all_hits<true>_wide_over_pairs"] < 1)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
