"""What an occlusion bake costs: the 2.8 M-triangle stand-in on the upload's fold (RT_CTX_OPT_ADAPTIVE_FOLD = 0); the points are the
first hits of the frame's 1920 x 1080 camera rays, kept on the device as rt_surface records (rt_scene_trace_buffer) and baked with RT_BAKE_FROM_SURFACES at 64
and 256 rays per point.  End to end: host-clock medians over --calls calls of rt_scene_bake_buffer + rt_finish after a warm-up.  Writes one JSON file.

  python tools/bake_profile.py --out profiles/bake_2p8M.json
  python tools/bake_profile.py --kernel-stats profiles/bake_2p8M_kernel_stats.csv

The second form gives the kernels' OWN times by one clock: per sample count it starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bake_profile.py
--kernels-only SAMPLES` as a fresh child process (no counters in that run).  The child bakes all points --kernel-calls + 1 times (k_bake), then takes the
unfused route over the IDENTICAL rays once: chunk by chunk the device form of rt_debug_bake_rays writes the chunk's rays, point-major, which go into a buffer
and through rt_scene_trace_buffer in any-hit mode (k_query_trace<true>; 2^24 rays per launch, so that the rays of a chunk fit a host array).  Compared are
k_bake's average time per launch and the SUM of k_query_trace<true>'s launches of the one pass; the unfused route's generation and reduction count as zero.
The rows of those kernels go to the CSV with the sample count in a first column; the ratios are added to --out's JSON when it exists."""
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
ap.add_argument("--kernel-calls", type=int, default=5)
ap.add_argument("--radius-fraction", type=float, default=0.02, help="the bake's radius as a fraction of the diagonal of the scene's bounding box")
ap.add_argument("--out", default="profiles/bake_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per sample count and write the measured kernels' statistics here")
ap.add_argument("--kernels-only", type=int, default=None, help="(the child of --kernel-stats) launch both routes at this sample count and leave")
a = ap.parse_args()
SAMPLES = (64, 256)
MEASURED = ("k_bake", "k_query_trace<true>")
CHUNK_RAYS = 1 << 24

if a.kernel_stats:
    rows, header, ratios = [], None, {}
    for samples in SAMPLES:
        head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--kernel-calls", a.kernel_calls, "--radius-fraction", repr(a.radius_fraction),
                                                        "--kernels-only", samples], lambda name: any(k in name for k in MEASURED) and "k_bake_rays" not in name,
                                             ROOT, "bake_profile_")
        header = ["samples"] + head
        col = {name: i for i, name in enumerate(head)}
        t = {}
        for r in kept:
            for k in MEASURED:
                if k in r[0]:
                    rows.append([str(samples)] + r)
                    t[k] = dict(calls=int(r[col["Calls"]]), total_ns=int(r[col["TotalDurationNs"]]), average_ns=float(r[col["AverageNs"]]))
        if len(t) == 2:
            ratios[str(samples)] = dict(k_bake_ms_per_launch=t["k_bake"]["average_ns"] / 1e6, k_bake_launches=t["k_bake"]["calls"],
                                        k_query_trace_any_hit_ms_one_pass=t["k_query_trace<true>"]["total_ns"] / 1e6, k_query_trace_launches=t["k_query_trace<true>"]["calls"],
                                        k_bake_over_k_query_trace=t["k_bake"]["average_ns"] / t["k_query_trace<true>"]["total_ns"])
    kernel_stats.write(a.kernel_stats, header, rows)
    for r in rows:
        print(", ".join(r[:6])[:240])
    print(json.dumps(ratios, indent=1))
    if os.path.exists(a.out):
        out = json.load(open(a.out))
        out["kernels"] = ratios
        if "256" in ratios:
            out["fused_kernel_is_faster_at_256"] = bool(ratios["256"]["k_bake_over_k_query_trace"] < 1.0)
        json.dump(out, open(a.out, "w"), indent=1)
    sys.exit(0)

cfg = bench.CONFIGS[a.config]
w, h = cfg["width"], cfg["height"]
scene, n_tris = bench.build_scene(argparse.Namespace(config=a.config, blob_tris=871_200, ball_tris=20_000), host, S)
scene.build_bvh(); scene.finalize()
arrays = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
p = np.stack([np.stack([arrays["triangles"][v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
diag = float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))
radius, bias = float(np.float32(a.radius_fraction * diag)), float(np.float32(1e-4 * diag))
ctx = capi.Context(0)
ctx.set_adaptive_fold(0)          # the upload's fold for both routes alike
ctx.upload_scene(arrays)
fr = capi.Frame(ctx, w, h)
fr.set_camera(host.default_camera(w, h)); fr.set_max_bounces(cfg["bounces"])
fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 1)
fr.set_option(capi.OPT_TRACE_VARIANT, 8)          # (k_trace2 walks to the queue: none of the measured kernels' names)
fr.reset(); fr.generate_rays(); ctx.finish()
rays, _, _ = fr.read_queue(0, 0)
rays = rays.copy()
n = len(rays)
b_rays, b_surf, b_out = ctx.create_buffer(rays), ctx.create_buffer(np.zeros(n, T.surface)), ctx.create_buffer(np.zeros(n, T.bake_result))
ctx.trace_buffer(b_rays, n, surfaces=b_surf); ctx.finish()
b_rays.close()
median = lambda v: float(np.median(np.asarray(v)))

if a.kernels_only is not None:
    samples = a.kernels_only
    for _ in range(a.kernel_calls + 1):
        ctx.bake_buffer(b_surf, n, b_out, samples, bias=bias, radius=radius, from_surfaces=True); ctx.finish()
    surf = b_surf.read(T.surface, n)
    per = CHUNK_RAYS // samples
    b_chunk, b_occ = ctx.create_buffer(np.zeros(per * samples, T.ray)), ctx.create_buffer(np.zeros(per * samples, np.uint32))
    for first in range(0, n, per):
        chunk = capi.debug_bake_rays(ctx, surf[first:first + per], samples, 0, bias, radius, from_surfaces=True, first_index=first)
        b_chunk.write(chunk.reshape(-1))
        ctx.trace_buffer(b_chunk, chunk.size, any_hit=True, occluded=b_occ); ctx.finish()
    for b in (b_chunk, b_occ, b_surf, b_out):
        b.close()
    fr.close(); ctx.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "device": ctx.device_info()[0], "calls": a.calls, "points": n,
       "radius": radius, "radius_fraction_of_diagonal": a.radius_fraction, "bias": bias, "code_object_sha256": codeobj.code_object_sha256(), "end_to_end": {}}
for samples in SAMPLES:
    for _ in range(2):
        ctx.bake_buffer(b_surf, n, b_out, samples, bias=bias, radius=radius, from_surfaces=True); ctx.finish()
    ms = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        ctx.bake_buffer(b_surf, n, b_out, samples, bias=bias, radius=radius, from_surfaces=True); ctx.finish()
        ms.append(1e3 * (time.perf_counter() - t0))
    got = b_out.read(T.bake_result, n)
    walked = got["unoccluded"] != 0xFFFFFFFF
    partial = walked & (got["unoccluded"] > 0) & (got["unoccluded"] < samples)
    out["end_to_end"][str(samples)] = dict(ms=median(ms), ms_min=float(min(ms)), ms_max=float(max(ms)), mrays_s=float(walked.sum()) * samples / median(ms) / 1e3,
                                           walked_points=int(walked.sum()), partially_occluded_points=int(partial.sum()),
                                           mean_ambient_term=float((got["unoccluded"][walked] / samples).mean()), bytes_in=64 * n, bytes_out=16 * n)
    print("samples %d: %d points (%d walked, %d partially occluded), %.3f ms, %.0f Mrays/s" % (samples, n, walked.sum(), partial.sum(), median(ms),
                                                                                             walked.sum() * samples / median(ms) / 1e3), flush=True)
out["tree_report_line"] = [ln for ln in ctx.tree_report().splitlines() if ln.startswith("ray queries: ")]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
for b in (b_surf, b_out):
    b.close()
fr.close(); ctx.close()
