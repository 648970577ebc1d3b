"""What a light bake costs next to the occlusion bake: the 2.8 M-triangle stand-in on the upload's fold (RT_CTX_OPT_ADAPTIVE_FOLD = 0);
the points are the first hits of a 1024 x 1024 frame's camera rays (1 Mi), kept on the device as rt_surface records (rt_scene_trace_buffer) and baked with
RT_BAKE_FROM_SURFACES at 64 rays per point.  End to end: host-clock medians, with minimum and maximum, over --calls calls + rt_finish after a warm-up of
  occlusion    rt_scene_bake_buffer, radius = sky_distance: k_bake, the yardstick
  light        rt_scene_light_bake_buffer: sky and lights
  sky_only     ... with RT_LIGHT_BAKE_NO_LIGHTS
  lights_only  ... with RT_LIGHT_BAKE_NO_SKY
  atlas        rt_scene_atlas_bake_light at 2048 x 2048 with scenes.synthetic_atlas (host form: the second UV set goes up, 32 bytes per texel come down)
Writes one JSON file.

  python tools/light_bake_profile.py --out profiles/light_bake_2p8M.json
  python tools/light_bake_profile.py --kernel-stats profiles/light_bake_2p8M_kernel_stats.csv

The second form gives the kernels' OWN times by one clock: it starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/light_bake_profile.py
--kernels-only` as a fresh child process (no counters in that run), which launches the occlusion bake, then the three light forms, --kernel-calls + 1 times
each in that order.  k_bake's and k_bake_light's rows go to the CSV; the ratio of their average times is added to --out's JSON when it exists (k_bake_light's
average is over the three forms: the end-to-end figures separate them)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import kernel_stats
from raytracing_amd import capi, codeobj, host, scenes as S, types as T

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=4)
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--kernel-calls", type=int, default=3)
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--side", type=int, default=1024, help="the pick pass is side x side camera rays")
ap.add_argument("--atlas", type=int, default=2048)
ap.add_argument("--distance-fraction", type=float, default=0.02, help="sky_distance (and the occlusion bake's radius) as a fraction of the diagonal of the scene's bounding box")
ap.add_argument("--out", default="profiles/light_bake_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on a child and write the measured kernels' statistics here")
ap.add_argument("--kernels-only", action="store_true", help="(the child of --kernel-stats) launch the four forms and leave")
a = ap.parse_args()
MEASURED = ("k_bake", "k_bake_light")

if a.kernel_stats:
    head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--kernel-calls", a.kernel_calls, "--samples", a.samples, "--side", a.side,
                                                    "--distance-fraction", repr(a.distance_fraction), "--kernels-only"],
                                         lambda name: "k_bake" in name and "rays" not in name, ROOT, "light_bake_profile_")
    col = {name: i for i, name in enumerate(head)}
    t = {}
    for r in kept:
        key = "k_bake_light" if "k_bake_light" in r[0] else "k_bake"
        t[key] = dict(calls=int(r[col["Calls"]]), total_ns=int(r[col["TotalDurationNs"]]), average_ns=float(r[col["AverageNs"]]))
    kernel_stats.write(a.kernel_stats, head, kept)
    for r in kept:
        print(", ".join(r[:6])[:240])
    if len(t) == 2 and os.path.exists(a.out):
        out = json.load(open(a.out))
        out["kernels"] = dict(t, k_bake_light_over_k_bake=t["k_bake_light"]["average_ns"] / t["k_bake"]["average_ns"])
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(t, indent=1))
    sys.exit(0)

cfg = bench.CONFIGS[a.config]
scene, n_tris = bench.build_scene(argparse.Namespace(config=a.config, blob_tris=871_200, ball_tris=20_000), host, S)
scene.build_bvh(); scene.finalize()
arrays = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
p = np.stack([np.stack([arrays["triangles"][v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
diag = float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))
distance, bias = float(np.float32(a.distance_fraction * diag)), float(np.float32(1e-4 * diag))
ctx = capi.Context(0)
ctx.set_adaptive_fold(0)          # the upload's fold for every form alike
ctx.upload_scene(arrays)
fr = capi.Frame(ctx, a.side, a.side)
fr.set_camera(host.default_camera(a.side, a.side)); fr.set_max_bounces(cfg["bounces"])
fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 1)
fr.set_option(capi.OPT_TRACE_VARIANT, 8)
fr.reset(); fr.generate_rays(); ctx.finish()
rays, _, _ = fr.read_queue(0, 0)
rays = rays.copy()
n = len(rays)
b_rays, b_surf = ctx.create_buffer(rays), ctx.create_buffer(np.zeros(n, T.surface))
b_ao, b_out = ctx.create_buffer(np.zeros(n, T.bake_result)), ctx.create_buffer(np.zeros(n, T.light_bake_result))
ctx.trace_buffer(b_rays, n, surfaces=b_surf); ctx.finish()
b_rays.close()
kw = dict(bias=bias, sky_distance=distance, from_surfaces=True)
FORMS = [("occlusion", lambda: ctx.bake_buffer(b_surf, n, b_ao, a.samples, bias=bias, radius=distance, from_surfaces=True)),
         ("light", lambda: ctx.bake_light_buffer(b_surf, n, b_out, a.samples, **kw)),
         ("sky_only", lambda: ctx.bake_light_buffer(b_surf, n, b_out, a.samples, lights=False, **kw)),
         ("lights_only", lambda: ctx.bake_light_buffer(b_surf, n, b_out, a.samples, sky=False, **kw))]


def leave():
    for b in (b_surf, b_ao, b_out):
        b.close()
    fr.close(); ctx.close()


if a.kernels_only:
    for _, call in FORMS:
        for _ in range(a.kernel_calls + 1):
            call(); ctx.finish()
    leave()
    sys.exit(0)


def timed(call, calls):
    for _ in range(2):
        call(); ctx.finish()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call(); ctx.finish()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


out = {"scene": "config %d stand-in, %d triangles; points: first hits of %d x %d camera rays" % (a.config, n_tris, a.side, a.side), "device": ctx.device_info()[0],
       "calls": a.calls, "points": n, "samples": a.samples, "lights": int(len(arrays["lights"])), "environment": list(arrays["env"].shape[:2]), "sky_distance": distance,
       "distance_fraction_of_diagonal": a.distance_fraction, "bias": bias, "code_object_sha256": codeobj.code_object_sha256(), "end_to_end": {}}
for name, call in FORMS:
    out["end_to_end"][name] = timed(call, a.calls)
    print(name, out["end_to_end"][name], flush=True)
ao, lb = b_ao.read(T.bake_result, n), b_out.read(T.light_bake_result, n)
walked = ao["unoccluded"] != 0xFFFFFFFF
e = out["end_to_end"]
out["walked_points"] = int(walked.sum())
out["unoccluded_sky_rays_per_walked_point"] = float(ao["unoccluded"][walked].mean()) if walked.any() else 0.0
for name in ("light", "sky_only", "lights_only"):
    e[name]["over_occlusion"] = e[name]["ms"] / e["occlusion"]["ms"]
side = a.atlas
uv = S.synthetic_atlas(arrays["triangles"], side, side)
e["atlas"] = dict(timed(lambda: ctx.bake_light_atlas(side, side, a.samples, bias=bias, sky_distance=distance, uv=uv), max(a.calls // 3, 3)), width=side, height=side)
print("atlas", e["atlas"], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
leave()
