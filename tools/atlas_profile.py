"""What a UV atlas costs: the 2.8 M-triangle stand-in with scenes.synthetic_atlas's second UV set at 2048 x 2048 texels (--size).
End to end, host-clock medians over --calls calls after a warm-up, everything resident in rt_buffers: the cover (rt_scene_atlas_buffer + rt_finish), its
surfaces (rt_scene_atlas_surfaces_buffer), and rt_scene_atlas_bake at --samples rays per texel (host form: 16 bytes per texel come back).  For comparison the
same cover by rt_debug_atlas(NULL) on the host (one call), and rt_scene_bake of the same surfaces from host memory (64 bytes per texel up).  Writes one JSON
file.

  python tools/atlas_profile.py --out profiles/atlas_2p8M.json"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from raytracing_amd import capi, codeobj, host, scenes as S, types as T

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=4)
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--gutter", type=int, default=2)
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--radius-fraction", type=float, default=0.02, help="the bake's radius as a fraction of the diagonal of the scene's bounding box")
ap.add_argument("--out", default="profiles/atlas_2p8M.json")
a = ap.parse_args()

scene, n_tris = bench.build_scene(argparse.Namespace(config=a.config, blob_tris=871_200, ball_tris=20_000), host, S)
scene.build_bvh(); scene.finalize()
arrays = {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}
tris = arrays["triangles"]
p = np.stack([np.stack([tris[v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
diag = float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))
radius, bias = float(np.float32(a.radius_fraction * diag)), float(np.float32(1e-4 * diag))
w = h = a.size
n = w * h
uv = S.synthetic_atlas(tris, w, h)
ctx = capi.Context(0)
ctx.set_adaptive_fold(0)
ctx.upload_scene(arrays)
median = lambda v: float(np.median(np.asarray(v)))


def timed(fn, calls=a.calls, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=median(ms), ms_min=float(min(ms)), ms_max=float(max(ms)))


b_uv, b_tx, b_st, b_sf = ctx.create_buffer(uv), ctx.create_buffer(np.zeros(n, T.texel)), ctx.create_buffer(np.zeros(1, T.atlas_stats)), ctx.create_buffer(np.zeros(n, T.surface))
out = {"scene": "config %d stand-in, %d triangles, synthetic atlas %d x %d (grid %d x %d), gutter %d" % ((a.config, n_tris, w, h) + S.synthetic_atlas_grid(len(tris), w, h) + (a.gutter,)),
       "device": ctx.device_info()[0], "calls": a.calls, "texels": n, "samples": a.samples, "radius": radius, "code_object_sha256": codeobj.code_object_sha256()}
out["cover_device"] = timed(lambda: (ctx.atlas_buffer(w, h, b_tx, a.gutter, uv=b_uv, stats=b_st), ctx.finish()))
out["cover_device_no_gutter"] = timed(lambda: (ctx.atlas_buffer(w, h, b_tx, 0, uv=b_uv, stats=b_st), ctx.finish()))
ctx.atlas_buffer(w, h, b_tx, a.gutter, uv=b_uv, stats=b_st); ctx.finish()
texels, stats = b_tx.read(T.texel, n), b_st.read(T.atlas_stats, 1)[0]
out["stats"] = {k: int(stats[k]) for k in T.atlas_stats.names if k != "reserved"}
out["cover_device"]["mtriangles_s"] = len(tris) / out["cover_device"]["ms"] / 1e3
out["surfaces_device"] = timed(lambda: (ctx.atlas_surfaces_buffer(b_tx, n, b_sf), ctx.finish()))
out["bake_atlas"] = timed(lambda: ctx.bake_atlas(w, h, a.samples, bias=bias, radius=radius, gutter=a.gutter, uv=uv), calls=max(a.calls // 2, 3), warm=1)
walked = int((texels["flags"] != 0).sum())
out["bake_atlas"]["mrays_s"] = walked * a.samples / out["bake_atlas"]["ms"] / 1e3
surfaces = b_sf.read(T.surface, n)
out["bake_of_host_surfaces"] = timed(lambda: ctx.bake(surfaces, a.samples, bias=bias, radius=radius, from_surfaces=True), calls=max(a.calls // 2, 3), warm=1)
t0 = time.perf_counter()
host_texels, host_stats = capi.debug_atlas(None, tris, w, h, a.gutter, uv=uv)
out["cover_host"] = dict(ms=1e3 * (time.perf_counter() - t0), equal_to_device=bool(host_texels.tobytes() == texels.tobytes() and host_stats.tobytes() == stats.tobytes()))
out["tree_report_line"] = [ln for ln in ctx.tree_report().splitlines() if ln.startswith("bakes: ") or ln.startswith("ray queries: ")]
for k in ("cover_device", "cover_device_no_gutter", "surfaces_device", "bake_atlas", "bake_of_host_surfaces", "cover_host"):
    print(k, json.dumps(out[k]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
for b in (b_uv, b_tx, b_st, b_sf):
    b.close()
ctx.close()
