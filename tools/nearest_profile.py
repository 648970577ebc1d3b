"""What a nearest-point query costs: the 2.8 M-triangle stand-in on the upload's fold, two point sets --
  near_surface  the first hits of the 1920 x 1080 camera rays pushed 1e-3 of the scene's diagonal along their geometric normals (snapping, clearance)
  far_field     a 128^3 grid over the scene's bounds (a distance field)
-- through rt_scene_nearest_buffer + rt_finish on the 4-wide records and, in a second context with RT_CTX_OPT_WIDE_BVH = 0, on the child-pair records; medians
over --calls calls by the host clock after a warm-up, points per second, and whether the two trees' records are identical.  Writes one JSON file.

  python tools/nearest_profile.py --out profiles/nearest_2p8M.json
  python tools/nearest_profile.py --kernel-stats profiles/nearest_2p8M_kernel_stats.csv

The second form gives k_nearest's OWN time by one clock: per tree it starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/nearest_profile.py
--kernels-only WIDE` as a fresh child process, without counters -- which launches the query --calls + 3 times on each point set -- and keeps the rows of
k_nearest, with the tree and the point set in the first columns (the child runs one point set per process, so the rows cannot mix)."""
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
ap.add_argument("--grid", type=int, default=128, help="the far-field set is a grid of this many points per axis")
ap.add_argument("--out", default="profiles/nearest_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and point set and write k_nearest's statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) WIDE,SET: launch the query on that tree and point set and leave")
a = ap.parse_args()
SETS = ("near_surface", "far_field")

if a.kernel_stats:
    rows, header = [], None
    for wide in (1, 0):
        for which in SETS:
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--grid", a.grid, "--kernels-only", "%d,%s" % (wide, which)],
                                                 lambda name: "k_nearest" in name, ROOT, "nearest_profile_")
            header = ["tree", "points"] + head
            rows += [["wide" if wide else "pairs", which] + r for r in kept]
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
    c.set_adaptive_fold(0)        # the upload's fold: no exchange of records half way
    if not wide:
        c.set_wide_bvh(0)
    c.upload_scene(arrays)
    return c


def point_sets(c, only=None):
    tris = arrays["triangles"]
    P = np.stack([np.stack([tris[v]["position"][k] for k in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    sets = {}
    if only in (None, "near_surface"):
        fr = capi.Frame(c, w, h)
        fr.set_camera(host.default_camera(w, h)); fr.set_max_bounces(cfg["bounces"])
        fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 1)
        fr.reset(); fr.generate_rays(); c.finish()
        rays = fr.read_queue(0, 0)[0].copy()
        fr.close()
        _, surf = c.trace(rays, surfaces=True)
        surf = surf[surf["primitive_id"] != 0xFFFFFFFF]
        pos = surf["position"] + surf["geometric_normal"] * np.float32(1e-3 * np.linalg.norm(hi - lo))
        sets["near_surface"] = capi.point_records(pos.astype(np.float32))
    if only in (None, "far_field"):
        g = [np.linspace(lo[k], hi[k], a.grid, dtype=np.float32) for k in range(3)]
        sets["far_field"] = capi.point_records(np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3))
    return sets


def timed(c, pts, calls):
    n = len(pts)
    b_pts, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.nearest))
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        c.nearest_buffer(b_pts, n, out=b_out); c.finish()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    got = b_out.read(T.nearest, n)
    b_pts.close(); b_out.close()
    return median(ms), got


if a.kernels_only is not None:
    wide, which = a.kernels_only.split(",")
    c = context(int(wide))
    timed(c, point_sets(c, which)[which], a.calls)
    c.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "code_object_sha256": codeobj.code_object_sha256(), "points": {}}
results = {}
for wide in (1, 0):
    c = context(wide)
    out["device"] = c.device_info()[0]
    for which, pts in point_sets(c).items():
        ms, got = timed(c, pts, a.calls)
        results[(wide, which)] = got
        row = out["points"].setdefault(which, {"points": len(pts)})
        row["wide_ms" if wide else "pairs_ms"] = ms
        row["wide_mpoints_s" if wide else "pairs_mpoints_s"] = len(pts) / ms / 1e3
        print("%s, %s: %d points, %.3f ms (%.1f Mpoints/s), %d found" % ("4-wide" if wide else "child pairs", which, len(pts), ms, len(pts) / ms / 1e3,
                                                                     int((got["primitive_id"] != 0xFFFFFFFF).sum())), flush=True)
    if wide:
        out["tree_report_line"] = [ln for ln in c.tree_report().splitlines() if ln.startswith("ray queries: ")]
    c.close()
for which, row in out["points"].items():
    row["wide_over_pairs"] = row["wide_ms"] / row["pairs_ms"]
    row["wide_is_faster"] = bool(row["wide_ms"] < row["pairs_ms"])
    row["records_identical"] = bool(results[(1, which)].tobytes() == results[(0, which)].tobytes())
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
