"""What a within query costs: the 2.8 M-triangle stand-in on the upload's fold, tools/nearest_profile.py's two point sets --
  near_surface  the first hits of the 1920 x 1080 camera rays pushed 1e-3 of the scene's diagonal along their geometric normals
  far_field     a 128^3 grid over the scene's bounds
-- every point with the radius 1e-2 of the scene's diagonal, through rt_scene_within_buffer + rt_finish with max_near 0, max_near 8 and RT_WITHIN_K_NEAREST at
k = 8, and rt_scene_nearest_buffer on the same points beside them, on the 4-wide records and, in a second context with RT_CTX_OPT_WIDE_BVH = 0, on the
child-pair records; medians over --calls calls by the host clock after a warm-up, the counts' mean, largest and share above 8, and whether the two trees'
records are identical.  Writes one JSON file.

  python tools/within_profile.py --out profiles/within_2p8M.json
  python tools/within_profile.py --kernel-stats profiles/within_2p8M_kernel_stats.csv

The second form gives each kernel's OWN time by one clock: per tree and point set it starts `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/within_profile.py --kernels-only WIDE,SET` as a fresh child process, without counters and under a time limit of its own -- which launches every
variant --calls + 3 times -- and keeps the rows of k_within and k_nearest, with the tree and the point set in the first columns."""
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
ap.add_argument("--radius", type=float, default=1e-2, help="the radius, as a share of the scene's diagonal")
ap.add_argument("--out", default="profiles/within_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and point set and write the kernels' statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) WIDE,SET: launch the queries on that tree and point set and leave")
ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds a child of --kernel-stats may take")
a = ap.parse_args()
SETS = ("near_surface", "far_field")
VARIANTS = (("count", 0, False), ("list8", 8, False), ("knn8", 8, True))          # (name, max_near, RT_WITHIN_K_NEAREST)

if a.kernel_stats:
    rows, header = [], None
    for wide in (1, 0):
        for which in SETS:
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--grid", a.grid, "--radius", a.radius,
                                                            "--kernels-only", "%d,%s" % (wide, which)],
                                                 lambda name: "k_within" in name or "k_nearest" in name, ROOT, "within_profile_", timeout=a.child_timeout)
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
    """tools/nearest_profile.py's two sets, every point with the radius"""
    tris = arrays["triangles"]
    P = np.stack([np.stack([tris[v]["position"][k] for k in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    diagonal = float(np.linalg.norm(hi - lo))
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
        pos = surf["position"] + surf["geometric_normal"] * np.float32(1e-3 * diagonal)
        sets["near_surface"] = capi.point_records(pos.astype(np.float32))
    if only in (None, "far_field"):
        g = [np.linspace(lo[k], hi[k], a.grid, dtype=np.float32) for k in range(3)]
        sets["far_field"] = capi.point_records(np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3))
    for pts in sets.values():
        pts["max_distance"] = np.float32(a.radius * diagonal)
    return sets


def timed(c, pts, calls, max_near, knn):
    n = len(pts)
    b_pts, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.point_hits))
    b_near = c.create_buffer(np.zeros(n * max_near, T.nearest)) if max_near else None
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        c.within_buffer(b_pts, n, max_near, b_out, near=b_near, k_nearest=knn); c.finish()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    got = (b_out.read(T.point_hits, n), b_near.read(T.nearest, n * max_near) if max_near else None)
    for b in (b_pts, b_out, b_near):
        if b is not None:
            b.close()
    return median(ms), got


def timed_nearest(c, pts, calls):
    n = len(pts)
    b_pts, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.nearest))
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        c.nearest_buffer(b_pts, n, out=b_out); c.finish()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    b_pts.close(); b_out.close()
    return median(ms)


if a.kernels_only is not None:
    wide, which = a.kernels_only.split(",")
    c = context(int(wide))
    pts = point_sets(c, which)[which]
    for name, max_near, knn in VARIANTS:
        timed(c, pts, a.calls, max_near, knn)
    timed_nearest(c, pts, a.calls)
    c.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "radius_share_of_diagonal": a.radius,
       "code_object_sha256": codeobj.code_object_sha256(), "points": {}}
results = {}
for wide in (1, 0):
    c = context(wide)
    out["device"] = c.device_info()[0]
    tree = "wide" if wide else "pairs"
    for which, pts in point_sets(c).items():
        row = out["points"].setdefault(which, {"points": len(pts), "radius": float(pts["max_distance"][0])})
        for name, max_near, knn in VARIANTS:
            ms, got = timed(c, pts, a.calls, max_near, knn)
            results[(wide, which, name)] = got
            row["%s_%s_ms" % (name, tree)] = ms
            print("%s, %s, %s: %d points, %.3f ms (%.1f Mpoints/s)" % (tree, which, name, len(pts), ms, len(pts) / ms / 1e3), flush=True)
        row["nearest_%s_ms" % tree] = timed_nearest(c, pts, a.calls)
        if wide:
            count = results[(1, which, "count")][0]["count"]
            row["count_mean"], row["count_largest"] = float(count.mean()), int(count.max())
            row["share_with_none"], row["share_above_8"] = float((count == 0).mean()), float((count > 8).mean())
    if wide:
        out["tree_report_line"] = [ln for ln in c.tree_report().splitlines() if ln.startswith("ray queries: ")]
    c.close()
same = lambda x, y: bool(x[0].tobytes() == y[0].tobytes() and (x[1] is None or x[1].tobytes() == y[1].tobytes()))
for which, row in out["points"].items():
    for name, _, _ in VARIANTS:
        row["%s_wide_over_pairs" % name] = row["%s_wide_ms" % name] / row["%s_pairs_ms" % name]
        row["%s_wide_is_faster" % name] = bool(row["%s_wide_ms" % name] < row["%s_pairs_ms" % name])
        row["%s_records_identical" % name] = same(results[(1, which, name)], results[(0, which, name)])
        row["%s_over_nearest_wide" % name] = row["%s_wide_ms" % name] / row["nearest_wide_ms"]
    row["knn8_list_equals_list8"] = bool(results[(1, which, "knn8")][1].tobytes() == results[(1, which, "list8")][1].tobytes())
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
