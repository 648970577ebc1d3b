"""What a separation query costs: the 2.8 M-triangle stand-in on the upload's fold, tools/nearest_profile.py's two point sets --
  near_surface  the first hits of the 1920 x 1080 camera rays pushed 1e-3 of the scene's diagonal along their geometric normals
  far_field     a 128^3 grid over the scene's bounds
-- the probes tools/cross_profile.py's equilateral triangles of edge --edge (a share of the scene's diagonal, 4e-3) centred on the points.
rt_scene_separation_buffer + rt_finish with max_distance inf and --radius (a share of the diagonal, 1e-2), on the 4-wide records and, in a second context
with RT_CTX_OPT_WIDE_BVH = 0, on the child-pair records; medians over --calls calls by the host clock after a warm-up, and whether the two trees' records are
identical.  The yardsticks, timed in the same run on kernels this query did not change: rt_scene_nearest_buffer on the probes' centroids (the same
max_distance) and rt_scene_cross_buffer with max_list 0 on the same probes.  The mean triangles handed to a probe at the leaves by rt_debug_separation_walk
on every --walk-sample-th probe stands beside rt_debug_nearest_walk's figure for the centroids (host walks, shared out among threads).  Then
rt_scene_separation_self_buffer with RT_SEPARATION_OTHER_OBJECTS over all triangles, the objects a 16 x 16 grid of cells over the two longest axes: with
--radius, and with inf when a 1/64 sample of the triangles says the whole takes less than --self-limit seconds.  Writes one JSON file.

  python tools/separation_profile.py --out profiles/separation_2p8M.json
  python tools/separation_profile.py --kernel-stats profiles/separation_2p8M_kernel_stats.csv

The second form gives each kernel's OWN time by one clock: per tree and point set it starts `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/separation_profile.py --kernels-only WIDE,SET` as a fresh child process, without counters and under a time limit of its own, and keeps the rows of
k_separation, k_nearest and k_cross, with the tree and the point set in the first columns."""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
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
ap.add_argument("--edge", type=float, default=4e-3, help="the probes' edge as a share of the scene's diagonal")
ap.add_argument("--radius", type=float, default=1e-2, help="the finite max_distance as a share of the scene's diagonal")
ap.add_argument("--walk-sample", type=int, default=16, help="the host walks count the triangles tested on every this-many-th probe")
ap.add_argument("--self-limit", type=float, default=20.0, help="the self form with max_distance inf runs whole only when a 1/64 sample projects fewer seconds than this")
ap.add_argument("--out", default="profiles/separation_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and point set and write the kernels' statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) WIDE,SET: launch the queries on that tree and point set and leave")
ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds a child of --kernel-stats may take")
a = ap.parse_args()
SETS = ("near_surface", "far_field")
INF = float("inf")

if a.kernel_stats:
    rows, header = [], None
    for wide in (1, 0):
        for which in SETS:
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--grid", a.grid, "--edge", a.edge, "--radius", a.radius,
                                                            "--kernels-only", "%d,%s" % (wide, which)],
                                                 lambda name: "k_separation" in name or "k_nearest" in name or "k_cross" in name, ROOT, "separation_profile_",
                                                 timeout=a.child_timeout)
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
tris = arrays["triangles"]
P3 = np.stack([np.stack([tris[v]["position"][k] for k in "xyz"], -1) for v in ("v1", "v2", "v3")], 1)
P = P3.reshape(-1, 3)
LO, HI = P.min(0), P.max(0)
DIAGONAL = float(np.linalg.norm(HI - LO))
RADII = (("inf", INF), ("radius", float(np.float32(a.radius * DIAGONAL))))


def context(wide, refittable=False):
    c = capi.Context(0)
    c.set_adaptive_fold(0)        # the upload's fold: no exchange of records half way
    if not wide:
        c.set_wide_bvh(0)
    if refittable:
        c.set_refittable(True)
    c.upload_scene(arrays)
    return c


def positions_of(c, only=None):
    """tools/nearest_profile.py's two sets: float32[n, 3] each"""
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
        sets["near_surface"] = (surf["position"] + surf["geometric_normal"] * np.float32(1e-3 * DIAGONAL)).astype(np.float32)
    if only in (None, "far_field"):
        g = [np.linspace(LO[k], HI[k], a.grid, dtype=np.float32) for k in range(3)]
        sets["far_field"] = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    return sets


def probes_about(pos, edge, seed=1):
    """tools/cross_profile.py's probes: an equilateral triangle of that edge centred on each position, in a plane and at an angle drawn with a fixed seed"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    u = np.cross(nrm, rng.normal(size=(n, 3))); u /= np.linalg.norm(u, axis=1)[:, None]
    v = np.cross(nrm, u)
    r = edge / np.sqrt(3.0)
    C = np.stack([pos + r * (np.cos(t) * u + np.sin(t) * v) for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)], 1)
    return T.probes_from_corners(C)


def points_of(pos, lim):
    pts = np.zeros(len(pos), T.point)
    pts["position"], pts["max_distance"] = pos, lim
    return pts


def timed(call, calls):
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        call()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    return median(ms)


def timed_separation(c, probes, calls, r):
    n = len(probes)
    b_pr, b_out = c.create_buffer(probes), c.create_buffer(np.zeros(n, T.separation))
    ms = timed(lambda: (c.separation_buffer(b_pr, n, r, 0, b_out), c.finish()), calls)
    got = b_out.read(T.separation, n)
    b_pr.close(); b_out.close()
    return ms, got


def timed_nearest(c, pts, calls):
    n = len(pts)
    b_pt, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.nearest))
    ms = timed(lambda: (c.nearest_buffer(b_pt, n, b_out), c.finish()), calls)
    b_pt.close(); b_out.close()
    return ms


def timed_cross(c, probes, calls):
    n = len(probes)
    b_pr, b_out = c.create_buffer(probes), c.create_buffer(np.zeros(n, T.probe_hits))
    ms = timed(lambda: (c.cross_buffer(b_pr, n, 0, 0, b_out, None), c.finish()), calls)
    b_pr.close(); b_out.close()
    return ms


def shared_out(fn, items, threads=16):
    """fn over `items` in `threads` contiguous pieces on host threads (the host walks take one probe after the other; the library calls release the GIL)"""
    cuts = [len(items) * k // threads for k in range(threads + 1)]
    with ThreadPoolExecutor(threads) as pool:
        return np.concatenate(list(pool.map(lambda k: fn(items[cuts[k]:cuts[k + 1]]), range(threads))))


def centroids(probes):
    return ((probes["p1"][:, :3].astype(np.float64) + probes["p2"][:, :3] + probes["p3"][:, :3]) / 3).astype(np.float32)


if a.kernels_only is not None:
    wide, which = a.kernels_only.split(",")
    c = context(int(wide))
    probes = probes_about(positions_of(c, which)[which], a.edge * DIAGONAL)
    for name, r in RADII:
        timed_separation(c, probes, a.calls, r)
        timed_nearest(c, points_of(centroids(probes), r), a.calls)
    timed_cross(c, probes, a.calls)
    c.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "code_object_sha256": codeobj.code_object_sha256(),
       "edge_share_of_diagonal": a.edge, "edge": a.edge * DIAGONAL, "radius_share_of_diagonal": a.radius, "radius": RADII[1][1], "points": {}}


def save():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


results = {}
for wide in (1, 0):
    c = context(wide)
    out["device"] = c.device_info()[0]
    tree = "wide" if wide else "pairs"
    for which, pos in positions_of(c).items():
        row = out["points"].setdefault(which, {"probes": len(pos)})
        probes = probes_about(pos, a.edge * DIAGONAL)
        cen = centroids(probes)
        row["cross_count_%s_ms" % tree] = timed_cross(c, probes, a.calls)
        for name, r in RADII:
            ms, got = timed_separation(c, probes, a.calls, r)
            results[(wide, which, name)] = got
            row["separation_%s_%s_ms" % (name, tree)] = ms
            row["nearest_%s_%s_ms" % (name, tree)] = timed_nearest(c, points_of(cen, r), a.calls)
            row["separation_over_nearest_%s_%s" % (name, tree)] = ms / row["nearest_%s_%s_ms" % (name, tree)]
            row["separation_over_cross_%s_%s" % (name, tree)] = ms / row["cross_count_%s_ms" % tree]
            print("%s, %s, %s: %d probes, separation %.3f ms, nearest of the centroids %.3f ms (ratio %.2f), cross %.3f ms (ratio %.2f)" % (
                tree, which, name, len(probes), ms, row["nearest_%s_%s_ms" % (name, tree)], row["separation_over_nearest_%s_%s" % (name, tree)],
                row["cross_count_%s_ms" % tree], row["separation_over_cross_%s_%s" % (name, tree)]), flush=True)
            if wide:
                found = got["flags"] & capi.SEPARATION_FOUND != 0
                row["share_found_%s" % name], row["share_crossing_%s" % name] = float(found.mean()), float((got["flags"] & capi.SEPARATION_CROSSING != 0).mean())
                row["distance_mean_%s" % name] = float(got["distance"][found].astype(np.float64).mean()) if found.any() else None
                row["features_%s" % name] = np.bincount(got["feature"][found], minlength=16).tolist()
                sample = probes[::a.walk_sample]
                t0 = time.perf_counter()
                tested = shared_out(lambda pr: capi.debug_separation_walk(arrays["nodes"], tris, pr, r, wide=True, counts=True)[1], sample)
                tested_pt = shared_out(lambda pt: capi.debug_nearest_walk(arrays["nodes"], tris, pt, wide=True, counts=True)[1], points_of(centroids(sample), r))
                row["triangles_tested_mean_%s" % name], row["nearest_triangles_tested_mean_%s" % name] = float(tested.mean()), float(tested_pt.mean())
                row["triangles_tested_largest_%s" % name] = int(tested.max())
                row["triangles_tested_over_nearest_%s" % name] = float(tested.mean() / max(tested_pt.mean(), 1e-30))
                print("%s, %s: triangles tested per probe %.2f (largest %d) against %.2f for the centroid; host walks of %d probes %.1f s" % (
                    which, name, tested.mean(), tested.max(), tested_pt.mean(), len(sample), time.perf_counter() - t0), flush=True)
        save()
    c.close()
for which, row in out["points"].items():
    for name, _ in RADII:
        row["separation_%s_wide_over_pairs" % name] = row["separation_%s_wide_ms" % name] / row["separation_%s_pairs_ms" % name]
        row["separation_%s_records_identical" % name] = bool(results[(1, which, name)].tobytes() == results[(0, which, name)].tobytes())
save()

# the self form with other-objects over all triangles: the objects are a 16 x 16 grid of cells over the two longest axes of the bounds
cen = P3.mean(1)
axes = np.argsort(HI - LO)[1:]
cell = [np.minimum((16 * (cen[:, k] - LO[k]) / max(HI[k] - LO[k], 1e-30)).astype(np.int64), 15) for k in axes]
ids = (cell[0] * 16 + cell[1]).astype(np.uint32)
c = context(1, refittable=True)
c.set_objects(ids, 256)
b_out = c.create_buffer(np.zeros(n_tris, T.separation))
OTHER = capi.SEPARATION_OTHER_OBJECTS


def self_ms(first, n, r):
    c.separation_self_buffer(first, n, r, OTHER, b_out); c.finish()
    t0 = time.perf_counter()
    c.separation_self_buffer(first, n, r, OTHER, b_out); c.finish()
    return 1e3 * (time.perf_counter() - t0)


out["separation_self"] = {"probes": int(n_tris), "objects": 256}
for name, r in (RADII[1], RADII[0]):
    part = n_tris // 64
    part_ms = self_ms(n_tris // 2, part, r)
    entry = {"sample_probes": int(part), "sample_ms": part_ms}
    if part_ms * 64 / 1e3 < a.self_limit:
        entry["ms"] = self_ms(0, n_tris, r)
        rec = b_out.read(T.separation, n_tris)
        found = rec["flags"] & capi.SEPARATION_FOUND != 0
        entry["found"], entry["crossing"] = int(found.sum()), int((rec["flags"] & capi.SEPARATION_CROSSING != 0).sum())
    else:
        entry["ms"] = None                                                # projected above --self-limit: not run whole
    out["separation_self"][name] = entry
    print("separation_self, %s:" % name, json.dumps(entry), flush=True)
    save()
b_out.close()
c.close()
