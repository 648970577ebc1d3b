"""What an overlap query costs: the 2.8 M-triangle stand-in on the upload's fold, tools/nearest_profile.py's two point sets --
  near_surface  the first hits of the 1920 x 1080 camera rays pushed 1e-3 of the scene's diagonal along their geometric normals
  far_field     a 128^3 grid over the scene's bounds
-- the regions axis-aligned cubes centred on the points.  THE EDGE is chosen from measured counts: for every edge of --edges (shares of the scene's
diagonal, largest first) the counting walk runs once on every --edge-sample-th point of both sets, the histogram of `count` is recorded, and the largest edge
whose mean count over both sets lies in [4, 64] is taken (section 7l learnt that 1e-2 of the diagonal meant 625 members per point).  Then
rt_scene_overlap_buffer + rt_finish with max_list 0 and 8 on the 4-wide records and, in a second context with RT_CTX_OPT_WIDE_BVH = 0, on the child-pair
records, beside rt_scene_within_buffer with max_near 0 on the same points with the radius half the cube's space diagonal (the circumscribed sphere, which
visits at least the cube's leaves; k_within is the parent commit's, unchanged); medians over --calls calls by the host clock after a warm-up, whether the
two trees' records are identical, and one rt_frame_pick_rect of the full frame and one of a 64 x 64 rectangle.  Writes one JSON file.

  python tools/region_profile.py --out profiles/region_2p8M.json
  python tools/region_profile.py --kernel-stats profiles/region_2p8M_kernel_stats.csv --edge 2.5e-4

The second form gives each kernel's OWN time by one clock: per tree and point set it starts `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/region_profile.py --kernels-only WIDE,SET` as a fresh child process, without counters and under a time limit of its own -- which launches every
variant --calls + 3 times -- and keeps the rows of k_region and k_within, with the tree and the point set in the first columns.  --edge fixes the edge (the
one the first form chose and wrote into its JSON file) so that the children do not choose it again."""
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
ap.add_argument("--edges", default="4e-3,2e-3,1e-3,5e-4,2.5e-4,1.25e-4", help="the cube edges tried, as shares of the scene's diagonal, largest first")
ap.add_argument("--edge", type=float, default=None, help="the cube's edge as a share of the diagonal: skips the choice")
ap.add_argument("--edge-sample", type=int, default=16, help="the choice measures every this-many-th point")
ap.add_argument("--out", default="profiles/region_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and point set and write the kernels' statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) WIDE,SET: launch the queries on that tree and point set and leave")
ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds a child of --kernel-stats may take")
a = ap.parse_args()
SETS = ("near_surface", "far_field")
VARIANTS = (("count", 0), ("list8", 8))          # (name, max_list)

if a.kernel_stats:
    if a.edge is None:
        sys.exit("--kernel-stats needs --edge (the edge the --out form chose)")
    rows, header = [], None
    for wide in (1, 0):
        for which in SETS:
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--grid", a.grid, "--edge", a.edge,
                                                            "--kernels-only", "%d,%s" % (wide, which)],
                                                 lambda name: "k_region" in name or "k_within" in name, ROOT, "region_profile_", timeout=a.child_timeout)
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
P = np.stack([np.stack([tris[v]["position"][k] for k in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).reshape(-1, 3)
LO, HI = P.min(0), P.max(0)
DIAGONAL = float(np.linalg.norm(HI - LO))


def context(wide):
    c = capi.Context(0)
    c.set_adaptive_fold(0)        # the upload's fold: no exchange of records half way
    if not wide:
        c.set_wide_bvh(0)
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


def cubes(pos, edge):
    """types.region[n]: the axis-aligned cube of that edge about each position (types.box_region's planes, made for all at once)"""
    half = np.float32(0.5 * edge)
    rg = np.zeros(len(pos), T.region)
    rg["num_planes"] = 6
    for k in range(3):
        rg["planes"][:, k, k], rg["planes"][:, k, 3] = -1.0, pos[:, k] - half
        rg["planes"][:, 3 + k, k], rg["planes"][:, 3 + k, 3] = 1.0, -(pos[:, k] + half)
    return rg


def timed(c, rg, calls, max_list):
    n = len(rg)
    b_rg, b_out = c.create_buffer(rg), c.create_buffer(np.zeros(n, T.region_hits))
    b_mem = c.create_buffer(np.zeros(n * max_list, T.region_member)) if max_list else None
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        c.overlap_buffer(b_rg, n, max_list, b_out, b_mem); c.finish()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    got = (b_out.read(T.region_hits, n), b_mem.read(T.region_member, n * max_list) if max_list else None)
    for b in (b_rg, b_out, b_mem):
        if b is not None:
            b.close()
    return median(ms), got


def timed_within(c, pos, radius, calls):
    pts = capi.point_records(pos)
    pts["max_distance"] = np.float32(radius)
    n = len(pts)
    b_pts, b_out = c.create_buffer(pts), c.create_buffer(np.zeros(n, T.point_hits))
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        c.within_buffer(b_pts, n, 0, b_out); c.finish()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    count = b_out.read(T.point_hits, n)["count"]
    b_pts.close(); b_out.close()
    return median(ms), count


def choose_edge(c, sets):
    """the largest edge of --edges whose mean count over both sets' samples lies in [4, 64]; the histograms of every edge tried"""
    tried, chosen = [], None
    for share in [float(x) for x in a.edges.split(",")]:
        row = {"edge_share_of_diagonal": share}
        counts = []
        for which, pos in sets.items():
            count = c.overlap(cubes(pos[::a.edge_sample], share * DIAGONAL), 0)["count"]
            counts.append(count)
            row[which] = {"mean": float(count.mean()), "largest": int(count.max()), "share_with_none": float((count == 0).mean()),
                          "histogram_upper_bounds": [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 1 << 30],
                          "histogram": np.histogram(count, [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 1025, 1 << 31])[0].tolist()}
        row["mean"] = float(np.concatenate(counts).mean())
        tried.append(row)
        print("edge %.3g of the diagonal: mean count %.1f" % (share, row["mean"]), flush=True)
        if chosen is None and 4.0 <= row["mean"] <= 64.0:
            chosen = share
    if chosen is None:
        sys.exit("no edge of --edges gives a mean count in [4, 64]: " + json.dumps([(r["edge_share_of_diagonal"], r["mean"]) for r in tried]))
    return chosen, tried


if a.kernels_only is not None:
    wide, which = a.kernels_only.split(",")
    c = context(int(wide))
    pos = positions_of(c, which)[which]
    edge = a.edge * DIAGONAL
    for name, max_list in VARIANTS:
        timed(c, cubes(pos, edge), a.calls, max_list)
    timed_within(c, pos, 0.5 * np.sqrt(3.0) * edge, a.calls)
    c.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "code_object_sha256": codeobj.code_object_sha256(), "points": {}}
results = {}
for wide in (1, 0):
    c = context(wide)
    out["device"] = c.device_info()[0]
    tree = "wide" if wide else "pairs"
    sets = positions_of(c)
    if wide:
        if a.edge is None:
            a.edge, out["edges_tried"] = choose_edge(c, sets)
        out["edge_share_of_diagonal"], out["edge"] = a.edge, a.edge * DIAGONAL
        out["sphere_radius"] = 0.5 * float(np.sqrt(3.0)) * a.edge * DIAGONAL
    for which, pos in sets.items():
        row = out["points"].setdefault(which, {"regions": len(pos)})
        rg = cubes(pos, a.edge * DIAGONAL)
        for name, max_list in VARIANTS:
            ms, got = timed(c, rg, a.calls, max_list)
            results[(wide, which, name)] = got
            row["%s_%s_ms" % (name, tree)] = ms
            print("%s, %s, %s: %d regions, %.3f ms (%.1f Mregions/s)" % (tree, which, name, len(rg), ms, len(rg) / ms / 1e3), flush=True)
        row["within_sphere_count_%s_ms" % tree], sphere = timed_within(c, pos, out["sphere_radius"], a.calls)
        if wide:
            count = results[(1, which, "count")][0]["count"]
            row["count_mean"], row["count_largest"], row["inside_mean"] = float(count.mean()), int(count.max()), float(results[(1, which, "count")][0]["inside"].mean())
            row["share_with_none"], row["share_above_8"], row["sphere_count_mean"] = float((count == 0).mean()), float((count > 8).mean()), float(sphere.mean())
    if wide:
        fr = capi.Frame(c, w, h)
        fr.set_camera(host.default_camera(w, h))
        for name, rect in (("pick_rect_full_frame_ms", (0, 0, w - 1, h - 1)), ("pick_rect_64x64_ms", (w // 2 - 32, h // 2 - 32, w // 2 + 31, h // 2 + 31))):
            fr.pick_rect(*rect)
            t0 = time.perf_counter()
            _, touching, _ = fr.pick_rect(*rect)
            out[name] = 1e3 * (time.perf_counter() - t0)
            out[name.replace("_ms", "_touching")] = int((touching & 1).sum())
        fr.close()
    c.close()
same = lambda x, y: bool(x[0].tobytes() == y[0].tobytes() and (x[1] is None or x[1].tobytes() == y[1].tobytes()))
for which, row in out["points"].items():
    for name, _ in VARIANTS:
        row["%s_wide_over_pairs" % name] = row["%s_wide_ms" % name] / row["%s_pairs_ms" % name]
        row["%s_wide_is_faster" % name] = bool(row["%s_wide_ms" % name] < row["%s_pairs_ms" % name])
        row["%s_records_identical" % name] = same(results[(1, which, name)], results[(0, which, name)])
    for tree in ("wide", "pairs"):
        row["count_over_within_sphere_%s" % tree] = row["count_%s_ms" % tree] / row["within_sphere_count_%s_ms" % tree]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
