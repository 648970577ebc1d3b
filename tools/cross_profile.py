"""What a crossing query costs: the 2.8 M-triangle stand-in on the upload's fold, tools/nearest_profile.py's two point sets --
  near_surface  the first hits of the 1920 x 1080 camera rays pushed 1e-3 of the scene's diagonal along their geometric normals
  far_field     a 128^3 grid over the scene's bounds
-- the probes equilateral triangles of edge --edge (a share of the scene's diagonal, 4e-3) centred on the points, their orientation drawn with a fixed seed.
rt_scene_cross_buffer + rt_finish with max_list 0 and 8 and with RT_CROSS_ANY, on the 4-wide records and, in a second context with RT_CTX_OPT_WIDE_BVH = 0,
on the child-pair records; medians over --calls calls by the host clock after a warm-up, and whether the two trees' records are identical.  The yardstick is
rt_scene_overlap_buffer with max_list 0 on each probe's bounding box (k_region is the parent commit's, unchanged): the cross walk prunes by that box AND the
probe's plane, so it enters no more leaves; the ratio of times is reported beside the ratio of the mean triangles tested by rt_debug_cross_walk and
rt_debug_overlap_walk on every --walk-sample-th probe.  Then rt_scene_cross_self over all triangles: time, members found, probes with count > 8.  Writes
one JSON file.

  python tools/cross_profile.py --out profiles/cross_2p8M.json
  python tools/cross_profile.py --kernel-stats profiles/cross_2p8M_kernel_stats.csv

The second form gives each kernel's OWN time by one clock: per tree and point set it starts `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/cross_profile.py --kernels-only WIDE,SET` as a fresh child process, without counters and under a time limit of its own -- which launches every
variant --calls + 3 times -- and keeps the rows of k_cross and k_region, with the tree and the point set in the first columns."""
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
ap.add_argument("--edge", type=float, default=4e-3, help="the probes' edge as a share of the scene's diagonal")
ap.add_argument("--walk-sample", type=int, default=16, help="the host walks count the triangles tested on every this-many-th probe")
ap.add_argument("--out", default="profiles/cross_2p8M.json")
ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on one child per tree and point set and write the kernels' statistics here")
ap.add_argument("--kernels-only", default=None, help="(the child of --kernel-stats) WIDE,SET: launch the queries on that tree and point set and leave")
ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds a child of --kernel-stats may take")
a = ap.parse_args()
SETS = ("near_surface", "far_field")
VARIANTS = (("count", 0, 0), ("list8", 8, 0), ("any", 0, capi.CROSS_ANY))          # (name, max_list, options)

if a.kernel_stats:
    rows, header = [], None
    for wide in (1, 0):
        for which in SETS:
            head, kept = kernel_stats.child_rows(__file__, ["--config", a.config, "--calls", a.calls, "--grid", a.grid, "--edge", a.edge,
                                                            "--kernels-only", "%d,%s" % (wide, which)],
                                                 lambda name: "k_cross" in name or "k_region" in name, ROOT, "cross_profile_", timeout=a.child_timeout)
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


def probes_about(pos, edge, seed=1):
    """types.probe[n]: an equilateral triangle of that edge centred on each position, in a plane and at an angle drawn with a fixed seed"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    u = np.cross(nrm, rng.normal(size=(n, 3))); u /= np.linalg.norm(u, axis=1)[:, None]
    v = np.cross(nrm, u)
    r = edge / np.sqrt(3.0)                                                  # the circumradius
    C = np.stack([pos + r * (np.cos(t) * u + np.sin(t) * v) for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)], 1)
    return T.probes_from_corners(C)


def boxes_of(probes):
    """types.region[n]: each probe's bounding box (types.box_region's planes, made for all at once)"""
    C = np.stack([probes[k][:, :3] for k in ("p1", "p2", "p3")], 1)
    lo, hi = C.min(1), C.max(1)
    rg = np.zeros(len(probes), T.region)
    rg["num_planes"] = 6
    for k in range(3):
        rg["planes"][:, k, k], rg["planes"][:, k, 3] = -1.0, lo[:, k]
        rg["planes"][:, 3 + k, k], rg["planes"][:, 3 + k, 3] = 1.0, -hi[:, k]
    return rg


def timed(call, calls):
    ms = []
    for k in range(calls + 3):
        t0 = time.perf_counter()
        call()
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    return median(ms)


def timed_cross(c, probes, calls, max_list, options):
    n = len(probes)
    b_pr, b_out = c.create_buffer(probes), c.create_buffer(np.zeros(n, T.probe_hits))
    b_mem = c.create_buffer(np.zeros(n * max_list, T.cross_member)) if max_list else None
    ms = timed(lambda: (c.cross_buffer(b_pr, n, max_list, options, b_out, b_mem), c.finish()), calls)
    got = (b_out.read(T.probe_hits, n), b_mem.read(T.cross_member, n * max_list) if max_list else None)
    for b in (b_pr, b_out, b_mem):
        if b is not None:
            b.close()
    return ms, got


def timed_overlap(c, rg, calls):
    n = len(rg)
    b_rg, b_out = c.create_buffer(rg), c.create_buffer(np.zeros(n, T.region_hits))
    ms = timed(lambda: (c.overlap_buffer(b_rg, n, 0, b_out), c.finish()), calls)
    count = b_out.read(T.region_hits, n)["count"]
    b_rg.close(); b_out.close()
    return ms, count


if a.kernels_only is not None:
    wide, which = a.kernels_only.split(",")
    c = context(int(wide))
    probes = probes_about(positions_of(c, which)[which], a.edge * DIAGONAL)
    for name, max_list, options in VARIANTS:
        timed_cross(c, probes, a.calls, max_list, options)
    timed_overlap(c, boxes_of(probes), a.calls)
    c.close()
    sys.exit(0)

out = {"scene": "config %d stand-in, %d triangles, %d x %d" % (a.config, n_tris, w, h), "calls": a.calls, "code_object_sha256": codeobj.code_object_sha256(),
       "edge_share_of_diagonal": a.edge, "edge": a.edge * DIAGONAL, "points": {}}
results = {}
for wide in (1, 0):
    c = context(wide)
    out["device"] = c.device_info()[0]
    tree = "wide" if wide else "pairs"
    for which, pos in positions_of(c).items():
        row = out["points"].setdefault(which, {"probes": len(pos)})
        probes = probes_about(pos, a.edge * DIAGONAL)
        for name, max_list, options in VARIANTS:
            ms, got = timed_cross(c, probes, a.calls, max_list, options)
            results[(wide, which, name)] = got
            row["%s_%s_ms" % (name, tree)] = ms
            print("%s, %s, %s: %d probes, %.3f ms (%.1f Mprobes/s)" % (tree, which, name, len(probes), ms, len(probes) / ms / 1e3), flush=True)
        row["overlap_box_count_%s_ms" % tree], box_count = timed_overlap(c, boxes_of(probes), a.calls)
        row["count_over_overlap_box_%s" % tree] = row["count_%s_ms" % tree] / row["overlap_box_count_%s_ms" % tree]
        print("%s, %s, overlap of the boxes: %.3f ms; cross / overlap %.3f" % (tree, which, row["overlap_box_count_%s_ms" % tree], row["count_over_overlap_box_%s" % tree]), flush=True)
        if wide:
            count = results[(1, which, "count")][0]["count"]
            row["count_mean"], row["count_largest"], row["box_count_mean"] = float(count.mean()), int(count.max()), float(box_count.mean())
            row["share_with_none"], row["share_above_8"] = float((count == 0).mean()), float((count > 8).mean())
            sample = probes[::a.walk_sample]
            t0 = time.perf_counter()
            _, tested = capi.debug_cross_walk(arrays["nodes"], tris, sample, 0, 0, wide=True, counts=True)
            print("host cross walk of %d probes: %.1f s" % (len(sample), time.perf_counter() - t0), flush=True)
            _, _, tested_box = capi.debug_overlap_walk(arrays["nodes"], tris, boxes_of(sample), 0, wide=True, counts=True)
            row["triangles_tested_mean"], row["overlap_box_triangles_tested_mean"] = float(tested.mean()), float(tested_box.mean())
            row["triangles_tested_over_overlap_box"] = float(tested.mean() / max(tested_box.mean(), 1e-30))
            print("%s: triangles tested per probe %.2f against %.2f for the box" % (which, tested.mean(), tested_box.mean()), flush=True)
    if wide:
        b_out, b_mem = c.create_buffer(np.zeros(n_tris, T.probe_hits)), c.create_buffer(np.zeros(n_tris * 8, T.cross_member))
        c.cross_self_buffer(0, n_tris, 8, 0, b_out, b_mem); c.finish()
        t0 = time.perf_counter()
        c.cross_self_buffer(0, n_tris, 8, 0, b_out, b_mem); c.finish()
        self_ms = 1e3 * (time.perf_counter() - t0)
        rec = b_out.read(T.probe_hits, n_tris)
        out["cross_self"] = {"probes": int(n_tris), "ms": self_ms, "probes_crossing": int((rec["count"] != 0).sum()),
                             "members_found": int(rec["count"].astype(np.int64).sum()), "members_listed": int(rec["stored"].astype(np.int64).sum()),
                             "probes_above_8": int((rec["count"] > 8).sum())}
        print("cross_self:", json.dumps(out["cross_self"]), flush=True)
        b_out.close(); b_mem.close()
    c.close()
same = lambda x, y: bool(x[0].tobytes() == y[0].tobytes() and (x[1] is None or x[1].tobytes() == y[1].tobytes()))
for which, row in out["points"].items():
    for name, _, _ in VARIANTS:
        row["%s_wide_over_pairs" % name] = row["%s_wide_ms" % name] / row["%s_pairs_ms" % name]
        row["%s_records_identical" % name] = same(results[(1, which, name)], results[(0, which, name)])
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
