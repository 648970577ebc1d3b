"""What skinning a scene's triangles costs: rt_scene_skin against rt_scene_pose on the same scene and rt_scene_refit_buffer (the floor neither can beat), on the
city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles, default options) with scenes.synthetic_skin, in one session on one device
(DESIGN.md section 7p).  Two palette sizes: 64 bones (staged in LDS) and one above capi.SKIN_LDS_BONES (gathered through L1 / L2).  Host clock around each call
+ rt_finish; a warm-up of every path first; the medians are what DESIGN quotes.

  python tools/skin_profile.py --out profiles/skin_2p8M.json --kernel-stats profiles/skin_2p8M_kernel_stats.csv

Per-kernel times (k_skin_triangles and k_pose_triangles alone) come from runs of their own: --kernel-stats starts, once per palette size,
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/skin_profile.py --kernels-only --bones N` as a fresh child process BEFORE this process opens the device,
keeps the child's kernel statistics (the 64-bone run's under the name given, the large palette's beside it with `_bonesN` in the name) and puts both kernels'
average / min / max and their ratio into the JSON.  The yardstick: k_pose_triangles in the same run, scaled by the bytes moved per triangle,
(160 + 72 + 160) / (160 + 4 + 160) = 1.21."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host, scenes as S, types as T  # noqa: E402

SKIN_BYTES, POSE_BYTES = 160 + 72 + 160, 160 + 4 + 160      # per triangle: rest + influences (object index) + staged


def positions(tris):
    return np.stack([np.stack([tris[v]["position"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1)


def built(arrays):
    scene = host.Scene(arrays=arrays)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items()}


def clusters(tris, cells):
    """object of every triangle: a cells x cells grid over the two widest axes of the centroids (tools/pose_profile.py's)"""
    c = positions(tris).mean(1)
    ax = np.argsort(np.ptp(c, axis=0))[-2:]
    lo, size = c[:, ax].min(0), np.ptp(c[:, ax], axis=0)
    cell = np.minimum(((c[:, ax] - lo) / size * cells).astype(np.int64), cells - 1)
    return (cell[:, 0] * cells + cell[:, 1]).astype(np.uint32), cells * cells


def pose_matrices(n, size, phase):
    rng = np.random.default_rng(11 + phase)
    m = np.zeros((n, 3, 4), np.float32)
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1.0
    m[:, :, 3] = (rng.normal(size=(n, 3)) * 0.001 * size).astype(np.float32)
    m[::5, :, 3] = 0.0
    return m


def timed(ctx, call, n):
    out = []
    for k in range(n):
        t = time.perf_counter()
        call(k)
        ctx.finish()
        out.append(time.perf_counter() - t)
    return {"median": round(1e3 * float(np.median(out)), 3), "min": round(1e3 * min(out), 3), "max": round(1e3 * max(out), 3), "calls": len(out)}


def kernel_rows(path):
    """{kernel: {calls, average_us, min_us, max_us}} of k_skin_triangles and k_pose_triangles in a rocprofv3 kernel statistics file"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in ("k_skin_triangles", "k_pose_triangles"):
                if k in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                              "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def kernel_stats(out_csv, triangles, calls, bones):
    """rocprofv3's kernel statistics of a kernels-only run (a fresh child process, the program after `--`)"""
    tmp = tempfile.mkdtemp(prefix="skin_profile_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--triangles", str(triangles), "--calls", str(calls), "--bones", str(bones), "--kernels-only"]
        subprocess.check_call(cmd, cwd=ROOT)
        found = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel statistics under " + tmp)
        shutil.copyfile(found[0], out_csv)
        rows = kernel_rows(out_csv)
        if len(rows) != 2:
            raise SystemExit("the kernel statistics lack k_skin_triangles or k_pose_triangles: " + out_csv)
        s, p = rows["k_skin_triangles"], rows["k_pose_triangles"]
        rows["skin_over_pose"] = round(s["average_us"] / p["average_us"], 3)
        rows["bytes_yardstick"] = round(SKIN_BYTES / POSE_BYTES, 3)
        rows["pose_spread_relative"] = round((p["max_us"] - p["min_us"]) / p["average_us"], 3)
        print(bones, "bones:", json.dumps(rows))
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


COUNTERS = ["SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_VALU", "SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES"]


def counters(out_csv, triangles, calls, bones):
    """a counter run of its own (no tracing beside it): rocprofv3 --pmc on a kernels-only child; keeps the per-dispatch rows of the two kernels and returns each
    counter's mean per launch"""
    tmp = tempfile.mkdtemp(prefix="skin_profile_")
    try:
        cmd = ["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                                                   "--triangles", str(triangles), "--calls", str(calls), "--bones", str(bones), "--kernels-only"]
        subprocess.check_call(cmd, cwd=ROOT)
        found = sorted(glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True))
        if not found:
            raise SystemExit("rocprofv3 wrote no counter collection under " + tmp)
        sums, kept = {}, []
        with open(found[0], newline="") as f:
            reader = csv.DictReader(f)
            for row in reader:
                for k in ("k_skin_triangles", "k_pose_triangles"):
                    if k in row["Kernel_Name"]:
                        kept.append(row)
                        tot = sums.setdefault(k, {}).setdefault(row["Counter_Name"], [0.0, 0])
                        tot[0] += float(row["Counter_Value"]); tot[1] += 1
            names = reader.fieldnames
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, names)
            w.writeheader()
            w.writerows(kept)
        out = {k: {c: round(v[0] / v[1], 1) for c, v in per.items()} for k, per in sums.items()}
        print(bones, "bones, counters per launch:", json.dumps(out))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


class Case:
    """one context on the stand-in with objects and a skin of `bones` bones set"""

    def __init__(self, sc, bones, cells):
        tris = sc["triangles"]
        self.tris, self.bones = tris, bones
        self.ids, self.n_objects = clusters(tris, cells)
        size = float(np.ptp(positions(tris).reshape(-1, 3), axis=0).max())
        self.pose_mats = [pose_matrices(self.n_objects, size, 0), pose_matrices(self.n_objects, size, 1)]
        self.infl = T.influences(*S.synthetic_skin(tris, bones))
        axis, lo, hi = S.skin_extent(tris)
        self.palettes = [S.bend_palette(bones, a, axis, lo, hi) for a in (0.002, -0.002)]
        self.ctx = capi.Context(0)
        self.ctx.set_refittable(True)
        self.ctx.upload_scene(sc)
        self.ctx.set_objects(self.ids, self.n_objects)
        self.ctx.set_skin(self.infl, bones)
        self.ctx.finish()
        for k in (0, 1):                                        # warm-up of both paths
            self.ctx.skin_scene(self.palettes[k])
            self.ctx.pose_scene(self.pose_mats[k])
        self.ctx.finish()

    def set_bones(self, bones):
        """the same context with another palette size (rt_scene_set_skin replaces the table; the rest pose is made from the scene as the identity left it)"""
        self.ctx.skin_scene(np.stack([np.eye(3, 4, dtype=np.float32)] * self.bones))
        self.bones = bones
        self.infl = T.influences(*S.synthetic_skin(self.tris, bones))
        axis, lo, hi = S.skin_extent(self.tris)
        self.palettes = [S.bend_palette(bones, a, axis, lo, hi) for a in (0.002, -0.002)]
        self.ctx.set_skin(self.infl, bones)
        for k in (0, 1):
            self.ctx.skin_scene(self.palettes[k])
        self.ctx.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=2_800_000)
    ap.add_argument("--cells", type=int, default=18, help="objects = cells x cells spatial clusters (rt_scene_pose's side)")
    ap.add_argument("--bones", type=int, default=64, help="the palette staged in LDS")
    ap.add_argument("--large-bones", type=int, default=1024, help="a palette above capi.SKIN_LDS_BONES, gathered through L1 / L2")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--kernels-only", action="store_true", help="only the rt_scene_skin and rt_scene_pose loops at --bones (for the kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="first run rocprofv3 on kernels-only children, one per palette size, and keep their kernel statistics here")
    ap.add_argument("--counters", default=None, help="also run rocprofv3 --pmc (LDS conflicts, VALU instructions, waits) on a kernels-only child of its own and keep the two kernels' rows here")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    a = ap.parse_args()
    if a.calls < 20:
        raise SystemExit("--calls: at least 20")
    if not a.kernels_only and not a.bones <= capi.SKIN_LDS_BONES < a.large_bones:
        raise SystemExit("--bones must be at most %d and --large-bones above it" % capi.SKIN_LDS_BONES)
    result = {}
    if a.kernel_stats:                                          # before this process opens the device
        stem, ext = os.path.splitext(a.kernel_stats)
        result["kernels"] = {"bones_%d" % a.bones: kernel_stats(a.kernel_stats, a.triangles, a.calls, a.bones),
                             "bones_%d" % a.large_bones: kernel_stats("%s_bones%d%s" % (stem, a.large_bones, ext), a.triangles, a.calls, a.large_bones)}
    if a.counters:
        result["counters_per_launch_bones_%d" % a.bones] = counters(a.counters, a.triangles, a.calls, a.bones)
    sc = built(S.city_block(a.triangles))
    case = Case(sc, a.bones, a.cells)
    ctx = case.ctx
    if a.kernels_only:
        for k in range(a.calls):
            ctx.skin_scene(case.palettes[k & 1])
            ctx.finish()
        for k in range(a.calls):
            ctx.pose_scene(case.pose_mats[k & 1])
            ctx.finish()
        ctx.close()
        return
    result.update({"triangles": int(len(case.tris)), "objects": int(case.n_objects), "lds_bones": capi.SKIN_LDS_BONES})
    skinned = [capi.debug_skin(None, case.tris, case.infl, p) for p in case.palettes]
    bufs = [ctx.create_buffer(p) for p in skinned]
    for b in bufs:                                              # warm-up
        ctx.refit_scene(b)
    ctx.finish()
    result["refit_buffer_ms"] = timed(ctx, lambda k: ctx.refit_scene(bufs[k & 1]), a.calls)
    for b in bufs:
        b.close()
    result["pose_ms"] = timed(ctx, lambda k: ctx.pose_scene(case.pose_mats[k & 1]), a.calls)
    result["skin_ms_bones_%d" % a.bones] = timed(ctx, lambda k: ctx.skin_scene(case.palettes[k & 1]), a.calls)
    case.set_bones(a.large_bones)
    result["skin_ms_bones_%d" % a.large_bones] = timed(ctx, lambda k: ctx.skin_scene(case.palettes[k & 1]), a.calls)
    report = ctx.tree_report().splitlines()
    result["report"] = [line for line in report if line.startswith(("posed objects: ", "skinned triangles: "))] + report[-1:]
    ctx.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
