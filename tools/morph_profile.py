"""What morphing a scene's triangles costs: rt_scene_morph against rt_scene_refit_buffer (the floor it cannot beat), rt_scene_morph_skin against rt_scene_morph
followed by a host round trip (a refit from a host array after the morph: the least a caller without the fused call pays, the read-back and the host's own skinning not counted) and against
rt_scene_skin alone, on the city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles, default options) with scenes.synthetic_morph and
scenes.synthetic_skin, in one session on one device.  Two densities: a face-like one (a few percent of the corners touched) and a dense
one; the target count and the share of corners touched are in the result.  Host clock around each call + rt_finish; a warm-up of every path first.

  python tools/morph_profile.py --out profiles/morph_2p8M.json --kernel-stats profiles/morph_2p8M_kernel_stats.csv

Per-kernel times (k_morph_triangles, k_morph_skin_triangles and k_skin_triangles alone) come from runs of their own: --kernel-stats starts, once per density,
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/morph_profile.py --kernels-only --radius R` as a fresh child process BEFORE this process opens the
device, keeps the child's kernel statistics (the face-like run's under the name given, the dense one's beside it with `_dense` in the name) and puts the three
kernels' average / min / max, their ratios and the bytes yardsticks into the JSON.  The yardstick of a kernel: k_skin_triangles in the same run, scaled by the
bytes moved per triangle -- rest 160 + row 4 + 32 per record at the measured density + 160 written (+ 72 of influences for the fused kernel), over the skin's
160 + 72 + 160.  The fused kernel's second yardstick: the sum of the other two, which it should undercut by about the 320 bytes per triangle it does not write
and read again."""
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

KERNELS = ("k_morph_skin_triangles", "k_morph_triangles", "k_skin_triangles")      # (none of the three names lies inside another)
SKIN_BYTES = 160 + 72 + 160


def built(arrays):
    scene = host.Scene(arrays=arrays)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items()}


def timed(ctx, call, n):
    out = []
    for k in range(n):
        t = time.perf_counter()
        call(k)
        ctx.finish()
        out.append(time.perf_counter() - t)
    return {"median": round(1e3 * float(np.median(out)), 3), "min": round(1e3 * min(out), 3), "max": round(1e3 * max(out), 3), "calls": len(out)}


def kernel_rows(path):
    """{kernel: {calls, average_us, min_us, max_us}} of the three kernels in a rocprofv3 kernel statistics file"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                              "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
                    break
    return out


def kernel_stats(out_csv, a, radius):
    """rocprofv3's kernel statistics of a kernels-only run (a fresh child process, the program after `--`)"""
    tmp = tempfile.mkdtemp(prefix="morph_profile_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--triangles", str(a.triangles), "--calls", str(a.calls), "--targets", str(a.targets), "--bones", str(a.bones), "--radius", repr(radius), "--kernels-only"]
        subprocess.check_call(cmd, cwd=ROOT)
        found = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel statistics under " + tmp)
        shutil.copyfile(found[0], out_csv)
        rows = kernel_rows(out_csv)
        if len(rows) != 3:
            raise SystemExit("the kernel statistics lack one of %s: %s" % (", ".join(KERNELS), out_csv))
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def with_yardsticks(rows, records_per_triangle):
    m, f, s = (rows[k]["average_us"] for k in ("k_morph_triangles", "k_morph_skin_triangles", "k_skin_triangles"))
    morph_bytes = 160 + 4 + 32 * records_per_triangle + 160
    rows["records_per_triangle"] = round(records_per_triangle, 4)
    rows["morph_over_skin"] = round(m / s, 3)
    rows["morph_bytes_yardstick"] = round(morph_bytes / SKIN_BYTES, 3)
    rows["fused_over_skin"] = round(f / s, 3)
    rows["fused_bytes_yardstick"] = round((morph_bytes + 72) / SKIN_BYTES, 3)
    rows["fused_over_sum"] = round(f / (m + s), 3)
    rows["fused_over_sum_bytes_yardstick"] = round((morph_bytes + 72) / (morph_bytes + SKIN_BYTES), 3)
    rows["skin_spread_relative"] = round((rows["k_skin_triangles"]["max_us"] - rows["k_skin_triangles"]["min_us"]) / s, 3)
    return rows


class Case:
    """one context on the stand-in with morph targets of one density and a skin set"""

    def __init__(self, sc, a, radius):
        tris = sc["triangles"]
        self.tris = tris
        self.deltas, self.offsets = T.morph_targets(S.synthetic_morph(tris, a.targets, radius=radius, amplitude=0.002))
        self.records_per_triangle = len(self.deltas) / len(tris)
        self.corners_touched = len(np.unique(self.deltas["corner"])) / (3 * len(tris))
        rng = np.random.default_rng(3)
        self.weights = [rng.uniform(0.1, 1.0, a.targets).astype(np.float32) for _ in (0, 1)]
        self.infl = T.influences(*S.synthetic_skin(tris, a.bones))
        axis, lo, hi = S.skin_extent(tris)
        self.palettes = [S.bend_palette(a.bones, angle, axis, lo, hi) for angle in (0.002, -0.002)]
        self.ctx = capi.Context(0)
        self.ctx.set_refittable(True)
        self.ctx.upload_scene(sc)
        self.ctx.set_morph(self.deltas, self.offsets, len(tris))
        self.ctx.set_skin(self.infl, a.bones)
        self.ctx.finish()
        for k in (0, 1):                                        # warm-up of the three paths
            self.ctx.morph_scene(self.weights[k])
            self.ctx.skin_scene(self.palettes[k])
            self.ctx.morph_skin_scene(self.weights[k], self.palettes[k])
        self.ctx.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=2_800_000)
    ap.add_argument("--targets", type=int, default=48)
    ap.add_argument("--bones", type=int, default=64, help="the skin's palette (staged in LDS)")
    ap.add_argument("--radius", type=float, default=0.008, help="synthetic_morph's radius of the face-like density")
    ap.add_argument("--dense-radius", type=float, default=0.08, help="... and of the dense one")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--kernels-only", action="store_true", help="only the morph, skin and fused loops at --radius (for the kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="first run rocprofv3 on kernels-only children, one per density, and keep their kernel statistics here")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    a = ap.parse_args()
    if a.calls < 20:
        raise SystemExit("--calls: at least 20")
    result = {}
    stats = {}
    if a.kernel_stats:                                          # before this process opens the device
        stem, ext = os.path.splitext(a.kernel_stats)
        stats = {"face": kernel_stats(a.kernel_stats, a, a.radius), "dense": kernel_stats(stem + "_dense" + ext, a, a.dense_radius)}
    sc = built(S.city_block(a.triangles))
    if a.kernels_only:
        case = Case(sc, a, a.radius)
        ctx = case.ctx
        for call in (lambda k: ctx.morph_scene(case.weights[k & 1]), lambda k: ctx.skin_scene(case.palettes[k & 1]),
                     lambda k: ctx.morph_skin_scene(case.weights[k & 1], case.palettes[k & 1])):
            for k in range(a.calls):
                call(k)
                ctx.finish()
        ctx.close()
        return
    result.update({"triangles": int(len(sc["triangles"])), "targets": a.targets, "bones": a.bones, "lds_targets": capi.MORPH_LDS_TARGETS})
    for name, radius in (("face", a.radius), ("dense", a.dense_radius)):
        case = Case(sc, a, radius)
        ctx = case.ctx
        r = {"radius": radius, "deltas": int(len(case.deltas)), "records_per_triangle": round(case.records_per_triangle, 4),
             "share_of_corners_touched": round(case.corners_touched, 4)}
        morphed = [capi.debug_morph(None, case.tris, case.deltas, case.offsets, w) for w in case.weights]
        bufs = [ctx.create_buffer(m) for m in morphed]
        for b in bufs:                                          # warm-up
            ctx.refit_scene(b)
        ctx.finish()
        r["refit_buffer_ms"] = timed(ctx, lambda k: ctx.refit_scene(bufs[k & 1]), a.calls)
        r["morph_ms"] = timed(ctx, lambda k: ctx.morph_scene(case.weights[k & 1]), a.calls)
        r["skin_ms"] = timed(ctx, lambda k: ctx.skin_scene(case.palettes[k & 1]), a.calls)
        r["morph_skin_ms"] = timed(ctx, lambda k: ctx.morph_skin_scene(case.weights[k & 1], case.palettes[k & 1]), a.calls)

        def round_trip(k):                                      # without the fused call: morph, then the triangles skinned elsewhere come back as a host array --
            ctx.morph_scene(case.weights[k & 1])                # 160 bytes per triangle up and a second refit.  A LOWER bound: reading the morphed triangles back
            ctx.finish()                                        # and skinning them on the host are not in it
            ctx.refit_scene(morphed[k & 1])

        r["morph_then_host_round_trip_ms"] = timed(ctx, round_trip, a.calls)
        for b in bufs:
            b.close()
        if name in stats:
            r["kernels"] = with_yardsticks(stats[name], case.records_per_triangle)
        report = ctx.tree_report().splitlines()
        r["report"] = [line for line in report if line.startswith(("morph targets: ", "skinned triangles: "))] + report[-1:]
        ctx.close()
        result[name] = r
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
