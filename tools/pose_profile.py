"""What posing a scene's objects costs: rt_scene_pose against rt_scene_refit (host array, over PCIe) and rt_scene_refit_buffer (the floor a pose cannot beat), on
the city-block stand-in of bench.py's config 4 (scenes.city_block, ~2.8 M triangles, default options), objects = a few hundred spatial clusters, in one session on
one device.  Host clock around each call + rt_finish; a warm-up of every path first; the medians are what DESIGN quotes.  The expectation
to check against: pose = refit_buffer + one streaming pass (164 bytes read + 160 written per triangle).

  python tools/pose_profile.py --out profiles/pose_2p8M.json

Per-kernel times (k_pose_triangles alone, for its fraction of the streaming rates) come from a run of their own:

  python tools/pose_profile.py --kernel-stats profiles/pose_2p8M_kernel_stats.csv

which starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/pose_profile.py --calls 20 --pose-only` as a fresh child process and keeps its
kernel statistics."""
import argparse
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
from raytracing_amd import capi, host, scenes as S  # noqa: E402

READ_TBPS, WRITE_TBPS = 5.8, 4.7                # calibrated streaming read / write rates
POSE_READ, POSE_WRITE = 164, 160                # bytes per triangle k_pose_triangles moves


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
    """object of every triangle: a cells x cells grid over the two widest axes of the centroids"""
    c = positions(tris).mean(1)
    ax = np.argsort(np.ptp(c, axis=0))[-2:]
    lo, size = c[:, ax].min(0), np.ptp(c[:, ax], axis=0)
    cell = np.minimum(((c[:, ax] - lo) / size * cells).astype(np.int64), cells - 1)
    return (cell[:, 0] * cells + cell[:, 1]).astype(np.uint32), cells * cells


def matrices(n, size, phase):
    """a small translation per object (a thousandth of the scene's extent), different for the two phases; every fifth object stands"""
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


def kernel_stats(out_csv, triangles, calls):
    """rocprofv3's kernel statistics of a pose-only run (a fresh child process, the program after `--`)"""
    tmp = tempfile.mkdtemp(prefix="pose_profile_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--triangles", str(triangles), "--calls", str(calls), "--pose-only"]
        subprocess.check_call(cmd, cwd=ROOT)
        found = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel statistics under " + tmp)
        shutil.copyfile(found[0], out_csv)
        for line in open(out_csv):
            if "k_pose_triangles" in line or "k_refit_triangles" in line:
                print(line.strip())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=2_800_000)
    ap.add_argument("--cells", type=int, default=18, help="objects = cells x cells spatial clusters")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--host-calls", type=int, default=6, help="rt_scene_refit from a host array is slow: fewer calls")
    ap.add_argument("--pose-only", action="store_true", help="only the rt_scene_pose loop (for the kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="run rocprofv3 on a pose-only child and copy its kernel statistics here")
    ap.add_argument("--kernel-us", type=float, default=None, help="k_pose_triangles' average time from the kernel statistics: adds its fraction of the streaming rates")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.triangles, a.calls)
        return
    sc = built(S.city_block(a.triangles))
    tris = sc["triangles"]
    ids, n = clusters(tris, a.cells)
    size = float(np.ptp(positions(tris).reshape(-1, 3), axis=0).max())
    mats = [matrices(n, size, 0), matrices(n, size, 1)]
    result = {"triangles": int(len(tris)), "objects": int(n)}

    ctx = capi.Context(0)
    ctx.set_refittable(True)
    ctx.upload_scene(sc)
    ctx.set_objects(ids, n)
    ctx.finish()
    for m in mats:                                          # warm-up
        ctx.pose_scene(m)
    ctx.finish()
    if not a.pose_only:
        poses = [capi.debug_pose(None, tris, ids, m) for m in mats]
        ctx.refit_scene(poses[0])                           # warm-up
        result["refit_host_array_ms"] = timed(ctx, lambda k: ctx.refit_scene(poses[k & 1]), a.host_calls)
        bufs = [ctx.create_buffer(p) for p in poses]
        for b in bufs:
            ctx.refit_scene(b)
        ctx.finish()
        result["refit_buffer_ms"] = timed(ctx, lambda k: ctx.refit_scene(bufs[k & 1]), a.calls)
        for b in bufs:
            b.close()
    result["pose_ms"] = timed(ctx, lambda k: ctx.pose_scene(mats[k & 1]), a.calls)
    report = ctx.tree_report().splitlines()
    result["report"] = [line for line in report if line.startswith("posed objects: ")] + report[-1:]
    ctx.close()
    stream_us = 1e6 * len(tris) * (POSE_READ / (READ_TBPS * 1e12) + POSE_WRITE / (WRITE_TBPS * 1e12))
    result["k_pose_triangles_streaming_floor_us"] = round(stream_us, 1)
    if a.kernel_us:
        result["k_pose_triangles_us"] = a.kernel_us
        result["k_pose_triangles_fraction_of_streaming_rates"] = round(stream_us / a.kernel_us, 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
