"""How RT_FILTER_DESC_DEFAULT (include/rt_hip.h) was chosen: on the Cornell and coverage golden scenes at 128 x 128 with 4 bounces, the
tone-mapped MSE of the filtered 4-spp frame against a 1024-spp frame of the same camera, relative to the unfiltered 4-spp frame's, over a grid
of iterations and sigmas (demodulation on).  Prints one line per setting and the best settings by the mean ratio of the two scenes."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi  # noqa: E402
from tests.conftest import load_golden_scene, GOLDEN  # noqa: E402
from raytracing_amd import host  # noqa: E402


def main():
    env = host.load_hdr(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    g = np.load(os.path.join(GOLDEN, "radiance.npz"))
    ctx = capi.Context(0)
    cases = []
    for key, cam_name in (("cornell", "cornell_64_b4_s2"), ("coverage", "coverage_64_b6_s2")):
        ctx.upload_scene(load_golden_scene(key, env))
        fr = capi.Frame(ctx, 128, 128)
        fr.set_camera(g[cam_name + "/camera"]); fr.set_max_bounces(4)
        fr.integrate(1024)
        ref = fr.resolve()[..., :3].astype(np.float64)
        fr.reset(); fr.integrate(4)
        noisy = fr.resolve()[..., :3]
        ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1)
        e0 = np.mean((noisy[ok] - ref[ok]) ** 2)
        res = {}
        for it, sc, sn, sz in itertools.product((1, 2, 3, 4, 5), (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0), (0.05, 0.1, 0.3, 1.0), (0.1, 0.3, 1.0)):
            out = fr.filter(dict(iterations=it, flags=1, sigma_color=sc, sigma_normal=sn, sigma_depth=sz))[..., :3]
            res[(it, sc, sn, sz)] = np.mean((out[ok] - ref[ok]) ** 2) / e0
        cases.append(res)
        fr.close()
    keys = sorted(cases[0], key=lambda k: np.mean([c[k] for c in cases]))
    for k in keys:
        print("iterations %d sigma_color %.2f sigma_normal %.2f sigma_depth %.2f: MSE ratio cornell %.3f coverage %.3f" % (k + tuple(c[k] for c in cases)))
    d = tuple(capi.FILTER_DEFAULT[k] for k in ("iterations", "sigma_color", "sigma_normal", "sigma_depth"))
    print("filter_sweep: best %s (mean ratio %.3f); the header's defaults %s: cornell %.3f coverage %.3f" %
          (keys[0], np.mean([c[keys[0]] for c in cases]), d, cases[0][d], cases[1][d]))
    ctx.close()


if __name__ == "__main__":
    main()
