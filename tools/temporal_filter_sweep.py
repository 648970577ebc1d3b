"""How RT_TEMPORAL_FILTER_DESC_DEFAULT (include/rt_hip.h) was chosen: on the Cornell and coverage golden scenes at 128 x 128 with 4 bounces, the
camera moving by a small fixed step per frame for 16 frames, each frame reset and traced with 1 spp, the tone-mapped MSE of the temporally filtered
last frame against a 1024-spp frame of the last camera, relative to the unfiltered last frame's, over a grid of iterations, alphas and sigmas
(demodulation on).  The frames are recorded once and replayed through rt_debug_filter_temporal on the GPU, which is bit for bit what
rt_frame_filter_temporal gives for them.  Prints the best settings by the mean ratio of the two scenes and the header's defaults."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from raytracing_amd import capi, host  # noqa: E402
from tests.conftest import load_golden_scene, GOLDEN  # noqa: E402
from tests.test_gpu_temporal_filter import moving_sequence, replay  # noqa: E402


def mse(a, b, ok):
    return float(np.mean((a[ok][:, :3].astype(np.float64) - b[ok][:, :3]) ** 2))


def main():
    env = host.load_hdr(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    g = np.load(os.path.join(GOLDEN, "radiance.npz"))
    ctx = capi.Context(0)
    grid = list(itertools.product((2, 3, 4, 5), (0.1, 0.2, 0.4), (1.0, 2.0, 4.0, 8.0), (0.05, 0.2), (0.1, 0.5)))
    cases = []
    for key, cam_name in (("cornell", "cornell_64_b4_s2"), ("coverage", "coverage_64_b6_s2")):
        ref, frames, noisy, spatial, denoised = moving_sequence(ctx, load_golden_scene(key, env), g[cam_name + "/camera"])
        ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1) & np.isfinite(denoised).all(-1)
        e0 = mse(noisy, ref, ok)
        print("%s: 1 spp MSE %.3e; rt_frame_filter %.3f, RT_OPT_DENOISER=1 %.3f of it" % (key, e0, mse(spatial, ref, ok) / e0,
                                                                                       mse(denoised, ref, ok) / e0))
        res = {}
        for it, alpha, sl, sn, sz in grid:
            out = replay(ctx, frames, dict(iterations=it, flags=1, alpha_color=alpha, alpha_moments=alpha, sigma_luminance=sl, sigma_normal=sn,
                                           sigma_depth=sz))
            res[(it, alpha, sl, sn, sz)] = mse(out, ref, ok) / e0
        d = capi.TEMPORAL_FILTER_DEFAULT
        dk = (d["iterations"], d["alpha_color"], d["sigma_luminance"], d["sigma_normal"], d["sigma_depth"])
        if dk not in res:
            res[dk] = mse(replay(ctx, frames, None), ref, ok) / e0
        cases.append(res)
    keys = sorted(cases[0], key=lambda k: np.mean([c.get(k, np.inf) for c in cases]))
    for k in keys[:15]:
        print("iterations %d alpha %.2f sigma_l %.1f sigma_n %.2f sigma_z %.2f: MSE ratio cornell %.3f coverage %.3f" % (k + tuple(c[k] for c in cases)))
    print("temporal_filter_sweep: best %s (mean ratio %.3f); the header's defaults %s: cornell %.3f coverage %.3f" %
          (keys[0], np.mean([c[keys[0]] for c in cases]), dk, cases[0][dk], cases[1][dk]))
    ctx.close()


if __name__ == "__main__":
    main()
