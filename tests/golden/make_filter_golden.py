"""Regenerates the filter pins in this directory from the PRODUCT build (librt_hip.so): what the spatial and temporal filters compute today,
recorded so that a change to the order of their operations shows up as a changed bit (the numpy restatements in test_spatial_filter.py and
test_temporal_filter.py agree only within a tolerance).

    python tests/golden/make_filter_golden.py                   # filters.npz: the host restatements (rt_debug_filter*(NULL, ...)); no GPU
    python tests/golden/make_filter_golden.py --frame [--out D]  # filters_frame.npz: one frame's guides and filters on GPU 0

Outputs:
  filters.npz        random inputs (NaN, invalid and demodulation-overflow pixels included) of two image sizes (12 x 20, 7 x 11), and for each the spatial
                     filter's output at iterations 0, 1, 2, 5, 8 and the temporal filter's (image, colour history, moments) at iterations
                     0, 1, 3 with a standing and a moving camera, each with and without RT_FILTER_DEMODULATE
  filters_frame.npz  the Cornell golden scene at 32 x 32: rt_frame_read_guides, rt_frame_filter with the defaults, and three
                     rt_frame_filter_temporal calls with the defaults on a camera that moves between them
"""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from raytracing_amd import capi                          # noqa: E402
from tests.test_temporal_filter import random_case       # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(12, 20), (7, 11)]
SPATIAL_ITERATIONS = (0, 1, 2, 5, 8)
TEMPORAL_ITERATIONS = (0, 1, 3)
FRAME = 32
FRAME_STEP = (0.02, 0.01, -0.01)          # the camera's move between the temporal calls


def inputs(H, W):
    """random_case with a few NaN, infinite and demodulation-overflow pixels among the valid ones"""
    rng = np.random.default_rng(1000 * H + W)
    cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm = random_case(rng, H, W)
    hdr[..., 3] = 1.0                                        # carried through unchanged: a constant keeps the fixture small
    valid = np.argwhere(dep < 20000.0)
    pick = valid[rng.choice(len(valid), 9, replace=False)]
    for k, (y, x) in enumerate(pick):
        if k < 4:
            hdr[y, x, k % 3] = np.nan
        elif k < 5:
            hdr[y, x, 1] = np.inf
        else:                                                # finite h, h / a overflows
            hdr[y, x, :3] = 3e38
            alb[y, x, :3] = 0.002
    return dict(cam=cam, prev=prev, hdr=hdr, alb=alb, nrm=nrm, dep=dep, pnrm=pnrm, pdep=pdep, hc=hc, hm=hm)


def spatial_desc(sig, it, demod):
    return dict(iterations=it, flags=demod, sigma_color=float(sig[0]), sigma_normal=float(sig[1]), sigma_depth=float(sig[2]))


def temporal_desc(par, it, demod):
    keys = ("alpha_color", "alpha_moments", "sigma_luminance", "sigma_normal", "sigma_depth")
    return dict(iterations=it, flags=demod, **{k: float(v) for k, v in zip(keys, par)})


def spatial_cases():
    for H, W in SIZES:
        for it in SPATIAL_ITERATIONS:
            for demod in (0, 1):
                yield "%dx%d" % (H, W), it, demod


def temporal_cases():
    for H, W in SIZES:
        for it in TEMPORAL_ITERATIONS:
            for demod in (0, 1):
                for moving in (0, 1):
                    yield "%dx%d" % (H, W), it, demod, moving


# tests/test_filter_golden.py replays the recorded cases with the three run_* functions below

def run_spatial(ctx, z, tag, it, demod):
    i = {k: z[tag + "/" + k] for k in ("hdr", "alb", "nrm", "dep")}
    return capi.debug_filter(ctx, i["hdr"], i["alb"], i["nrm"], i["dep"], spatial_desc(z[tag + "/spatial_sigmas"], it, demod))


def run_temporal(ctx, z, tag, it, demod, moving):
    i = {k: z[tag + "/" + k] for k in ("cam", "prev", "hdr", "alb", "nrm", "dep", "pnrm", "pdep", "hc", "hm")}
    return capi.debug_filter_temporal(ctx, i["cam"], i["prev"] if moving else None, i["hdr"], i["alb"], i["nrm"], i["dep"], i["pnrm"], i["pdep"],
                                      i["hc"], i["hm"], temporal_desc(z[tag + "/temporal_params"], it, demod))


def make_filters():
    z = {}
    for H, W in SIZES:
        tag = "%dx%d" % (H, W)
        for k, v in inputs(H, W).items():
            z[tag + "/" + k] = v
        z[tag + "/spatial_sigmas"] = np.array([0.7, 0.3, 0.4], np.float32)          # sigma_color, sigma_normal, sigma_depth
        z[tag + "/temporal_params"] = np.array([0.2, 0.3, 4.0, 0.3, 0.4], np.float32)  # alpha_color, alpha_moments, sigma_l, sigma_n, sigma_z
    for tag, it, demod in spatial_cases():
        z["%s/spatial_it%d_d%d" % (tag, it, demod)] = run_spatial(None, z, tag, it, demod)
    for tag, it, demod, moving in temporal_cases():
        out = run_temporal(None, z, tag, it, demod, moving)
        for name, a in zip(("image", "hist", "moments"), out):
            z["%s/temporal_it%d_d%d_m%d/%s" % (tag, it, demod, moving, name)] = a
    path = os.path.join(HERE, "filters.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


def frame_cameras(cam, n=3):
    out = []
    for k in range(n):
        c = np.array(cam, copy=True)
        for i, key in enumerate("xyz"):
            c["position"][key] = np.float32(np.float32(cam["position"][key]) + np.float32(k) * np.float32(FRAME_STEP[i]))
        out.append(c)
    return out


def run_frame(ctx, scene, cam):
    """{name: array} of one frame: guides and rt_frame_filter after 2 samples at cam, then three 1-sample rt_frame_filter_temporal calls"""
    ctx.upload_scene(scene)
    fr = capi.Frame(ctx, FRAME, FRAME)
    fr.set_max_bounces(4)
    fr.set_camera(cam)
    fr.integrate(2)
    alb, nrm, dep, passes = fr.guides()
    out = dict(albedo=alb, normal=nrm, depth=dep, filter=fr.filter())
    for k, c in enumerate(frame_cameras(cam)):
        fr.set_camera(c)
        fr.reset()
        fr.integrate(1)
        out["temporal%d" % k] = fr.filter_temporal()
    fr.close()
    return out


def make_frame(out_dir):
    from tests.conftest import load_golden_scene
    from raytracing_amd import host
    env = host.load_hdr(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene = load_golden_scene("cornell", env)
    cam = np.load(os.path.join(HERE, "radiance.npz"))["cornell_64_b4_s2/camera"]
    ctx = capi.Context(0)
    z = run_frame(ctx, scene, cam)
    ctx.close()
    z["camera"] = cam
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "filters_frame.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true", help="record filters_frame.npz on GPU 0 instead of filters.npz")
    ap.add_argument("--out", default=HERE, help="directory for filters_frame.npz")
    a = ap.parse_args()
    if a.frame:
        make_frame(a.out)
    else:
        make_filters()
