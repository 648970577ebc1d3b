"""-m gpu: the temporal filter (rt_frame_filter_temporal, rt_frame_read_filter_history, rt_frame_filter_history_reset, rt_debug_filter_temporal;
raytracing_amd/csrc/temporal_filter.h).  The kernels equal the host restatement bit for bit, a frame's moving-camera sequence equals the host
restatement fed with each call's inputs, alpha 1 with zero iterations is rt_frame_resolve bit for bit, the refusals hold, and on a moving camera's
one-sample frames the filter beats the unfiltered frame, the spatial filter and the reference's temporal denoiser."""
import numpy as np
import pytest

from raytracing_amd import capi
from tests.test_gpu_spatial_filter import stage_sample
from tests.test_temporal_filter import random_case

pytestmark = pytest.mark.gpu
MAX_DIST = 20000.0
STEP = (0.005, 0.0, 0.0)          # the sweep's camera step per frame (a fifth of a pixel at the back wall, 128 x 128)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, NaN for NaN (a NaN's payload may differ between numpy and the device)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a)), bits(np.where(nb, 0, b)))


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (23, 41), (1080, 1920)])
def test_kernels_equal_host_restatement_bit_for_bit(ctx, shape):
    rng = np.random.default_rng(shape[0] + 11 * shape[1])
    args = list(random_case(rng, *shape))
    args[2][rng.random(shape) < 0.001, 0] = np.nan
    big = shape[0] > 100
    for it in ((0, 5, 8) if big else range(0, 9)):
        for demod in (0, 1):
            for standing in ((False, True) if big or it % 2 == 0 else (False,)):
                a = list(args)
                if standing:
                    a[1] = None
                desc = dict(iterations=it, flags=demod, alpha_color=float(rng.uniform(0.0, 0.5)), alpha_moments=float(rng.uniform(0.0, 0.5)),
                            sigma_luminance=float(rng.uniform(0.5, 8.0)), sigma_normal=float(rng.uniform(0.05, 1.0)),
                            sigma_depth=float(rng.uniform(0.05, 1.0)))
                dev = capi.debug_filter_temporal(ctx, *a, desc)
                ref = capi.debug_filter_temporal(None, *a, desc)
                for d, r, what in zip(dev, ref, ("image", "colour history", "moments")):
                    assert np.array_equal(bits(d), bits(r)), (it, demod, standing, what, int((bits(d) != bits(r)).sum()))


def moving_cameras(cam, n, step=STEP):
    """cam moved by k * step for k = 0 .. n-1 (float32, as rt_render --camera_step computes it)"""
    out = []
    for k in range(n):
        c = np.array(cam, copy=True)
        for i, key in enumerate("xyz"):
            c["position"][key] = np.float32(np.float32(cam["position"][key]) + np.float32(k) * np.float32(step[i]))
        out.append(c)
    return out


def tonemap(x):
    out = np.array(x, np.float32, copy=True)
    out[..., :3] = out[..., :3] / (out[..., :3] + np.float32(1.0))
    out[..., 3] = 1.0
    return out


def test_frame_sequence_equals_host_restatement(ctx, golden_scenes, golden_radiance):
    ctx.upload_scene(golden_scenes["coverage"])
    cams = moving_cameras(golden_radiance["coverage_64_b6_s2/camera"], 12, (0.01, 0.004, -0.003))
    cams[6] = cams[5]                                        # a standing step: the identity reprojection
    fr = capi.Frame(ctx, 64, 48)
    fr.set_max_bounces(4)
    desc = dict(iterations=3, flags=capi.FILTER_DEMODULATE, alpha_color=0.2, alpha_moments=0.3, sigma_luminance=4.0, sigma_normal=0.1,
                sigma_depth=0.2)
    prev = None
    for k, cam in enumerate(cams):
        fr.set_camera(cam)
        fr.reset()
        fr.integrate(1)
        hdr = fr.radiance() / np.float32(fr.sample_count())
        alb, nrm, dep, _ = fr.guides()
        hc, hm = fr.filter_history()
        got = fr.filter_temporal(desc)
        if prev is None:
            want = capi.debug_filter_temporal(None, cam, None, hdr, alb, nrm, dep, nrm, dep, hc, np.zeros_like(hm), desc)
        else:
            want = capi.debug_filter_temporal(None, cam, prev[0], hdr, alb, nrm, dep, prev[1], prev[2], hc, hm, desc)
        assert same(got, tonemap(want[0])), k
        hc2, hm2 = fr.filter_history()
        assert np.array_equal(bits(hc2), bits(want[1])) and np.array_equal(bits(hm2), bits(want[2])), k
        prev = (cam, nrm, dep)
    L = hm2[..., 2]
    assert L.max() >= 6 and (L == 1).any()                   # long histories and disocclusions
    fr.close()


def check_identity(fr):
    rad = fr.radiance()
    want = fr.resolve()
    got = fr.filter_temporal(dict(iterations=0, alpha_color=1.0, alpha_moments=1.0))
    assert np.array_equal(bits(got), bits(want))
    fr.filter_temporal()                                     # the default filter leaves the frame's own state alone
    assert np.array_equal(bits(fr.radiance()), bits(rad))
    assert np.array_equal(bits(fr.filter_temporal(dict(iterations=0, alpha_color=1.0))), bits(fr.resolve()))


@pytest.mark.parametrize("path", ["integrate_in_flight", "samples_ahead", "frame_kernel", "after_reset"])
def test_alpha_1_zero_iterations_is_resolve_bit_for_bit(ctx, golden_scenes, golden_radiance, path):
    ctx.upload_scene(golden_scenes["coverage"])
    cam = golden_radiance["coverage_64_b6_s2/camera"]
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(cam); fr.set_max_bounces(4)
    if path == "integrate_in_flight":
        fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 4)
        fr.integrate(7)
    elif path == "samples_ahead":
        fr.set_option(capi.OPT_SAMPLES_AHEAD, 4)
        for _ in range(9):
            stage_sample(fr, 4)
        assert fr.stats().samples_from_banks > 0
    elif path == "frame_kernel":
        fr.set_option(capi.OPT_FRAME_KERNEL, 1)
        for _ in range(3):
            stage_sample(fr, 4)
        assert fr.stats().frame_kernel_samples > 0
    else:
        fr.integrate(3)
        fr.filter_temporal()
        fr.reset()
        fr.integrate(2)
    check_identity(fr)
    fr.close()


def check_fresh_history(fr):
    _, _, dep, _ = fr.guides()
    hdr = fr.radiance()
    valid = (dep < MAX_DIST) & np.isfinite(hdr[..., :3]).all(-1)
    L = fr.filter_history()[1][..., 2]
    assert (L[valid] == 1).all() and (L[~valid] == 0).all()


def test_refusals_and_history_drops(ctx, golden_scenes, golden_radiance):
    ctx.upload_scene(golden_scenes["cornell"])
    cam = golden_radiance["cornell_64_b4_s2/camera"]
    tile = capi.Frame(ctx, 64, 64, tile_rank=0, tile_count=2, band_height=8)
    tile.set_camera(cam)
    tile.integrate(1)
    with pytest.raises(capi.RtError, match="whole image"):
        tile.filter_temporal()
    tile.close()
    fr = capi.Frame(ctx, 64, 64)
    fr.set_camera(cam); fr.set_max_bounces(4)
    fr.integrate(1)
    for opt, name in ((capi.OPT_AOV, "RT_OPT_AOV"), (capi.OPT_DENOISER, "RT_OPT_DENOISER")):
        fr.set_option(opt, 1)
        with pytest.raises(capi.RtError, match=name):
            fr.filter_temporal()
        fr.set_option(opt, 0)
    for bad in (dict(iterations=9), dict(alpha_color=1.5), dict(alpha_moments=-0.5), dict(sigma_luminance=0.0), dict(flags=4)):
        with pytest.raises(capi.RtError, match="rt_frame_filter_temporal"):
            fr.filter_temporal(bad)
    assert (fr.filter_history()[1] == 0).all()              # refusals made no history
    for _ in range(3):
        fr.integrate(1)
        fr.filter_temporal()
    assert fr.filter_history()[1][..., 2].max() == 3
    fr.filter_history_reset()
    assert (fr.filter_history()[1] == 0).all()
    fr.filter_temporal()
    check_fresh_history(fr)
    fr.filter_temporal()
    assert fr.filter_history()[1][..., 2].max() == 2
    ctx.upload_scene(golden_scenes["cornell"])
    fr.integrate(1)
    fr.filter_temporal()
    check_fresh_history(fr)
    fr.close()


def tonemapped_mse(a, b, ok):
    return float(np.mean((a[ok][:, :3].astype(np.float64) - b[ok][:, :3]) ** 2))


def moving_sequence(ctx, scene, cam, n=16, w=128, h=128, bounces=4, step=STEP):
    """the sweep's setup: n frames of 1 spp, each reset, the camera moving by `step` per frame.  Returns (reference 1024 spp at the last
    camera, the frames' radiance / guides, the last 1-spp frame, the spatial filter's default on it, the reference's denoiser after n frames)"""
    ctx.upload_scene(scene)
    cams = moving_cameras(cam, n, step)
    fr = capi.Frame(ctx, w, h)
    fr.set_max_bounces(bounces)
    fr.set_camera(cams[-1])
    fr.integrate(1024)
    ref = fr.resolve()
    frames = []
    for c in cams:
        fr.set_camera(c)
        fr.reset()
        fr.integrate(1)
        alb, nrm, dep, _ = fr.guides()
        frames.append((c, fr.radiance(), alb, nrm, dep))
    noisy, spatial = fr.resolve(), fr.filter()
    fr.close()
    dn = capi.Frame(ctx, w, h)
    dn.set_max_bounces(bounces)
    dn.set_option(capi.OPT_DENOISER, 1)
    for c in cams:
        dn.set_camera(c)
        dn.reset()
        stage_sample(dn, bounces, aovs=True)
    denoised = dn.resolve()
    dn.close()
    return ref, frames, noisy, spatial, denoised


def replay(ctx, frames, desc):
    """the temporal filter over recorded frames through rt_debug_filter_temporal: what rt_frame_filter_temporal gives for them, tone-mapped"""
    hc = hm = None
    prev = None
    for c, hdr, alb, nrm, dep in frames:
        if hc is None:
            hc, hm = np.zeros_like(hdr), np.zeros_like(hdr)
        out, hc, hm = capi.debug_filter_temporal(ctx, c, prev[0] if prev else None, hdr, alb, nrm, dep, prev[1] if prev else nrm,
                                                 prev[2] if prev else dep, hc, hm, desc)
        prev = (c, nrm, dep)
    return tonemap(out)


@pytest.mark.parametrize("name", ["cornell_64_b4_s2", "coverage_64_b6_s2"])
def test_moving_camera_quality(ctx, golden_scenes, golden_radiance, name):
    ref, frames, noisy, spatial, denoised = moving_sequence(ctx, golden_scenes[name.split("_")[0]], golden_radiance[name + "/camera"])
    # the frame itself over the same sequence (bit for bit what replay() gives, test_frame_sequence_equals_host_restatement)
    ctx.upload_scene(golden_scenes[name.split("_")[0]])
    fr = capi.Frame(ctx, 128, 128)
    fr.set_max_bounces(4)
    for c, hdr, *_ in frames:
        fr.set_camera(c)
        fr.reset()
        fr.integrate(1)
        assert np.array_equal(bits(fr.radiance()), bits(hdr))
        out = fr.filter_temporal()
    fr.close()
    ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1) & np.isfinite(denoised).all(-1)
    e = {k: tonemapped_mse(v, ref, ok) for k, v in (("noisy", noisy), ("spatial", spatial), ("denoiser", denoised), ("temporal", out))}
    print("%s: tone-mapped MSE against 1024 spp: 1 spp %.3e, rt_frame_filter %.3e, RT_OPT_DENOISER=1 %.3e, temporal %.3e; "
          "temporal / 1 spp %.3f, / spatial %.3f, / denoiser %.3f" % (name, e["noisy"], e["spatial"], e["denoiser"], e["temporal"],
                                                                      e["temporal"] / e["noisy"], e["temporal"] / e["spatial"],
                                                                      e["temporal"] / e["denoiser"]))
    assert e["temporal"] < e["noisy"] and e["temporal"] < e["spatial"] and e["temporal"] < e["denoiser"]
