"""The temporal filter's arithmetic on the host (rt_debug_filter_temporal(NULL, ...)): against an independent numpy restatement of
raytracing_amd/csrc/temporal_filter.h, and the properties a reprojecting, accumulating filter must have.  No GPU needed."""
import numpy as np
import pytest

from raytracing_amd import capi, types as T
from tests.test_spatial_filter import random_inputs

MAX_DIST = np.float32(20000.0)
f32, f64 = np.float32, np.float64
B3 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
G3 = [f32(0.25), f32(0.5), f32(0.25)]


def vec(cam, key):
    return [f32(cam[key][k]) for k in "xyz"]


def make_camera(pos, front, up, fov, aspect):
    cam = np.zeros((), T.camera)
    for key, v in (("position", pos), ("front", front), ("up", up)):
        for k, x in zip("xyz", v):
            cam[key][k] = f32(x)
    cam["fov"], cam["aspect_ratio"] = f32(fov), f32(aspect)
    return cam


def tan_half(cam):
    return f32(np.tan(f64(f32(f32(0.5) * f32(cam["fov"])))))


def guide_dirs(cam, W, H):
    """k_sf_guide_rays' pixel-centre directions, in float32 in the kernel's order"""
    t = tan_half(cam)
    ys, xs = np.mgrid[0:H, 0:W]
    x = (xs.astype(f32) + f32(0.5)) * (f32(1.0) / f32(W))
    y = (ys.astype(f32) + f32(0.5)) * (f32(1.0) / f32(H))
    x = (x * f32(2.0) - f32(1.0)) * t * f32(cam["aspect_ratio"])
    y = (y * f32(2.0) - f32(1.0)) * t
    fr, up = vec(cam, "front"), vec(cam, "up")
    r = [fr[1] * up[2] - fr[2] * up[1], fr[2] * up[0] - fr[0] * up[2], fr[0] * up[1] - fr[1] * up[0]]
    d = [r[c] * x + up[c] * y + fr[c] for c in range(3)]
    ln = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return [dc / ln for dc in d]


def lum(c):
    return f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1] + f32(0.0722) * c[..., 2]


def expw(e):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(-e.astype(f64)).astype(f32)


def shifted(a, dy, dx, fill):
    """a[y + dy, x + dx] where inside, else fill"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[ys, xs] = a[yq, xq]
    return out


def restated(cam, prev_cam, hdr, alb, nrm, dep, pnrm, pdep, hc, hm, desc):
    """temporal_filter.h in numpy, written from its comment: (HDR out, colour history, moments history)"""
    d = capi.temporal_filter_desc(desc)
    H, W = dep.shape
    h, a, n, z = hdr[..., :3], alb[..., :3], nrm[..., :3], dep
    through = ~(z < MAX_DIST) | ~np.isfinite(h).all(-1)
    c = h.copy()
    demod = bool(d.flags & 1)
    with np.errstate(all="ignore"):
        if demod:
            m = (a >= f32(1e-3)) & ~through[..., None]
            c = np.where(m, h / np.where(m, a, f32(1)), h)
            through |= ~np.isfinite(c).all(-1)
    valid = ~through
    l = lum(c)
    # 1. reproject
    hit = np.zeros((H, W), bool)
    lh = np.zeros((H, W), f32)
    ch, mh = c.copy(), np.zeros((H, W, 2), f32)
    if prev_cam is None or prev_cam.tobytes() == cam.tobytes():
        hit = valid & (hm[..., 2] > 0)
        lh = np.where(hit, hm[..., 2], f32(0))
        ch = np.where(hit[..., None], hc[..., :3], c)
        mh = hm[..., :2].copy()
    else:
        dd = guide_dirs(cam, W, H)
        p, pp = vec(cam, "position"), vec(prev_cam, "position")
        X = [p[k] + z * dd[k] for k in range(3)]
        e = [X[k] - pp[k] for k in range(3)]
        dist = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        with np.errstate(all="ignore"):
            u3 = [e[k] / dist for k in range(3)]
            fr, up = vec(prev_cam, "front"), vec(prev_cam, "up")
            den = fr[0] * u3[0] + fr[1] * u3[1] + fr[2] * u3[2]
            ip = [u3[k] / den for k in range(3)]
            r = [fr[1] * up[2] - fr[2] * up[1], fr[2] * up[0] - fr[0] * up[2], fr[0] * up[1] - fr[1] * up[0]]
            t = tan_half(prev_cam)
            u = (r[0] * ip[0] + r[1] * ip[1] + r[2] * ip[2]) / (t * f32(prev_cam["aspect_ratio"]))
            v = (up[0] * ip[0] + up[1] * ip[1] + up[2] * ip[2]) / t
            sx = (u * f32(0.5) + f32(0.5)) * f32(W) - f32(0.5)
            sy = (v * f32(0.5) + f32(0.5)) * f32(H) - f32(0.5)
            ok = valid & (den > 0) & (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
        sx, sy = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        sw = np.zeros((H, W), f32)
        sc, sm = np.zeros((H, W, 3), f32), np.zeros((H, W, 2), f32)
        for tap in range(4):
            qx, qy = x0.astype(int) + (tap & 1), y0.astype(int) + (tap >> 1)
            bw = (fx if tap & 1 else f32(1) - fx) * (fy if tap >> 1 else f32(1) - fy)
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            mq, gq, cq = hm[qyc, qxc], pnrm[qyc, qxc, :3], hc[qyc, qxc, :3]
            with np.errstate(all="ignore"):
                cnt = ok & (bw > 0) & inside & (mq[..., 2] > 0) & (np.abs(pdep[qyc, qxc] - dist) <= f32(0.1) * dist)
                cnt &= (n[..., 0] * gq[..., 0] + n[..., 1] * gq[..., 1] + n[..., 2] * gq[..., 2]) >= f32(0.9)
            first = cnt & ~hit
            ch = np.where(first[..., None], cq, ch)
            mh = np.where(first[..., None], mq[..., :2], mh)
            hit |= cnt
            sw = np.where(cnt, sw + bw, sw)
            sc = np.where(cnt[..., None], sc + bw[..., None] * (cq - ch), sc)
            sm = np.where(cnt[..., None], sm + bw[..., None] * (mq[..., :2] - mh), sm)
            lh = np.where(cnt, np.maximum(lh, mq[..., 2]), lh)
        with np.errstate(all="ignore"):
            ch = np.where(hit[..., None], ch + sc / sw[..., None], ch)
            mh = np.where(hit[..., None], mh + sm / sw[..., None], mh)
    # 2. accumulate
    length = np.where(hit, np.minimum(lh + f32(1), f32(1024)), f32(1))
    inv = f32(1) / length
    al, am = np.maximum(f32(d.alpha_color), inv), np.maximum(f32(d.alpha_moments), inv)
    with np.errstate(all="ignore"):
        acc = np.where((hit & (al != 1))[..., None], ch + al[..., None] * (c - ch), c)
        m1 = np.where(hit & (am != 1), mh[..., 0] + am * (l - mh[..., 0]), l)
        m2 = np.where(hit & (am != 1), mh[..., 1] + am * (l * l - mh[..., 1]), l * l)
    own = ~hit | (al == 1)
    acc = np.where(valid[..., None], acc, f32(0))
    mom = np.stack([m1, m2, length, np.zeros_like(m1)], -1)
    mom[~valid] = 0
    inv_n, inv_z = f32(1) / f32(d.sigma_normal), f32(1) / f32(d.sigma_depth)

    def taps(radius, step, fn):
        for k in range(-radius, radius + 1):
            for j in range(-radius, radius + 1):
                ok = shifted(valid, step * k, step * j, False)
                fn(j, k, ok, lambda a, fill=0: shifted(a, step * k, step * j, fill))

    def normal_depth_term(j, k, step, q):
        with np.errstate(all="ignore"):
            e = (f32(1) - (n[..., 0] * q(n)[..., 0] + n[..., 1] * q(n)[..., 1] + n[..., 2] * q(n)[..., 2])) * inv_n
            if j or k:
                e = e + np.abs(z - q(z, 1)) * inv_z / (z * f32(step * max(abs(j), abs(k))))
        return e

    col, var = acc.copy(), np.zeros((H, W), f32)
    if d.iterations:
        # 3. variance
        s = [np.zeros((H, W), f32) for _ in range(3)]

        def vt(j, k, ok, q):
            w = np.where(ok, expw(normal_depth_term(j, k, 1, q)), f32(0))
            s[0][...] = s[0] + w
            s[1][...] = s[1] + w * (q(mom[..., 0]) - mom[..., 0])
            s[2][...] = s[2] + w * (q(mom[..., 1]) - mom[..., 1])
        taps(3, 1, vt)
        with np.errstate(all="ignore"):
            sp = (mom[..., 2] < 4) & (s[0] > 0)
            v1 = np.where(sp, mom[..., 0] + s[1] / s[0], mom[..., 0])
            v2 = np.where(sp, mom[..., 1] + s[2] / s[0], mom[..., 1])
        var = np.where(valid, np.maximum(v2 - v1 * v1, f32(0)), f32(0))
    hist = None
    for i in range(d.iterations):
        step = 1 << i
        gs, gw = np.zeros((H, W), f32), np.zeros((H, W), f32)
        for k in (-1, 0, 1):
            for j in (-1, 0, 1):
                ok = shifted(valid, k, j, False)
                gw = np.where(ok, gw + G3[j + 1] * G3[k + 1], gw)
                gs = np.where(ok, gs + G3[j + 1] * G3[k + 1] * shifted(var, k, j, 0), gs)
        with np.errstate(all="ignore"):
            den = f32(d.sigma_luminance) * np.sqrt(gs / gw) + f32(1e-4)
        lp = lum(col)
        acc_ = [np.zeros((H, W), f32) for _ in range(5)]

        def pt(j, k, ok, q):
            with np.errstate(all="ignore"):
                e = np.abs(lp - lum(q(col))) / den + normal_depth_term(j, k, step, q)
                w = np.where(ok, (B3[j + 2] * B3[k + 2]) * expw(e), f32(0))
            acc_[0][...] = acc_[0] + w
            for ch_ in range(3):
                acc_[1 + ch_][...] = acc_[1 + ch_] + w * (q(col[..., ch_]) - col[..., ch_])
            acc_[4][...] = acc_[4] + (w * w) * q(var)
        taps(2, step, pt)
        with np.errstate(all="ignore"):
            upd = valid & (acc_[0] > 0)
            col = np.where(upd[..., None], col + np.stack(acc_[1:4], -1) / acc_[0][..., None], col)
            var = np.where(upd, acc_[4] / (acc_[0] * acc_[0]), var)
        if i == 0:
            hist = col.copy()
    if hist is None:
        hist = acc.copy()
    hist = np.where(valid[..., None], hist, f32(0))
    # 5. finish
    with np.errstate(all="ignore"):
        out = np.where(demod & (a >= f32(1e-3)), col * a, col)
    pas = ~valid | ~np.isfinite(out).all(-1) | ~np.isfinite(col).all(-1) | ((d.iterations == 0) & own)
    out = np.where(pas[..., None], h, out)
    hist4 = np.concatenate([hist, np.zeros((H, W, 1), f32)], -1)
    return out, hist4, mom


def random_history(rng, H, W, max_len=8):
    hc = np.zeros((H, W, 4), f32)
    hc[..., :3] = rng.exponential(0.5, (H, W, 3))
    lum_ = rng.exponential(0.5, (H, W)).astype(f32)
    hm = np.zeros((H, W, 4), f32)
    hm[..., 0] = lum_
    hm[..., 1] = lum_ * lum_ * f32(1.5)
    hm[..., 2] = rng.integers(0, max_len, (H, W))
    return hc, hm


def random_cameras(rng, W, H):
    pos = rng.normal(size=3) * 0.1
    front = np.array([0.0, 0.0, -1.0]) + rng.normal(size=3) * 0.05
    front /= np.linalg.norm(front)
    up = np.cross(np.cross(front, [0, 1, 0]), front)
    up /= -np.linalg.norm(up) if up[1] < 0 else np.linalg.norm(up)
    cam = make_camera(pos, front, up, 1.0, W / H)
    move = rng.normal(size=3) * 0.01
    prev = make_camera(pos - move, front, up, 1.0, W / H)
    return cam, prev


def host(cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm, desc):
    return capi.debug_filter_temporal(None, cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm, desc)


def random_case(rng, H, W):
    hdr, alb, nrm, dep = random_inputs(rng, H, W)
    _, _, pnrm, pdep = random_inputs(rng, H, W)
    agree = rng.random((H, W)) < 0.6                                  # most previous guides agree with this call's
    pnrm[agree] = nrm[agree]
    keep = rng.random((H, W)) < 0.7
    pdep[keep] = dep[keep]
    hc, hm = random_history(rng, H, W)
    cam, prev = random_cameras(rng, W, H)
    return cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (16, 16), (23, 41)])
@pytest.mark.parametrize("demod", [0, 1])
def test_host_filter_matches_numpy_restatement(shape, demod):
    rng = np.random.default_rng(shape[0] * 31 + shape[1] + demod)
    args = random_case(rng, *shape)
    for it in (0, 1, 3):
        for standing in (False, True):
            a = list(args)
            if standing:
                a[1] = None
            desc = dict(iterations=it, flags=demod, alpha_color=float(rng.uniform(0.05, 0.5)), alpha_moments=float(rng.uniform(0.05, 0.5)),
                        sigma_luminance=float(rng.uniform(0.5, 8.0)), sigma_normal=float(rng.uniform(0.05, 1.0)),
                        sigma_depth=float(rng.uniform(0.05, 1.0)))
            got = host(*a, desc)
            want = restated(*a, desc)
            assert np.array_equal(got[2], want[2]), (it, standing)               # moments and lengths: no exponential involved
            np.testing.assert_allclose(got[0][..., :3], want[0], rtol=1e-5, atol=1e-6, err_msg=str((it, standing)))
            np.testing.assert_allclose(got[1], want[1], rtol=1e-5, atol=1e-6, err_msg=str((it, standing)))
            assert (got[0][..., 3] == 1).all()
            if shape == (23, 41) and not standing:
                L = got[2][..., 2]
                assert (L == 1).sum() > 20 and (L > 1).sum() > 200 and (L == 0).sum() > 20     # misses, hits and pass-through pixels


def plane_case(W=24, H=16, D=3.0, shift_px=1.0, fov=1.0):
    """a camera looking straight down at the plane z = 0 from height D, and the previous camera shift_px pixel widths to its -x"""
    cam = make_camera((0.0, 0.0, D), (0, 0, -1), (0, 1, 0), fov, W / H)
    px = f64(2.0) * D * f64(tan_half(cam)) * f64(f32(W / H)) / W
    prev = make_camera((-shift_px * px, 0.0, D), (0, 0, -1), (0, 1, 0), fov, W / H)

    def depth(c):
        d = guide_dirs(c, W, H)
        return (f32(D) / -d[2]).astype(f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    return cam, prev, depth(cam), depth(prev), nrm


def test_a_flat_field_stays_exactly_flat():
    rng = np.random.default_rng(5)
    H, W = 16, 24
    cam, prev, dep, pdep, nrm = plane_case(W, H, shift_px=0.37)
    hdr = np.full((H, W, 4), 0.3, f32)
    alb = np.full((H, W, 4), 0.7, f32)
    hc, hm = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    cams = [prev, cam]
    for call in range(5):
        c, p = cams[call % 2], cams[(call + 1) % 2]
        desc = dict(iterations=int(rng.integers(0, 6)), flags=1)
        out, hc, hm = host(c, p if call else None, hdr, alb, nrm, dep if c is cam else pdep, nrm, pdep if c is cam else dep, hc, hm, desc)
        assert len(np.unique(out[..., :3].reshape(-1, 3), axis=0)) == 1, call
        assert len(np.unique(hc[..., :3].reshape(-1, 3), axis=0)) == 1, call
        assert (hm[..., 2] >= 1).all() and (hm[..., 0] == hm[0, 0, 0]).all()


def test_nan_pixel_stays_one_pixel_and_invalid_pixels_pass_through():
    rng = np.random.default_rng(9)
    H, W = 20, 20
    cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm = random_case(rng, H, W)
    dep[10, 10] = 2.0
    hdr[10, 10, 1] = np.nan
    invalid = dep >= MAX_DIST
    for it in (0, 2, 5):
        for demod in (0, 1):
            out, hc2, hm2 = host(cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm, dict(iterations=it, flags=demod))
            bad = ~np.isfinite(out[..., :3]).all(-1)
            assert bad.sum() == 1 and bad[10, 10]
            assert np.array_equal(out[invalid][:, :3].view(np.uint32), hdr[invalid][:, :3].view(np.uint32))
            assert (hm2[invalid] == 0).all() and hm2[10, 10, 2] == 0 and (hc2[invalid] == 0).all()


def test_standing_camera_alpha_0_is_the_running_mean():
    rng = np.random.default_rng(11)
    H, W = 12, 17
    _, alb, nrm, dep = random_inputs(rng, H, W, invalid=0.0)
    cam, _ = random_cameras(rng, W, H)
    hc, hm = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    inputs = []
    for k in range(7):
        hdr = np.zeros((H, W, 4), f32)
        hdr[..., :3] = rng.exponential(0.5, (H, W, 3))
        inputs.append(hdr[..., :3].astype(f64))
        out, hc, hm = host(cam, None, hdr, alb, nrm, dep, nrm, dep, hc, hm, dict(iterations=0, flags=0, alpha_color=0.0, alpha_moments=0.0))
        np.testing.assert_allclose(hc[..., :3], np.mean(inputs, 0), rtol=1e-6)
        assert (hm[..., 2] == k + 1).all()
        l = [lum(x.astype(f32)).astype(f64) for x in inputs]
        np.testing.assert_allclose(hm[..., 0], np.mean(l, 0), rtol=1e-5)
        np.testing.assert_allclose(hm[..., 1], np.mean([v * v for v in l], 0), rtol=1e-5)
        if k:
            np.testing.assert_allclose(out[..., :3], hc[..., :3], rtol=1e-6)   # no demodulation, no pass: the output is the history


def test_one_pixel_pan_takes_history_from_the_neighbour():
    H, W = 16, 24
    cam, prev, dep, pdep, nrm = plane_case(W, H, shift_px=1.0)
    hdr = np.zeros((H, W, 4), f32)
    hdr[..., :3] = 0.5
    alb = np.ones((H, W, 4), f32)
    hc = np.zeros((H, W, 4), f32)
    hc[..., 0] = np.arange(W, dtype=f32)[None, :]
    hc[..., 1] = np.arange(H, dtype=f32)[:, None]
    hm = np.zeros((H, W, 4), f32)
    hm[..., 2] = 5
    out, hc2, hm2 = host(cam, prev, hdr, alb, nrm, dep, nrm, pdep, hc, hm, dict(iterations=0, flags=0, alpha_color=0.25, alpha_moments=0.25))
    inner = (slice(None), slice(0, W - 1))
    want = np.zeros((H, W, 3))
    want[..., 0] = np.arange(W)[None, :] + 1.0                # pixel x sees what pixel x + 1 saw
    want[..., 1] = np.arange(H)[:, None]
    want = want + 0.25 * (0.5 - want)
    np.testing.assert_allclose(hc2[inner][..., :3], want[inner], atol=1e-3)
    assert (hm2[inner][..., 2] == 6).all()
    assert (hm2[:, W - 1, 2] <= 6).all()


def test_pixels_entering_at_the_edge_miss():
    H, W = 16, 24
    cam, prev, dep, pdep, nrm = plane_case(W, H, shift_px=2.5)
    hdr = np.full((H, W, 4), 0.5, f32)
    hm = np.zeros((H, W, 4), f32)
    hm[..., 2] = 5
    _, _, hm2 = host(cam, prev, hdr, np.ones_like(hdr), nrm, dep, nrm, pdep, np.zeros_like(hdr), hm, dict(iterations=2, flags=0))
    assert (hm2[:, W - 2:, 2] == 1).all()                     # they were outside the previous image
    assert (hm2[:, :W - 4, 2] == 6).all()
    # and the other way round: the camera moving to -x brings pixels in at the left edge
    _, _, hm3 = host(prev, cam, hdr, np.ones_like(hdr), nrm, pdep, nrm, dep, np.zeros_like(hdr), hm, dict(iterations=2, flags=0))
    assert (hm3[:, :2, 2] == 1).all() and (hm3[:, 4:, 2] == 6).all()


@pytest.mark.parametrize("what", ["depth", "normal"])
def test_disagreeing_depth_or_normal_misses(what):
    H, W = 16, 24
    cam, prev, dep, pdep, nrm = plane_case(W, H, shift_px=1.0)
    hdr = np.full((H, W, 4), 0.5, f32)
    hm = np.zeros((H, W, 4), f32)
    hm[..., 2] = 5
    # (a far tap of a 2 x 2 footprint may carry a bilinear weight of ~1e-7 and still counts: the step must clear the depth gradient across it)
    for factor, cosine, hits in ((1.3, 0.85, False), (1.05, 0.95, True)):
        pnrm, pd = nrm.copy(), pdep.copy()
        if what == "depth":
            pd[:H // 2] *= f32(factor)
        else:
            pnrm[:H // 2, :, 0] = np.sqrt(1 - cosine ** 2)
            pnrm[:H // 2, :, 2] = cosine
        _, _, hm2 = host(cam, prev, hdr, np.ones_like(hdr), nrm, dep, pnrm, pd, np.zeros_like(hdr), hm, dict(iterations=1, flags=0))
        L = hm2[1:H // 2 - 1, :W - 1, 2]
        assert (L == (6 if hits else 1)).all(), (factor, cosine)
        assert (hm2[H // 2 + 1:, :W - 1, 2] == 6).all()


def test_an_empty_history_misses_everywhere_and_alpha_1_is_the_input():
    rng = np.random.default_rng(2)
    cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm = random_case(rng, 14, 19)
    out, hc2, hm2 = host(cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, np.zeros_like(hm), dict(iterations=3, flags=1))
    valid = dep < MAX_DIST
    assert (hm2[valid, 2] == 1).all() and (hm2[~valid, 2] == 0).all()
    out, _, _ = host(cam, prev, hdr, alb, nrm, dep, pnrm, pdep, hc, hm, dict(iterations=0, flags=1, alpha_color=1.0))
    assert np.array_equal(out[..., :3].view(np.uint32), hdr[..., :3].view(np.uint32))


@pytest.mark.parametrize("bad", [dict(iterations=9), dict(flags=2), dict(alpha_color=-0.1), dict(alpha_color=1.5), dict(alpha_moments=float("nan")),
                                 dict(sigma_luminance=0.0), dict(sigma_normal=float("inf")), dict(sigma_depth=-1.0)])
def test_desc_out_of_range_is_refused(bad):
    rng = np.random.default_rng(4)
    args = random_case(rng, 4, 5)
    with pytest.raises(capi.RtError, match="rt_debug_filter_temporal"):
        host(*args, bad)


def test_header_defaults_match_python():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rt_hip.h")).read()
    m = re.search(r"#define RT_TEMPORAL_FILTER_DESC_DEFAULT \{ (\d+)u, RT_FILTER_DEMODULATE, ([\d.]+)f, ([\d.]+)f, ([\d.]+)f, ([\d.]+)f, ([\d.]+)f \}", text)
    assert m
    d = capi.TEMPORAL_FILTER_DEFAULT
    assert int(m.group(1)) == d["iterations"] and d["flags"] == capi.FILTER_DEMODULATE
    assert [float(m.group(i)) for i in range(2, 7)] == [d[k] for k in ("alpha_color", "alpha_moments", "sigma_luminance", "sigma_normal", "sigma_depth")]
