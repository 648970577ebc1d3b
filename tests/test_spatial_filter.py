"""The spatial filter's arithmetic on the host (rt_debug_filter(NULL, ...)): against an independent float64 numpy restatement of
raytracing_amd/csrc/spatial_filter.h, and the properties an edge-avoiding filter must have.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from raytracing_amd import capi

MAX_DIST = 20000.0
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def restated(hdr, alb, nrm, dep, iterations, demod, sc, sn, sz):
    """spatial_filter.h in float64 numpy, written from its comment, not from its code"""
    h = hdr[..., :3].astype(np.float64)
    a = alb[..., :3].astype(np.float64)
    n = nrm[..., :3].astype(np.float64)
    z = dep.astype(np.float64)
    H, W = z.shape
    through = ~(z < MAX_DIST) | ~np.isfinite(h).all(-1)
    c = h.copy()
    if demod:
        m = (a >= np.float32(1e-3)) & ~through[..., None]
        c = np.where(m, h / np.where(m, a, 1.0), h)
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(iterations):
        s = 1 << i
        inv_c = float(np.float32(1.0) / np.float32(np.float32(sc) * np.float32(sc))) * 4.0 ** i
        inv_n, inv_z = float(np.float32(1.0) / np.float32(sn)), float(np.float32(1.0) / np.float32(sz))
        sw = np.zeros((H, W))
        acc = np.zeros((H, W, 3))
        for k in range(-2, 3):
            for j in range(-2, 3):
                qy, qx = ys + s * k, xs + s * j
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                ok = inside & ~through[qyc, qxc]
                cq = c[qyc, qxc]
                e = ((c - cq) ** 2).sum(-1) * inv_c + (1.0 - (n * n[qyc, qxc]).sum(-1)) * inv_n
                if j or k:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        e = e + np.abs(z - z[qyc, qxc]) * inv_z / (z * s * max(abs(j), abs(k)))
                with np.errstate(invalid="ignore", over="ignore"):
                    w = np.where(ok, B3[j + 2] * B3[k + 2] * np.exp(-np.where(ok, e, 0.0)), 0.0)
                sw += w
                acc += w[..., None] * np.where(ok[..., None], cq, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(through[..., None], c, acc / sw[..., None])
    if demod:
        m = (a >= np.float32(1e-3)) & ~through[..., None]
        c = np.where(m, c * a, c)
    return c


def random_inputs(rng, H, W, invalid=0.1):
    hdr = np.zeros((H, W, 4), np.float32)
    hdr[..., :3] = rng.exponential(0.5, (H, W, 3))
    hdr[..., 3] = rng.random((H, W))
    alb = np.zeros((H, W, 4), np.float32)
    alb[..., :3] = rng.random((H, W, 3))
    alb[..., :3][rng.random((H, W, 3)) < 0.1] = 0.0005           # below the demodulation threshold
    v = rng.normal(size=(H, W, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    flat = rng.random((H, W)) < 0.5                                 # half the normals agree: weights span the whole range
    v[flat] = (0.0, 0.0, 1.0)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., :3] = v
    dep = rng.uniform(1.0, 3.0, (H, W)).astype(np.float32)
    dep[rng.random((H, W)) < invalid] = MAX_DIST
    return hdr, alb, nrm, dep


def host_filter(hdr, alb, nrm, dep, **desc):
    return capi.debug_filter(None, hdr, alb, nrm, dep, desc)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (16, 16), (23, 41)])
@pytest.mark.parametrize("demod", [0, 1])
def test_host_filter_matches_numpy_restatement(shape, demod):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + demod)
    hdr, alb, nrm, dep = random_inputs(rng, *shape)
    for it in range(0, 9):
        sig = dict(sigma_color=float(rng.uniform(0.2, 2.0)), sigma_normal=float(rng.uniform(0.05, 1.0)), sigma_depth=float(rng.uniform(0.05, 1.0)))
        got = host_filter(hdr, alb, nrm, dep, iterations=it, flags=demod, **sig)
        if it == 0:
            assert np.array_equal(got.view(np.uint32), hdr.view(np.uint32))
            continue
        want = restated(hdr, alb, nrm, dep, it, demod, sig["sigma_color"], sig["sigma_normal"], sig["sigma_depth"])
        np.testing.assert_allclose(got[..., :3], want, rtol=1e-5, atol=1e-30, err_msg="iterations %d" % it)
        assert np.array_equal(got[..., 3], hdr[..., 3])               # alpha is carried, not filtered


def test_constant_image_is_unchanged():
    H, W = 40, 50
    for value, albedo in ((0.37, 0.61), (2.5, 0.2), (0.125, 1.0)):
        hdr = np.zeros((H, W, 4), np.float32)
        hdr[..., :3] = value
        alb = np.zeros_like(hdr)
        alb[..., :3] = albedo
        nrm = np.zeros_like(hdr)
        nrm[..., 1] = 1.0
        dep = np.full((H, W), 4.0, np.float32)
        for demod in (0, 1):
            out = host_filter(hdr, alb, nrm, dep, iterations=8, flags=demod, sigma_color=0.5, sigma_normal=0.1, sigma_depth=0.1)
            ulp = np.abs(out[..., :3].view(np.int32).astype(np.int64) - hdr[..., :3].view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (value, albedo, demod, ulp.max())


@pytest.mark.parametrize("edge", ["normal", "depth"])
def test_two_flat_regions_stay_two_flat_regions(edge):
    H, W = 32, 32
    hdr = np.zeros((H, W, 4), np.float32)
    alb = np.full((H, W, 4), 0.5, np.float32)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = 1.0
    dep = np.full((H, W), 2.0, np.float32)
    left = np.zeros((H, W), bool)
    left[:, :W // 2] = True
    hdr[left, :3], hdr[~left, :3] = (0.2, 0.3, 0.4), (0.21, 0.31, 0.39)    # the colours alone do not tell the regions apart
    if edge == "normal":
        nrm[~left] = (1.0, 0.0, 0.0, 0.0)
        desc = dict(iterations=5, flags=1, sigma_color=10.0, sigma_normal=0.1, sigma_depth=0.1)
    else:
        # the depth term is a relative depth step PER PIXEL of tap distance (spatial_filter.h): a depth edge holds while the jump
        # is large against sigma_depth x the tap spacing -- here up to 4 pixels (3 passes)
        dep[~left] = 20.0
        desc = dict(iterations=3, flags=1, sigma_color=10.0, sigma_normal=0.1, sigma_depth=0.01)
    out = host_filter(hdr, alb, nrm, dep, **desc)
    for region in (left, ~left):
        np.testing.assert_allclose(out[region, :3], hdr[region, :3], rtol=1e-3)
    # without the edge the same filter blends them
    flat = host_filter(hdr, alb, np.broadcast_to(nrm[:, :1], nrm.shape), np.full((H, W), 2.0, np.float32), **desc)
    assert np.abs(flat[:, W // 2 - 1, 0] - flat[:, W // 2, 0]).max() < 0.005


def test_nan_and_inf_pixels_stay_and_do_not_spread():
    rng = np.random.default_rng(7)
    hdr, alb, nrm, dep = random_inputs(rng, 24, 24, invalid=0.0)
    hdr[5, 5, :3] = np.nan
    hdr[12, 7, 1] = np.nan
    hdr[18, 18, :3] = np.inf
    hdr[3, 20, 2] = -np.inf
    bad = np.zeros((24, 24), bool)
    bad[5, 5] = bad[12, 7] = bad[18, 18] = bad[3, 20] = True
    for demod in (0, 1):
        out = host_filter(hdr, alb, nrm, dep, iterations=5, flags=demod, sigma_color=1.0, sigma_normal=0.2, sigma_depth=0.2)
        assert np.array_equal(out[bad].view(np.uint32), hdr[bad].view(np.uint32))
        assert np.isfinite(out[~bad]).all()


def test_invalid_pixels_are_copied_unchanged():
    rng = np.random.default_rng(11)
    hdr, alb, nrm, dep = random_inputs(rng, 30, 20, invalid=0.3)
    inv = dep >= MAX_DIST
    for demod in (0, 1):
        out = host_filter(hdr, alb, nrm, dep, iterations=6, flags=demod, sigma_color=1.0, sigma_normal=0.2, sigma_depth=0.2)
        assert np.array_equal(out[inv].view(np.uint32), hdr[inv].view(np.uint32))
        assert not np.array_equal(out[~inv], hdr[~inv])


def _raw(desc, hdr=True, alb=True, nrm=True, dep=True, out=True, w=4, h=4):
    lib = capi.load()
    a = np.ones((h, w, 4), np.float32)
    d = np.ones((h, w), np.float32)
    o = np.zeros_like(a)
    rc = lib.rt_debug_filter(None, w, h, a.ctypes.data if hdr else None, a.ctypes.data if alb else None, a.ctypes.data if nrm else None,
                             d.ctypes.data if dep else None, C.byref(desc) if desc is not None else None, o.ctypes.data if out else None)
    return rc, (lib.rt_last_error(None) or b"").decode()


@pytest.mark.parametrize("bad", [dict(iterations=9), dict(iterations=100), dict(flags=2), dict(sigma_color=0.0), dict(sigma_normal=-1.0),
                                 dict(sigma_depth=float("nan")), dict(sigma_color=float("inf"))])
def test_out_of_range_desc_fails_with_a_message(bad):
    rc, msg = _raw(capi.filter_desc(None, **bad))
    assert rc != 0 and "rt_debug_filter" in msg
    with pytest.raises(capi.RtError):
        host_filter(*random_inputs(np.random.default_rng(0), 4, 4), **bad)


@pytest.mark.parametrize("missing", ["desc", "hdr", "alb", "nrm", "dep", "out"])
def test_null_arguments_fail_with_a_message(missing):
    kw = dict(hdr=True, alb=True, nrm=True, dep=True, out=True)
    desc = capi.filter_desc()
    if missing == "desc":
        desc = None
    else:
        kw[missing] = False
    rc, msg = _raw(desc, **kw)
    assert rc != 0 and "NULL" in msg


def test_frame_entry_points_refuse_null_arguments():
    lib = capi.load()
    d = capi.filter_desc()
    out = np.zeros(4, np.float32)
    assert lib.rt_frame_filter(None, C.byref(d), out.ctypes.data) != 0 and b"NULL" in lib.rt_last_error(None)
    assert lib.rt_frame_read_guides(None, None, None, None, None) != 0 and b"NULL" in lib.rt_last_error(None)


def test_defaults_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "rt_hip.h")).read()
    m = re.search(r"#define RT_FILTER_DESC_DEFAULT \{ (\d+)u, RT_FILTER_DEMODULATE, ([\d.]+)f, ([\d.]+)f, ([\d.]+)f \}", hdr)
    assert m, "RT_FILTER_DESC_DEFAULT not found"
    d = capi.FILTER_DEFAULT
    assert (d["iterations"], d["flags"], d["sigma_color"], d["sigma_normal"], d["sigma_depth"]) == \
        (int(m.group(1)), capi.FILTER_DEMODULATE, float(m.group(2)), float(m.group(3)), float(m.group(4)))
