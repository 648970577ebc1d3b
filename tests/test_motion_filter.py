"""The temporal filter's history across a refit of moving geometry (RT_CTX_OPT_REFIT_MOTION) on the host: the motion images'
arithmetic (rt_debug_guide_motion(NULL, ...)) against numpy, rt_debug_filter_temporal_motion(NULL, ...) without motion images against the entry it
extends, and a synthetic moved patch whose history must follow it.  Also the bookkeeping the GPU tests of tests/test_gpu_motion_filter.py share: the
Cornell sequence (which triangles move, by how much) and the pixels whose history must survive it, checked here with first hits traced in numpy.
No GPU needed."""
import numpy as np
import pytest

from raytracing_amd import capi, types as T
from tests.test_refit import positions, moved
from tests.test_temporal_filter import random_case, make_camera, guide_dirs, tan_half, vec

f32, f64 = np.float32, np.float64
INVALID = 0xFFFFFFFF


def normals(tris):
    """float32[nt, 3 vertices, 3]"""
    return np.stack([np.stack([tris[v]["normal"][c] for c in "xyz"], -1) for v in ("v1", "v2", "v3")], 1)


def random_triangles(rng, n, extent=10.0):
    tris = np.zeros(n, T.triangle)
    P = rng.uniform(-extent, extent, (n, 3, 3)).astype(f32)
    N = rng.normal(size=(n, 3, 3))
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    tris = moved(tris, P)
    for k, v in enumerate(("v1", "v2", "v3")):
        for a, c in enumerate("xyz"):
            tris[v]["normal"][c] = N[:, k, a].astype(f32)
    return tris


def hits_of(u, v, prim):
    h = np.zeros(u.shape + (4,), f32)
    h[..., 0], h[..., 1] = u, v
    h[..., 2] = np.asarray(prim, np.uint32).view(f32)
    return h


def test_host_restatement_against_numpy():
    rng = np.random.default_rng(1)
    nt, n = 300, 5000
    extent = 10.0
    prev = random_triangles(rng, nt, extent)
    # the pose now: every triangle displaced by at least 1 % of the extent, so that the wrong pose (or a wrong vertex) is off by far more than the bound
    shift = rng.normal(size=(nt, 1, 3))
    shift *= rng.uniform(0.01 * 2 * extent, 0.1 * 2 * extent, (nt, 1, 1)) / np.linalg.norm(shift, axis=-1, keepdims=True)
    now = moved(prev, (positions(prev) + shift).astype(f32))
    assert np.linalg.norm(positions(now).astype(f64) - positions(prev), axis=-1).min() >= 0.01 * 2 * extent * 0.999
    u = rng.uniform(0, 1, n)
    v = rng.uniform(0, 1, n) * (1 - u)
    prim = rng.integers(0, nt, n).astype(np.uint32)
    prim[::97] = INVALID
    prim[5::211] = nt                                        # one past the end: no hit either
    hits = hits_of(u.astype(f32), v.astype(f32), prim)
    pos, nrm = capi.debug_guide_motion(None, hits, prev)
    ok = prim < nt
    assert (pos[~ok] == 0).all() and (nrm[~ok] == 0).all() and (~ok).sum() > 20
    uu, vv = hits[ok, 0].astype(f64), hits[ok, 1].astype(f64)
    w0 = 1.0 - uu - vv
    P, N = positions(prev).astype(f64)[prim[ok]], normals(prev).astype(f64)[prim[ok]]
    want = P[:, 0] * w0[:, None] + P[:, 1] * uu[:, None] + P[:, 2] * vv[:, None]
    bound = 8 * 2.0 ** -23 * np.abs(positions(prev)).max()
    assert np.abs(pos[ok, :3] - want).max() <= bound
    assert (pos[ok, 3] == 1).all() and (nrm[ok, 3] == 0).all()
    # ... and it is the PREVIOUS pose: the pose now is at least 1 % of the extent away
    now_at = positions(now).astype(f64)[prim[ok]]
    now_at = now_at[:, 0] * w0[:, None] + now_at[:, 1] * uu[:, None] + now_at[:, 2] * vv[:, None]
    assert np.linalg.norm(pos[ok, :3] - now_at, axis=-1).min() > 0.009 * 2 * extent
    wn = N[:, 0] * w0[:, None] + N[:, 1] * uu[:, None] + N[:, 2] * vv[:, None]
    wn /= np.linalg.norm(wn, axis=-1, keepdims=True)
    assert np.abs(np.linalg.norm(nrm[ok, :3].astype(f64), axis=-1) - 1).max() <= 1e-6
    assert np.abs(nrm[ok, :3] - wn).max() <= 1e-5           # the direction too (the interpolated normals here are no shorter than ~0.1)
    # shapes travel: an image of hits gives images
    pos2, nrm2 = capi.debug_guide_motion(None, hits[:4998].reshape(42, 119, 4), prev)
    assert pos2.shape == (42, 119, 4) and np.array_equal(pos2.reshape(-1, 4).view(np.uint32), pos[:4998].view(np.uint32))
    assert np.array_equal(nrm2.reshape(-1, 4).view(np.uint32), nrm[:4998].view(np.uint32))


DESCS = [dict(iterations=it, flags=demod, alpha_color=0.2, alpha_moments=0.3, sigma_luminance=4.0, sigma_normal=0.1, sigma_depth=0.2)
         for it in (0, 2) for demod in (0, 1)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (23, 41)])
def test_null_motion_is_the_old_filter(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    args = list(random_case(rng, *shape))
    some = np.zeros(shape + (4,), f32)
    for desc in DESCS:
        for standing in (False, True):
            a = list(args)
            if standing:
                a[1] = None
            want = capi.debug_filter_temporal(None, *a, desc)
            for pp, pn in ((None, None), (some, None), (None, some)):
                got = capi.debug_filter_temporal_motion(None, *a, pp, pn, desc)
                for g, w in zip(got, want):
                    assert g.tobytes() == w.tobytes()


def test_motion_images_without_motion_are_the_camera_rule():
    """w = 0 everywhere (no motion known) under a moving camera: TF_REPROJECT by the camera alone"""
    rng = np.random.default_rng(3)
    args = list(random_case(rng, 23, 41))
    zero = np.zeros((23, 41, 4), f32)
    for desc in DESCS:
        want = capi.debug_filter_temporal(None, *args, desc)
        got = capi.debug_filter_temporal_motion(None, *args, zero, zero, desc)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()


def test_a_moved_patch_keeps_its_history():
    """A camera looking straight down from height D at the plane z = 0 and at a patch floating at z = 1, which moved K whole pixels to +x between the
    calls.  The history: length 5 where the patch WAS, 2 elsewhere; the colour a ramp in x and y."""
    W, H, D, K = 48, 32, 3.0, 3
    cam = make_camera((0.0, 0.0, D), (0, 0, -1), (0, 1, 0), 1.0, W / H)
    d = guide_dirs(cam, W, H)
    px_patch = f64(2.0) * (D - 1.0) * f64(tan_half(cam)) * f64(f32(W / H)) / W          # one pixel's width on the patch's plane
    ys, xs = np.mgrid[0:H, 0:W]
    patch_now = (xs >= 20) & (xs < 36) & (ys >= 8) & (ys < 24)
    patch_prev = (xs >= 20 - K) & (xs < 36 - K) & (ys >= 8) & (ys < 24)
    inner = (xs >= 22) & (xs < 34) & (ys >= 10) & (ys < 22)                            # >= 2 pixels from the patch's border

    def depth(patch):
        return np.where(patch, f32(D - 1.0), f32(D)) / -d[2]
    dep, pdep = depth(patch_now).astype(f32), depth(patch_prev).astype(f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    X = np.stack([f32(cam["position"][k]) + dep * d[i] for i, k in enumerate("xyz")], -1).astype(f64)
    prev_pos = np.ones((H, W, 4), f32)
    prev_pos[..., :3] = X
    prev_pos[patch_now, 0] = (X[patch_now, 0] - K * px_patch)                            # the patch came from K pixels to the left
    prev_n = nrm.copy()
    hdr = np.zeros((H, W, 4), f32)
    hdr[..., :3] = 0.5
    alb = np.ones((H, W, 4), f32)
    hc = np.zeros((H, W, 4), f32)
    hc[..., 0], hc[..., 1] = xs, ys
    hm = np.zeros((H, W, 4), f32)
    hm[..., 2] = np.where(patch_prev, 5, 2)
    desc = dict(iterations=0, flags=0, alpha_color=0.25, alpha_moments=0.25)
    base = (cam, None, hdr, alb, nrm, dep, nrm, pdep, hc, hm)
    out, hc2, hm2 = capi.debug_filter_temporal_motion(None, *base, prev_pos, prev_n, desc)
    # with motion: inside the patch the history is the patch's own, L_h + 1 = 6, and its colour is what the pixel K to the left held
    assert (hm2[inner][:, 2] == 6).all()
    want = np.stack([xs - K, ys], -1).astype(f64)
    want = want + 0.25 * (0.5 - want)
    np.testing.assert_allclose(hc2[inner][:, :2], want[inner], atol=1e-3)
    # ... the static plane away from both patch positions keeps its own
    far = (xs < 15) | (xs >= 38)
    assert (hm2[far][:, 2] == 3).all()
    # ... and what the patch uncovered has nothing to take: the depth disagrees
    uncovered = patch_prev & ~patch_now
    assert (hm2[uncovered][:, 2] == 1).all()
    # without the motion images: the old TF_IDENTITY result, every pixel its own history whatever lies there
    out0, hc0, hm0 = capi.debug_filter_temporal_motion(None, *base, None, None, desc)
    old = capi.debug_filter_temporal(None, *base, desc)
    for g, w in zip((out0, hc0, hm0), old):
        assert g.tobytes() == w.tobytes()
    assert np.array_equal(hm0[..., 2], np.where(patch_prev, 6, 3))
    assert (hm0[inner & ~patch_prev][:, 2] == 3).all() and (inner & ~patch_prev).sum() > 0
    # a normal that turned with the object: tested where it WAS (prev_n), not where it is
    turned = nrm.copy()
    turned[patch_now, :3] = (0.6, 0.0, 0.8)
    a = list(base)
    a[4] = turned
    _, _, hm3 = capi.debug_filter_temporal_motion(None, *a, prev_pos, prev_n, desc)
    assert (hm3[inner][:, 2] == 6).all()
    _, _, hm4 = capi.debug_filter_temporal_motion(None, *a, prev_pos, turned, desc)
    assert (hm4[inner][:, 2] == 1).all()


# ---- the Cornell sequence of the GPU tests: which object moves, and where the history must survive

SHORT_BOX = ((-0.06, -0.78, -0.01), (0.71, -0.02, 0.61))      # the golden Cornell box's short block: every vertex inside, no other triangle's
STEP = (0.004, 0.0, 0.0)                                      # per frame: about a pixel at 128 x 128 on the block's faces


def moving_triangles(tris, box=SHORT_BOX):
    """the triangles with all three vertices inside `box`"""
    P = positions(tris)
    lo, hi = np.array(box[0], f32), np.array(box[1], f32)
    sel = ((P >= lo) & (P <= hi)).all((1, 2))
    assert sel.any() and not sel.all()
    return sel


def pose(tris, sel, k, step=STEP):
    """the selected triangles translated by k * step (float32)"""
    P = positions(tris).copy()
    P[sel] = (P[sel] + f32(k) * np.array(step, f32)).astype(f32)
    return moved(tris, P)


def eroded(bad, r=2):
    """pixels within Chebyshev distance r of a bad one"""
    H, W = bad.shape
    out = bad.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            out[ys, xs] |= bad[yq, xq]
    return out


def stable_pixels(frames, r=2):
    """frames: per frame (valid bool[h, w], moving bool[h, w], normal float32[h, w, 3]).  The pixels p that in every frame k are valid and whose
    neighbours q within Chebyshev distance r, in frame k AND in frame k - 1, are valid, of p's class in frame k and keep dot(n_q, n_p) >= 0.9: a
    2 x 2 tap of a reprojection that moves less than r - 1 pixels then lies on the surface p itself lies on.  (Frame k - 1's neighbours are compared with
    p's values in frame k: the tap is tested against what p is now.)"""
    H, W = frames[0][0].shape
    S = np.ones((H, W), bool)
    for k, (valid, moving, n) in enumerate(frames):
        S &= valid
        for j in ([k] if k == 0 else [k, k - 1]):
            vq, mq, nq = frames[j]
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                    yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                    same = vq[yq, xq] & (mq[yq, xq] == moving[ys, xs]) & ((nq[yq, xq] * n[ys, xs]).sum(-1) >= 0.9)
                    S[ys, xs] &= same
    return S


def numpy_first_hits(tris, cam, W, H):
    """(primitive int[h, w] (-1: none), u, v, depth) of the pixel-centre rays, Moeller-Trumbore in binary64"""
    d = np.stack(guide_dirs(cam, W, H), -1).astype(f64)
    o = np.array(vec(cam, "position"), f64)
    P = positions(tris).astype(f64)
    best = np.full((H, W), np.inf)
    prim = np.full((H, W), -1)
    bu, bv = np.zeros((H, W)), np.zeros((H, W))
    for i in range(len(P)):
        e1, e2 = P[i, 1] - P[i, 0], P[i, 2] - P[i, 0]
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - P[i, 0]
            u = (pv @ tv) * inv
            qv = np.cross(tv, e1)
            v = (d * qv).sum(-1) * inv
            t = (qv @ e2) * inv
        hit = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6) & (t < best)
        best[hit], prim[hit], bu[hit], bv[hit] = t[hit], i, u[hit], v[hit]
    return prim, bu, bv, best


def test_the_cornell_sequence_leaves_enough_stable_pixels(golden_scenes, golden_radiance):
    """What tests/test_gpu_motion_filter.py asserts on the device's guides, with first hits traced here: the short block moves about a pixel per frame, and
    the pixels whose history must survive 8 frames are at least a quarter of the image and include the block."""
    tris = golden_scenes["cornell"]["triangles"]
    cam = golden_radiance["cornell_64_b4_s2/camera"]
    W = H = 128
    sel = moving_triangles(tris)
    assert sel.sum() == 10
    frames, shift = [], 0.0
    for k in range(8):
        now = pose(tris, sel, k)
        prim, u, v, _ = numpy_first_hits(now, cam, W, H)
        valid = prim >= 0
        moving = valid & sel[np.maximum(prim, 0)]
        N = normals(now).astype(f64)[np.maximum(prim, 0)]
        n = N[..., 0, :] * (1 - u - v)[..., None] + N[..., 1, :] * u[..., None] + N[..., 2, :] * v[..., None]
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        frames.append((valid, moving, n))
    S = stable_pixels(frames)
    moving_in_S = (S & frames[-1][1]).sum()
    print("stable pixels: %.3f of the image, %d of them on the moving block" % (S.mean(), moving_in_S))
    assert S.mean() >= 0.25 and moving_in_S > 0
