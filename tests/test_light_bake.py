"""Light bakes without a device: the items of a light bake -- rt_debug_light_bake_rays(NULL, ...), the host restatement that k_bake_light
and k_light_bake_rays share (raytracing_amd/csrc/light_bake.h) -- and its reduction rt_debug_light_bake_reduce against numpy in the stated order, bit for bit;
the exact cases of the lights' terms; the environment look-up; skipped points; the refusals that need no GPU; and the condition that keeps
tests/test_gpu_light_bake.py from passing on verdicts that are all alike, pinned here with the oracle's any-hit verdicts."""
import ctypes as C
import numpy as np
import pytest
from raytracing_amd import capi, scenes, types as T
from tests.test_bake import (BakeCase, bake_cases, back_faced, random_points, np_points, np_frame, np_rays, mix32, INVALID, SKIP_KINDS)     # noqa: F401 (a fixture)
from tests.test_gpu_pose import city          # noqa: F401 (a fixture)

f32, f64, u32 = np.float32, np.float64, np.uint32
PI, TWO_PI, INV_PI, INV_TWO_PI = f32(3.14159265359), f32(6.28318530718), f32(0.31830988618), f32(0.15915494309)
H = f64.fromhex
SKY_DISTANCE = 20000.0


# ---- rt_detmath.h's atan2 and acos in numpy: binary64 + - * / sqrt in the header's order, rounded once

def atan01(a):
    i = (a * f64(4.0) + f64(0.5)).astype(np.int64)
    c = i.astype(f64) * f64(0.25)
    base = np.select([i == 0, i == 1, i == 2, i == 3], [f64(0.0), H("0x1.f5b75f92c80ddp-3"), H("0x1.dac670561bb4fp-2"), H("0x1.4978fa3269ee1p-1")], H("0x1.921fb54442d18p-1"))
    u = (a - c) / (f64(1.0) + a * c)
    z = u * u
    p = f64(1.0 / 21.0)
    for k in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = f64(1.0 / k) - p * z
    return base + (u - (u * z) * p)


def atan2(y, x):
    with np.errstate(all="ignore"):
        xneg, yneg = np.signbit(x), np.signbit(y)
        ax, ay = np.abs(x), np.abs(y)
        small = ay <= ax
        q = np.where(small, ay / np.where(ax == 0, f64(1.0), ax), ax / np.where(ay == 0, f64(1.0), ay))
        r = np.where(small, atan01(q), H("0x1.921fb54442d18p+0") - atan01(q))
        r = np.where((ax == 0) & (ay == 0), f64(0.0), r)
        r = np.where(xneg, H("0x1.921fb54442d18p+1") - r, r)
        r = np.where(yneg, -r, r)
        return np.where(np.isnan(x) | np.isnan(y), x + y, r)


def atan2f(y, x):
    return atan2(y.astype(f64), x.astype(f64)).astype(f32)


def acosf(z):
    with np.errstate(all="ignore"):
        zd = z.astype(f64)
        return (f64(2.0) * atan2(np.sqrt(f64(1.0) - zd), np.sqrt(f64(1.0) + zd))).astype(f32)


# ---- light_bake.h in numpy

def np_normalize3(v):
    with np.errstate(all="ignore"):
        l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        return (v / l[..., None]).astype(f32)


def np_sample_sky(env, d):
    """SampleSky's arithmetic over float32[..., 3] directions (already normalised and clamped)"""
    h, w = env.shape[:2]
    with np.errstate(all="ignore"):
        cx = atan2f(d[..., 0], d[..., 1]) + PI
        cy = acosf(d[..., 2])
        cx = np.where(cx < 0, cx + TWO_PI, cx)
        cx = cx * INV_TWO_PI
        cy = cy * INV_PI
        u = (cx - np.floor(cx)) * f32(w)
        v = (cy - np.floor(cy)) * f32(h)
        fu, fv = np.floor(u - f32(0.5)), np.floor(v - f32(0.5))
        i0 = np.where(np.isnan(fu), 0, np.nan_to_num(fu)).astype(np.int64)
        j0 = np.where(np.isnan(fv), 0, np.nan_to_num(fv)).astype(np.int64)
        i1, j1 = i0 + 1, j0 + 1
        i0 = np.where(i0 < 0, w + i0, i0); i1 = np.where(i1 > w - 1, i1 - w, i1)
        j0 = np.where(j0 < 0, h + j0, j0); j1 = np.where(j1 > h - 1, j1 - h, j1)
        a, b = (u - f32(0.5)) - fu, (v - f32(0.5)) - fv
        wa0, wb0 = f32(1.0) - a, f32(1.0) - b
        w00, w10, w01, w11 = (wa0 * wb0)[..., None], (a * wb0)[..., None], (wa0 * b)[..., None], (a * b)[..., None]
        t00, t10, t01, t11 = env[j0, i0, :3], env[j0, i1, :3], env[j1, i0, :3], env[j1, i1, :3]
        out = w00 * t00 + w10 * t10 + w01 * t01 + w11 * t11
    assert out.dtype == f32
    return out


def np_sky(env, direction, clamp=True):
    d = np_normalize3(direction)
    if clamp:
        d[..., 2] = np.where(d[..., 2] > 1, f32(1.0), np.where(d[..., 2] < -1, f32(-1.0), d[..., 2]))
    return np_sample_sky(env, d)


def np_items(points, samples, lights, seed=0, bias=1e-3, sky_distance=SKY_DISTANCE, from_surfaces=False, sky=True, use_lights=True, first_index=0):
    """(types.ray[n, samples + M], E float32[n, M, 3], walked[n]): every item's ray (zeros: none) and every light item's contribution"""
    pos, nrm, ok = np_points(points, from_surfaces)
    walked, nn, _, _, origin = np_frame(pos, nrm, ok, bias)
    n, M = len(pos), len(lights)
    rays = np.zeros((n, samples + M), T.ray)
    sky_rays, _ = np_rays(points, samples, seed, bias, sky_distance, from_surfaces, first_index)
    if sky:
        rays[:, :samples] = sky_rays
    E = np.zeros((n, M, 3), f32)
    lo = np.stack([lights["origin"][q] for q in "xyz"], -1).astype(f32).reshape(M, 3)
    lr = np.stack([lights["radiance"][q] for q in "xyz"], -1).astype(f32).reshape(M, 3)
    with np.errstate(all="ignore"):
        for j in range(M if use_lights else 0):
            point = lights["type"][j] == 0
            v = (lo[j][None] - origin) if point else np.broadcast_to(lo[j][None], origin.shape).astype(f32)
            d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            c = ((nn[:, 0] * v[:, 0] + nn[:, 1] * v[:, 1]) + nn[:, 2] * v[:, 2]) / np.sqrt(d2)
            made = walked & np.isfinite(origin).all(1) & np.isfinite(v).all(1) & np.isfinite(lr[j]).all() & (d2 > 0) & np.isfinite(d2) & (c > 0)
            if point:
                d, t_max, e = v, f32(1.0), (lr[j][None] / d2[:, None]) * c[:, None]
            else:
                d, t_max, e = np_normalize3(v), f32(sky_distance), lr[j][None] * c[:, None]
            assert e.dtype == f32 and d.dtype == f32
            E[:, j] = np.where(made[:, None], e, f32(0.0))
            r = rays[:, samples + j]
            for q, name in enumerate("xyz"):
                r["origin"][name] = np.where(made, origin[:, q], f32(0.0))
                r["direction"][name] = np.where(made, d[:, q], f32(0.0))
            r["direction"]["w"] = np.where(made, t_max, f32(0.0))
            rays[:, samples + j] = r
    return rays, E, walked


def tree(v, L):
    s = L // 2
    while s:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return v[:, 0]


def np_light_bake(points, samples, occluded, lights, env, **kw):
    rays, E, walked = np_items(points, samples, lights, **kw)
    n, M, L = len(walked), len(lights), min(samples, 64)
    made = (np.stack([rays["direction"][q] for q in "xyz"], -1) != 0).any(-1)
    adds = made & (np.asarray(occluded).reshape(n, samples + M) == 0)
    d = np.stack([rays["direction"][q][:, :samples] for q in "xyz"], -1).astype(f32)
    rgb = np_sky(env, d) if env is not None else np.zeros_like(d)
    sky = np.zeros((n, L, 3), f32)
    for j in range(samples // L):                                   # slot l adds its items l, l + L, ... in rising r
        sl = slice(j * L, (j + 1) * L)
        sky = sky + np.where(adds[:, sl, None], rgb[:, sl], f32(0.0))
    lit = np.zeros((n, L, 3), f32)
    Mp = -(-M // L) * L                                             # light j is item samples + j: slot j % L (samples is a multiple of L)
    Ep = np.zeros((n, Mp, 3), f32); Ep[:, :M] = E
    ap = np.zeros((n, Mp), bool); ap[:, :M] = adds[:, samples:]
    for j in range(Mp // L):
        sl = slice(j * L, (j + 1) * L)
        lit = lit + np.where(ap[:, sl, None], Ep[:, sl], f32(0.0))
    out = np.zeros(n, T.light_bake_result)
    S = tree(sky, L) * (PI / f32(samples))
    assert S.dtype == f32
    out["sky"] = np.where(walked[:, None], S, f32(0.0))
    out["lights"] = np.where(walked[:, None], tree(lit, L), f32(0.0))
    out["sky_unoccluded"] = np.where(walked, adds[:, :samples].sum(1), INVALID)
    out["lights_unshadowed"] = np.where(walked, adds[:, samples:].sum(1), INVALID)
    return out


# ---- fixtures of this file and of tests/test_gpu_light_bake.py

def random_lights(rng, M):
    lg = np.zeros(M, T.light)
    for q in "xyz":
        lg["origin"][q] = rng.normal(size=M) * 4
        lg["radiance"][q] = rng.uniform(0, 20, M)
    lg["type"] = rng.integers(0, 2, M)
    if M >= 3:
        lg["type"][2] = 7                                           # any type but the point light's is directional
    if M >= 70:
        lg["radiance"]["y"][5] = np.inf; lg["origin"]["x"][6] = np.nan; lg["origin"][7] = (0, 0, 0, 0); lg["type"][7] = 1     # items without a ray
    return lg


def random_env(rng, w=7, h=5):
    env = rng.uniform(0, 3, (h, w, 4)).astype(f32)
    env[..., 3] = np.nan                                            # the ignored lane
    return env


def scene_lights(case):
    """scenes.make_lights for a bake case: one directional light, a point light inside the scene's box, one far outside it (behind the walls), and one
    coincident with a baked point (filled in by the caller: with_coincident)"""
    from tests.test_refit import positions
    p = positions(case.scene["triangles"]).reshape(-1, 3)
    lo, hi = p.min(0).astype(f64), p.max(0).astype(f64)
    mid, ext = (lo + hi) / 2, hi - lo
    inside = mid + ext * np.array([0.11, -0.07, 0.23])
    outside = mid + ext * np.array([3.0, 2.5, 0.4])
    return scenes.make_lights(directional=[((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))],
                              point=[(tuple(inside), (30.0, 20.0, 40.0)), (tuple(outside), (50.0, 50.0, 50.0)), (tuple(mid), (9.0, 9.0, 9.0))])


def lights_of(case, M, coincident_with=None):
    """M lights for a bake case: scene_lights' four repeated with their radiance varied; light 3 moved onto the position of a baked point"""
    base = scene_lights(case)
    if coincident_with is not None:
        for k, q in enumerate("xyz"):
            base["origin"][q][3] = coincident_with[k]
    lg = np.zeros(M, T.light)
    for j in range(M):
        lg[j] = base[[1, 0, 2, 3][j % 4]]                           # M = 1: the point light inside
        for q in "xyz":
            lg["radiance"][q][j] *= f32(1 + j // 4)
    return lg


class LightCase:
    """a BakeCase with lights and gradient_env: the scene a light bake is uploaded with, and what the host says it gives"""

    def __init__(self, bake_case, M, n):
        self.base, self.n = bake_case, n
        self.pts = bake_case.points(n)
        walked = np.flatnonzero(np_frame(*np_points(self.pts, False), bake_case.bias)[0])
        self.lights = lights_of(bake_case, M, self.pts[walked[0], 0:3] if len(walked) else None)
        self.env = scenes.gradient_env()
        self.scene = dict(bake_case.scene); self.scene["lights"] = self.lights; self.scene["env"] = self.env
        self.bias, self.sky_distance = bake_case.bias, bake_case.radius

    def expected(self, points, samples, seed=0, from_surfaces=False, first_index=0, sky=True, use_lights=True, lights=None):
        lg = self.lights if lights is None else lights
        kw = dict(seed=seed, bias=self.bias, sky_distance=self.sky_distance, from_surfaces=from_surfaces, sky=sky, use_lights=use_lights, first_index=first_index)
        rays = capi.debug_light_bake_rays(None, points, samples, lg, **kw)
        return capi.debug_light_bake_reduce(points, samples, self.base.verdicts(rays), lg, self.env, **kw), rays


# ---- 1. the numpy restatement

def surfaces(rng, n):
    s = np.zeros(n, T.surface)
    s["position"] = rng.normal(size=(n, 3)) * 2; s["shading_normal"] = rng.normal(size=(n, 3))
    s["geometric_normal"] = rng.normal(size=(n, 3)); s["t"] = 5; s["primitive_id"] = np.arange(n)
    s["flags"] = np.where(np.arange(n) % 3 == 0, 3, 1)               # every third meets its back face
    s["flags"][4] = 0; s["flags"][10] = 2                            # miss records
    s["shading_normal"][7] = np.nan
    return s


@pytest.mark.parametrize("samples", [16, 64, 256])
@pytest.mark.parametrize("M", [0, 1, 3, 70])
def test_host_equals_numpy_bit_for_bit(samples, M):
    """Every operation of light_bake.h has the same IEEE operation in numpy, so nothing here is compared with a tolerance."""
    rng = np.random.default_rng(1000 * samples + M)
    env, lg = random_env(rng), random_lights(rng, M)
    for points, from_surfaces in ((random_points(rng, 41), False), (surfaces(rng, 23), True)):
        n = len(points)
        for sky, use_lights, first in ((True, True, 0), (False, True, 5), (True, False, 0xFFFFFFF0), (False, False, 0)):
            kw = dict(seed=7 + M, bias=0.01, sky_distance=9.5, from_surfaces=from_surfaces, sky=sky, use_lights=use_lights, first_index=first)
            got = capi.debug_light_bake_rays(None, points, samples, lg, **kw)
            want, E, walked = np_items(points, samples, lg, **kw)
            assert got.shape == (n, samples + M)
            assert got.tobytes() == want.tobytes(), (samples, M, sky, use_lights)
            assert not got[~walked].tobytes().strip(b"\0") and (~walked).sum() >= 3 and walked.sum() * 2 >= n
            if not sky: assert not got[:, :samples].tobytes().strip(b"\0")
            if not use_lights: assert not got[:, samples:].tobytes().strip(b"\0")
            occ = (rng.uniform(size=(n, samples + M)) < rng.uniform(0, 1, (n, 1))).astype(u32) * rng.integers(1, 9, (n, samples + M)).astype(u32)
            occ[0] = 0; occ[2] = 1
            res = capi.debug_light_bake_reduce(points, samples, occ, lg, env, **kw)
            ref = np_light_bake(points, samples, occ, lg, env, **kw)
            assert res.tobytes() == ref.tobytes(), [(k, res[k][:4], ref[k][:4]) for k in T.light_bake_result.names if res[k].tobytes() != ref[k].tobytes()]
            assert (res["sky_unoccluded"][~walked] == INVALID).all() and (res["lights_unshadowed"][~walked] == INVALID).all()
            assert not res["sky"][~walked].any() and not res["lights"][~walked].any()
            if sky and walked[0]: assert res["sky_unoccluded"][0] == samples
            if M >= 3 and use_lights:
                made = (got["direction"]["w"][:, samples:] != 0)
                assert made.any() and not made.all()                                   # lights above and below the horizon
                assert (res["lights_unshadowed"][walked] <= made[walked].sum(1)).all()


def test_sky_rays_are_the_occlusion_bakes():
    rng = np.random.default_rng(3)
    pts = random_points(rng, 20)
    a = capi.debug_light_bake_rays(None, pts, 64, None, seed=9, bias=0.125, sky_distance=3.0, first_index=4)
    b = capi.debug_bake_rays(None, pts, 64, 9, 0.125, 3.0, first_index=4)
    assert a.tobytes() == b.tobytes()


# ---- 2. exact cases

def up_point(z=0.0):
    p = np.zeros((1, 8), f32); p[0, 2] = z; p[0, 6] = 2.0          # a normal of length 2: the frame normalises it exactly
    return p


def test_point_light_overhead_is_exact():
    h = 4.0
    lg = scenes.make_lights(point=[((0.0, 0.0, h), (8.0, 32.0, 0.5))])
    out = capi.debug_light_bake_reduce(up_point(), 16, np.zeros((1, 17), u32), lg, None, bias=0.0, sky=False)
    assert out["lights"][0].tolist() == [8.0 / 16, 32.0 / 16, 0.5 / 16] and out["lights_unshadowed"][0] == 1 and out["sky_unoccluded"][0] == 0
    rays = capi.debug_light_bake_rays(None, up_point(), 16, lg, bias=0.0, sky=False)
    r = rays[0, 16]
    assert tuple(r["direction"]) == (0.0, 0.0, h, 1.0) and tuple(r["origin"]) == (0.0, 0.0, 0.0, 0.0)      # the segment ends at the light
    shadowed = capi.debug_light_bake_reduce(up_point(), 16, np.ones((1, 17), u32), lg, None, bias=0.0, sky=False)
    assert not shadowed["lights"].any() and shadowed["lights_unshadowed"][0] == 0
    sun = scenes.make_lights(directional=[((0.0, 0.0, 2.0), (3.0, 5.0, 7.0))])                            # straight above: c = 1, E = radiance
    out = capi.debug_light_bake_reduce(up_point(), 16, np.zeros((1, 17), u32), sun, None, bias=0.0, sky=False, sky_distance=64.0)
    assert out["lights"][0].tolist() == [3.0, 5.0, 7.0]
    assert tuple(capi.debug_light_bake_rays(None, up_point(), 16, sun, bias=0.0, sky=False, sky_distance=64.0)[0, 16]["direction"]) == (0.0, 0.0, 1.0, 64.0)


def test_lights_that_make_no_ray():
    lg = scenes.make_lights(directional=[((0.0, 1.0, -1.0), (1.0, 1.0, 1.0)), ((1.0, 0.0, 0.0), (1.0, 1.0, 1.0))],       # below the horizon; on it (c = 0)
                            point=[((0.0, 0.0, -3.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 1.0), (np.nan, 1.0, 1.0)),
                                   ((0.0, np.inf, 1.0), (1.0, 1.0, 1.0))])                                                 # below; at the origin (d2 = 0); not finite
    rays = capi.debug_light_bake_rays(None, up_point(), 16, lg, bias=0.0)
    assert not rays[0, 16:].tobytes().strip(b"\0") and rays[0, :16].tobytes().strip(b"\0")
    out = capi.debug_light_bake_reduce(up_point(), 16, np.zeros((1, 22), u32), lg, scenes.gradient_env(), bias=0.0)
    assert out["lights_unshadowed"][0] == 0 and not out["lights"].any() and out["sky_unoccluded"][0] == 16


# ---- 3. the environment

@pytest.mark.parametrize("samples", [16, 256, 4096])
def test_constant_environment_gives_pi_times_its_value(samples):
    """Roundings: a four-term bilinear blend of equal texels, at most 64 adds per slot, six tree levels, one scale: under 100 * 2^-24 relative < 1e-5."""
    rng = np.random.default_rng(samples)
    pts = random_points(rng, 24, spoiled=False)
    value = np.array([0.75, 2.5, 0.01], f32)
    env = np.zeros((8, 16, 4), f32); env[..., :3] = value
    out = capi.debug_light_bake_reduce(pts, samples, np.zeros((24, samples), u32), None, env)
    want = np.pi * value.astype(f64)
    assert np.abs(out["sky"].astype(f64) / want - 1).max() < 1e-5 and (out["sky_unoccluded"] == samples).all()
    half = np.zeros((24, samples), u32); half[:, ::2] = 1
    out = capi.debug_light_bake_reduce(pts, samples, half, None, env)
    assert np.abs(out["sky"].astype(f64) / (want / 2) - 1).max() < 1e-5 and (out["sky_unoccluded"] == samples // 2).all()


def inverse_mix32(x):
    def unshift(v, s):
        r = v
        for _ in range(32 // s + 1):
            r = v ^ (r >> s)
        return r
    x = unshift(x, 16); x = (x * pow(0x846ca68b, -1, 1 << 32)) & 0xFFFFFFFF
    x = unshift(x, 15); x = (x * pow(0x7feb352d, -1, 1 << 32)) & 0xFFFFFFFF
    return unshift(x, 16)


def test_no_nan_at_the_poles_and_the_clamp():
    """acos of a z one ulp above 1 is NaN, and SampleSky's rule then reads texel (0, 0) with NaN weights: a NaN sample.  The look-up clamps z first.  Ray 0 of
    the point whose rotation r1 is 1 - 0.5 / samples has u1 = 0: its direction is the frame's normal itself, so normals at and beside both poles put rays
    exactly there; the restatement above, checked bit for bit against the host's, shows what the clamp is for with a z one ulp outside on either side."""
    env = scenes.gradient_env()
    samples, seed = 16, 0
    index = inverse_mix32(0xF8000000) ^ int(mix32(np.array([seed], u32))[0])           # h1 >> 8 = 31/32 * 2^24
    normals = [(0, 0, 1), (0, 0, -1), (1e-4, 0, 1), (0, -3e-4, -1), (1e-8, 1e-8, 1), (2e-4, 1e-4, 0.7)]
    pts = np.zeros((len(normals), 8), f32); pts[:, 4:7] = normals
    for p in range(len(pts)):
        one = pts[p:p + 1]
        rays = capi.debug_light_bake_rays(None, one, samples, None, seed=seed, bias=0.0, first_index=index)
        n = np_frame(*np_points(one, False), 0.0)[1][0]
        assert tuple(rays[0, 0]["direction"])[:3] == tuple(n)                            # u1 = 0: the normal itself
        out = capi.debug_light_bake_reduce(one, samples, np.zeros((1, samples), u32), None, env, seed=seed, bias=0.0, first_index=index)
        assert np.isfinite(out["sky"]).all() and out["sky_unoccluded"][0] == samples
    above = np.array([[0, 0, np.nextafter(f32(1), f32(2))], [0, 0, np.nextafter(f32(-1), f32(-2))]], f32)
    assert np.isnan(np_sample_sky(env, above)).all()                                     # SampleSky's own rule: NaN, and no address outside the image
    inside = np.array([[0, 0, 1], [0, 0, -1]], f32)
    assert np.isfinite(np_sample_sky(env, inside)).all()
    clamped = above.copy(); clamped[:, 2] = np.clip(clamped[:, 2], -1, 1)
    assert np_sample_sky(env, clamped).tobytes() == np_sample_sky(env, inside).tobytes()


# ---- 4. records, exports, refusals

def test_record_layout_and_exports():
    names = T.light_bake_result.names
    assert T.light_bake_result.itemsize == 32 and {k: T.light_bake_result.fields[k][1] for k in names} == dict(sky=0, sky_unoccluded=12, lights=16, lights_unshadowed=28)
    assert C.sizeof(capi.rt_light_bake_desc) == 20
    header = open(capi._HERE + "/../include/rt_hip.h").read()
    assert "RT_STATIC_ASSERT(sizeof(rt_light_bake_result) == 32" in header and "#define RT_LIGHT_BAKE_NO_SKY    2u" in header and "#define RT_LIGHT_BAKE_NO_LIGHTS 4u" in header
    for name in ("rt_scene_light_bake", "rt_scene_light_bake_buffer", "rt_scene_atlas_bake_light", "rt_debug_light_bake_rays", "rt_debug_light_bake_reduce"):
        assert name in capi.EXPORTS and hasattr(capi.load(), name)


def test_refusals_without_a_device():
    lib = capi.load()
    pts, out, rays = random_points(np.random.default_rng(0), 4), np.zeros(4, T.light_bake_result), np.zeros((4, 18), T.ray)
    occ, lg, env = np.zeros((4, 18), u32), random_lights(np.random.default_rng(1), 2), scenes.gradient_env(8, 4)
    err = lambda: lib.rt_last_error(None).decode()
    p = lambda a: a.ctypes.data
    D = capi.light_bake_desc
    good = D(16, 0, 1e-3, 1.0)
    atlas = capi.atlas_desc(4, 4)
    assert lib.rt_scene_light_bake(None, p(pts), 4, C.byref(good), p(out)) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_light_bake(None, None, 0, None, None) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_light_bake_buffer(None, None, 4, C.byref(good), None) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_atlas_bake_light(None, C.byref(atlas), None, C.byref(good), p(out), None, None) != 0 and "ctx is NULL" in err()
    bad = [(D(0), "power of two"), (D(8), "power of two"), (D(48), "power of two"), (D(8192), "power of two"), (D(16, bias=np.nan), "bias"), (D(16, bias=np.inf), "bias"),
           (D(16, sky_distance=0.0), "sky_distance"), (D(16, sky_distance=-1.0), "sky_distance"), (D(16, sky_distance=np.inf), "sky_distance"),
           (D(16, sky_distance=np.nan), "sky_distance"), (D(16, flags=8), "unknown flag"), (D(16, flags=0x80000001), "unknown flag")]
    reduce = lambda d, pp=p(pts), ll=p(lg), ee=p(env), oo=p(occ), rr=p(out), m=2: lib.rt_debug_light_bake_reduce(pp, 4, 0, d, ll, m, ee, 8, 4, oo, rr)
    for d, text in bad:
        assert lib.rt_debug_light_bake_rays(None, p(pts), 4, 0, C.byref(d), p(lg), 2, p(rays)) != 0 and text in err(), (text, err())
        assert reduce(C.byref(d)) != 0 and text in err(), (text, err())
    g = C.byref(good)
    for args in ((None, 4, 0, g, p(lg), 2, p(rays)), (p(pts), 4, 0, None, p(lg), 2, p(rays)), (p(pts), 4, 0, g, p(lg), 2, None), (p(pts), 4, 0, g, None, 2, p(rays))):
        assert lib.rt_debug_light_bake_rays(None, *args) != 0 and "NULL argument" in err()
    assert lib.rt_debug_light_bake_rays(None, p(pts), 1 << 20, 0, C.byref(D(4096)), None, 0, p(rays)) != 0 and "2^28" in err()
    assert lib.rt_debug_light_bake_rays(None, p(pts), 4, 0, g, p(lg), 0x80000000, p(rays)) != 0 and "2^28" in err()
    assert lib.rt_debug_light_bake_rays(None, None, 0, 0, None, None, 0, None) == 0                          # n == 0 does nothing
    for kw in (dict(pp=None), dict(d=None), dict(ll=None), dict(oo=None), dict(rr=None)):
        assert reduce(**dict(dict(d=g), **kw)) != 0 and "NULL argument" in err()
    assert reduce(g, ee=None) != 0 and "no environment image" in err()
    assert lib.rt_debug_light_bake_reduce(p(pts), 4, 0, g, p(lg), 2, p(env), 0, 4, p(occ), p(out)) != 0 and "no environment image" in err()
    assert reduce(C.byref(D(16, sky_distance=1.0, sky=False)), ee=None) == 0                                  # no sky asked for: no image needed
    assert not out["sky"].any() and (out["sky_unoccluded"][out["sky_unoccluded"] != INVALID] == 0).all()
    out[:] = 0
    assert lib.rt_debug_light_bake_reduce(None, 0, 0, None, None, 0, None, 0, 0, None, None) == 0
    assert out.tobytes() == bytes(out.nbytes) and rays.tobytes() == bytes(rays.nbytes)                        # the refusals wrote nothing
    with pytest.raises(capi.RtError, match="one verdict per item"):
        capi.debug_light_bake_reduce(pts, 16, occ[:3], lg, env)
    with pytest.raises(capi.RtError, match="float32\\[h, w, 4\\]"):
        capi.debug_light_bake_reduce(pts, 16, occ, lg, env[..., :3])
    try:
        ctx = capi.Context(0)
    except capi.RtError as e:
        assert "no HIP device" in str(e)
        return
    try:
        with pytest.raises(capi.RtError, match="no scene uploaded"):
            ctx.bake_light(pts, 16)
    finally:
        ctx.close()


# ---- 5. the light bakes of the GPU tests are not vacuous

GPU_SHAPES = [(16, (1, 7)), (64, (1, 5)), (256, (1, 3))]        # four points per wave with a partly filled last wave; one point per wave; four refills per lane
GPU_LIGHTS = [0, 1, 3, 70]                                      # more lights than slots at every L


@pytest.mark.parametrize("name", ["cornell", "coverage"])
def test_non_vacuity(bake_cases, name):
    """Over the cases tests/test_gpu_light_bake.py compares, the oracle's verdicts leave some point with 0 < sky_unoccluded < samples, and light items both
    shadowed and unshadowed: a device that answered all-free or all-blocked could not pass."""
    partial = shadowed = unshadowed = coincident = 0
    for M in GPU_LIGHTS:
        for samples, counts in GPU_SHAPES:
            for n in counts:
                case = LightCase(bake_cases[name], M, n)
                want, rays = case.expected(case.pts, samples, seed=n)
                walked = want["sky_unoccluded"] != INVALID
                partial += int((walked & (want["sky_unoccluded"] > 0) & (want["sky_unoccluded"] < samples)).sum())
                made = (rays["direction"]["w"][:, samples:] != 0).sum(1)
                unshadowed += int(want["lights_unshadowed"][walked].sum())
                shadowed += int((made[walked] - want["lights_unshadowed"][walked]).sum())
                if M >= 4 and walked.any():
                    first = np.flatnonzero(walked)[0]
                    coincident += int(not rays[first, samples + 3].tobytes().strip(b"\0"))     # the light on the point itself: behind the biased origin, no ray
    print(name, "partially occluded points", partial, "light items shadowed", shadowed, "unshadowed", unshadowed, "coincident without a ray", coincident)
    assert partial > 0 and shadowed > 0 and unshadowed > 0 and coincident > 0
