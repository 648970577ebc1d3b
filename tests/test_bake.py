"""Occlusion bakes without a device: the rays of a bake -- rt_debug_bake_rays(NULL, ...), the host restatement that k_bake and k_bake_rays
share (raytracing_amd/csrc/bake.h) -- against numpy, bit for bit; the reduction rt_debug_bake_reduce against numpy in the stated order, bit for bit; the
conversion from rt_surface records; the refusals that need no GPU; and the condition that keeps tests/test_gpu_bake.py from passing on all-zero or all-full
counts, pinned here with the oracle's any-hit verdicts."""
import ctypes as C
import os
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _oracle
from tests.test_wide_bvh import wide_of
from tests.test_refit import positions
from tests.test_gpu_query import camera_rays
from tests.test_gpu_pose import city          # noqa: F401 (a fixture)

f32, f64, u32 = np.float32, np.float64, np.uint32
INVALID = 0xFFFFFFFF
TWO_PI = f32(6.28318530718)                    # RT_TWO_PI
SAMPLES = [16, 32, 64, 256, 4096]

# the bake of each test scene: radius as a fraction of the diagonal of the triangles' bounding box, bias likewise.  Chosen so that test_non_vacuity below
# holds (what it measured, 257 points, 64 samples: cornell 257 walked / 206 partially occluded, coverage 257 / 240, city 244 / 225)
RADIUS_FRACTION = {"cornell": 0.25, "coverage": 0.25, "city": 0.05}
BIAS_FRACTION = 1e-4


# ---- bake.h in numpy: every operation the binary32 (or, in the sine and cosine, binary64) one of the header, in its order

def mix32(x):
    x = x.astype(u32)
    x = x ^ (x >> u32(16)); x = x * u32(0x7feb352d)
    x = x ^ (x >> u32(15)); x = x * u32(0x846ca68b)
    return x ^ (x >> u32(16))


def bitreverse32(k):
    return np.array([int("{:032b}".format(int(v))[::-1], 2) for v in k], u32)


def ksin(r):
    z = r * r
    p = f64(1.0 / 355687428096000.0)
    for c, sign in ((1307674368000.0, -1), (6227020800.0, 1), (39916800.0, -1), (362880.0, 1), (5040.0, -1), (120.0, 1), (6.0, -1)):
        p = p * z + f64(1.0 / c) if sign > 0 else p * z - f64(1.0 / c)
    return r + (r * z) * p


def kcos(r):
    z = r * r
    p = f64(1.0 / 6402373705728000.0)
    for c in (20922789888000.0, 87178291200.0, 479001600.0, 3628800.0, 40320.0, 720.0, 24.0):
        p = f64(1.0 / c) - p * z
    p = f64(0.5) - p * z
    return f64(1.0) - z * p


def sincos(x):
    """rt_detmath.h's rtd_sincos over float64 arrays (0 <= x < 7: the range check never fires)"""
    kf = np.floor(x * f64.fromhex("0x1.45f306dc9c883p-1") + f64(0.5))
    r = (x - kf * f64.fromhex("0x1.921fb54400000p+0")) - kf * f64.fromhex("0x1.0b4611a626331p-34")
    q = kf.astype(np.int64) & 3
    sr, cr = ksin(r), kcos(r)
    s = np.select([q == 0, q == 1, q == 2], [sr, cr, -sr], -cr)
    c = np.select([q == 0, q == 1, q == 2], [cr, -sr, -cr], sr)
    return s, c


def np_points(points, from_surfaces):
    """(position[n, 3], normal[n, 3], record is not a miss[n]) of point rows or surface records"""
    if from_surfaces:
        flags = points["flags"]
        nrm = np.where((flags & 2)[:, None] != 0, -points["shading_normal"], points["shading_normal"]).astype(f32)
        return points["position"].astype(f32), nrm, (flags & 1) != 0
    p = np.asarray(points, f32)
    return p[:, 0:3], p[:, 4:7], np.ones(len(p), bool)


def np_frame(pos, nrm, ok, bias):
    with np.errstate(all="ignore"):
        l2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        walked = ok & np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (l2 > 0) & np.isfinite(l2)
        n = nrm / np.sqrt(l2)[:, None]
        sg = np.copysign(f32(1.0), n[:, 2])
        a = f32(-1.0) / (sg + n[:, 2])
        b = (n[:, 0] * n[:, 1]) * a
        t = np.stack([f32(1.0) + ((sg * n[:, 0]) * n[:, 0]) * a, sg * b, (-sg) * n[:, 0]], -1)
        bt = np.stack([b, sg + (n[:, 1] * n[:, 1]) * a, -n[:, 1]], -1)
        origin = pos + n * f32(bias)
    return walked, n.astype(f32), t.astype(f32), bt.astype(f32), origin.astype(f32)


def np_rays(points, samples, seed=0, bias=1e-3, radius=1.0, from_surfaces=False, first_index=0):
    pos, nrm, ok = np_points(points, from_surfaces)
    walked, n, t, bt, origin = np_frame(pos, nrm, ok, bias)
    i = (np.arange(len(pos), dtype=np.uint64) + np.uint64(first_index)).astype(u32)
    h1 = mix32(i ^ mix32(np.array([seed], u32)))
    h2 = mix32(h1 ^ u32(0x9E3779B9))
    r1 = (h1 >> u32(8)).astype(f32) * f32(2.0 ** -24)
    r2 = (h2 >> u32(8)).astype(f32) * f32(2.0 ** -24)
    k = np.arange(samples, dtype=u32)
    u1 = ((k.astype(f32) + f32(0.5)) / f32(samples))[None] + r1[:, None]
    u1 = np.where(u1 >= 1, u1 - f32(1.0), u1).astype(f32)
    u2 = ((bitreverse32(k) >> u32(8)).astype(f32) * f32(2.0 ** -24))[None] + r2[:, None]
    u2 = np.where(u2 >= 1, u2 - f32(1.0), u2).astype(f32)
    phi = TWO_PI * u2
    assert phi.dtype == f32
    s, c = sincos(phi.astype(f64))
    sn, cs = s.astype(f32), c.astype(f32)
    r = np.sqrt(u1)
    x, y = r * cs, r * sn
    z = np.sqrt(np.maximum(f32(1.0) - u1, f32(0.0)))
    with np.errstate(all="ignore"):
        d = (t[:, None, :] * x[:, :, None] + bt[:, None, :] * y[:, :, None]) + n[:, None, :] * z[:, :, None]
    assert d.dtype == f32
    rays = np.zeros((len(pos), samples), T.ray)
    for q, name in enumerate("xyz"):
        rays["origin"][name] = np.where(walked, origin[:, q], f32(0.0))[:, None]
        rays["direction"][name] = np.where(walked[:, None], d[:, :, q], f32(0.0))
    rays["direction"]["w"] = np.where(walked, f32(radius), f32(0.0))[:, None]
    return rays, walked


def np_reduce(rays, occluded, samples):
    n = rays.shape[0]
    L = min(samples, 64)
    d = np.stack([rays["direction"][q] for q in "xyz"], -1).astype(f32)
    free = np.asarray(occluded).reshape(n, samples) == 0
    v = np.zeros((n, L, 3), f32)
    for j in range(samples // L):                                  # slot l adds its rays l, l + L, ... in rising k
        sl = slice(j * L, (j + 1) * L)
        v = v + np.where(free[:, sl, None], d[:, sl], f32(0.0))    # (a slot's sum is never -0: adding +0 changes nothing)
    s = L // 2
    while s:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    S = v[:, 0]
    with np.errstate(all="ignore"):
        l2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
        good = (l2 > 0) & np.isfinite(l2)
        bent = np.where(good[:, None], S / np.sqrt(l2)[:, None], f32(0.0)).astype(f32)
    skipped = (d[:, 0] == 0).all(1)
    out = np.zeros(n, T.bake_result)
    out["bent_normal"] = np.where(skipped[:, None], f32(0.0), bent)
    out["unoccluded"] = np.where(skipped, INVALID, free.sum(1))
    return out


# ---- points

SKIP_KINDS = 5


def spoil(points, i, kind):
    """make row i of float32[n, 8] a skipped point of one of the kinds"""
    if kind == 0: points[i, 1] = np.nan                    # a NaN position component
    elif kind == 1: points[i, 4] = np.inf                  # an infinite normal component
    elif kind == 2: points[i, 4:7] = 0.0                   # a zero normal
    elif kind == 3: points[i, 4:7] = 1e30                  # a finite normal whose squared length is not
    else: points[i, 4:7] = 1e-30                           # a non-zero normal whose squared length is zero


def random_points(rng, n, spoiled=True):
    pts = np.zeros((n, 8), f32)
    pts[:, 0:3] = rng.normal(size=(n, 3)) * 3
    pts[:, 4:7] = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10, (n, 1))
    pts[:, 3] = np.nan; pts[:, 7] = np.inf                 # the ignored lanes
    if n >= 6:
        pts[0, 4:7] = (0, 0, 1); pts[2, 4:7] = (0, 0, -1)  # both poles of the basis
        pts[3, 4:7] = (1, 0, 0); pts[5, 4:7] = (0, -2, 0)
    if spoiled:
        for j, i in enumerate(range(1, n, 3)):
            spoil(pts, i, j % SKIP_KINDS)
    return pts


def bounds_diagonal(scene):
    p = positions(scene["triangles"]).reshape(-1, 3)
    return float(np.linalg.norm(p.max(0).astype(f64) - p.min(0).astype(f64)))


class BakeCase:
    """a scene, its oracle, the bake's radius and bias, and surface points under its camera (computed once, shared, never changed)"""

    def __init__(self, name, scene, cam):
        self.name, self.scene, self.cam = name, scene, cam
        self.orc = _oracle.Oracle(16, 16, scene)
        self.wide, self.entry = wide_of(scene["nodes"], 1)
        diag = bounds_diagonal(scene)
        self.radius, self.bias = float(f32(RADIUS_FRACTION[name] * diag)), float(f32(BIAS_FRACTION * diag))
        self._surfaces = {}

    def surfaces(self, n, seed=0):
        """the surface records (types.surface) of the oracle's first hits of n camera rays"""
        if (n, seed) not in self._surfaces:
            rays = camera_rays(self.cam, n, np.random.default_rng(4000 + 31 * seed + n))
            hits = self.orc.wide_trace(self.wide, self.entry, rays, False)
            self._surfaces[(n, seed)] = capi.debug_query_surface(None, self.scene["triangles"], rays, hits)
        return self._surfaces[(n, seed)]

    def mixed_rays(self, n, seed):
        """the camera rays of default_rng(seed) with every fourth, from the second, looking the other way: it leaves the scene, so the first hits hold miss
        records (the coverage scene's camera sees no sky)"""
        rays = camera_rays(self.cam, n, np.random.default_rng(seed))
        away = np.arange(n) % 4 == 1
        for k in "xyz":
            rays["direction"][k] = np.where(away, -rays["direction"][k], rays["direction"][k])
        return rays

    def points(self, n, spoiled=True):
        """float32[n, 8] rows of surfaces(n); a miss becomes a skipped point (a zero normal); every third point from the second is spoiled"""
        s = self.surfaces(n)
        pos, nrm, ok = np_points(s, True)
        pts = np.zeros((n, 8), f32)
        pts[:, 0:3], pts[:, 4:7] = pos, np.where(ok[:, None], nrm, f32(0.0))
        if spoiled:
            for j, i in enumerate(range(1, n, 3)):
                spoil(pts, i, j % SKIP_KINDS)
        return pts

    def verdicts(self, rays):
        """the oracle's any-hit verdicts of types.ray[n, samples]; a ray no query walks (a skipped point's zeros) is not occluded"""
        flat = rays.reshape(-1)
        occ = (self.orc.wide_trace(self.wide, self.entry, flat, True) != INVALID).astype(u32)
        zero = (flat["direction"]["x"] == 0) & (flat["direction"]["y"] == 0) & (flat["direction"]["z"] == 0)
        occ[zero] = 0
        return occ.reshape(rays.shape)

    def expected(self, points, samples, seed=0, from_surfaces=False, first_index=0):
        rays = capi.debug_bake_rays(None, points, samples, seed, self.bias, self.radius, from_surfaces, first_index)
        return capi.debug_bake_reduce(rays, self.verdicts(rays), samples)


@pytest.fixture(scope="module")
def bake_cases(golden_scenes, golden_radiance, city):
    return {"cornell": BakeCase("cornell", golden_scenes["cornell"], golden_radiance["cornell_64_b4_s2/camera"]),
            "coverage": BakeCase("coverage", golden_scenes["coverage"], golden_radiance["coverage_64_b6_s2/camera"]),
            "city": BakeCase("city", city, T.default_camera(64, 64))}


# ---- 1. ray generation

@pytest.mark.parametrize("samples", SAMPLES)
def test_host_rays_equal_numpy_bit_for_bit(samples):
    """Every operation of bake.h has the same IEEE operation in numpy (binary32 + - * / sqrt, binary64 + - * floor, the two conversions), so nothing here
    is compared with a tolerance."""
    rng = np.random.default_rng(samples)
    for n, seed, first, bias, radius in ((1, 0, 0, 1e-3, 1.0), (67, 12345, 0, 0.25, 7.5), (9, 0xFFFFFFFF, 0xFFFFFFFA, -0.5, 1e-3)):   # (the index wraps at 2^32)
        pts = random_points(rng, n)
        got = capi.debug_bake_rays(None, pts, samples, seed, bias, radius, first_index=first)
        want, walked = np_rays(pts, samples, seed, bias, radius, first_index=first)
        assert got.shape == (n, samples)
        assert got.tobytes() == want.tobytes(), [k for k in ("origin", "direction") if got[k].tobytes() != want[k].tobytes()]
        assert not got[~walked].tobytes().strip(b"\0")               # a skipped point's rays are zeros
        if n >= 6:
            assert walked.sum() * 2 >= n and (~walked).sum() >= min(SKIP_KINDS, (n + 1) // 3)


def test_ray_properties():
    rng = np.random.default_rng(1)
    pts = random_points(rng, 64, spoiled=False)
    bias, radius, samples = 0.125, 3.0, 256
    rays = capi.debug_bake_rays(None, pts, samples, 7, bias, radius)
    d = np.stack([rays["direction"][q] for q in "xyz"], -1).astype(f64)
    o = np.stack([rays["origin"][q] for q in "xyz"], -1)
    n = pts[:, 4:7] / np.sqrt(((pts[:, 4] * pts[:, 4] + pts[:, 5] * pts[:, 5]) + pts[:, 6] * pts[:, 6]))[:, None]
    assert n.dtype == f32
    assert (np.einsum("psq,pq->ps", d.astype(f32), n) >= 0).all()                           # the hemisphere about the normal (binary32 dot, as a kernel would see it)
    assert np.abs(np.linalg.norm(d, axis=2) - 1).max() < 1e-5
    assert (o == (pts[:, 0:3] + n * f32(bias))[:, None, :]).all()                           # the origin offset, one origin per point
    assert (rays["origin"]["w"] == 0).all() and (rays["direction"]["w"] == f32(radius)).all()
    for p in range(len(pts)):
        assert len({r.tobytes() for r in rays[p]["direction"]}) == samples                  # rays of the same point differ
    assert len({rays[p]["direction"].tobytes() for p in range(len(pts))}) == len(pts)
    other = capi.debug_bake_rays(None, pts, samples, 8, bias, radius)
    assert (other["direction"]["x"] != rays["direction"]["x"]).mean() > 0.99                # two seeds give different rays
    same = np.tile(pts[:1], (8, 1))                                                         # the same point at another index: other rotations
    r8 = capi.debug_bake_rays(None, same, 16, 0, bias, radius)
    assert len({r8[p]["direction"].tobytes() for p in range(8)}) == 8
    assert capi.debug_bake_rays(None, same[3:], 16, 0, bias, radius, first_index=3).tobytes() == r8[3:].tobytes()    # first_index is the index of points[0]
    # cosine weighting: the mean of dot(direction, n) over the hemisphere is 2/3 (and 1/2 for a uniform one)
    cosines = np.einsum("psq,pq->ps", d, n.astype(f64))
    assert abs(cosines.mean() - 2.0 / 3.0) < 5e-3


# ---- 2. reduction

@pytest.mark.parametrize("samples", [16, 64, 256])
def test_reduce_equals_numpy_bit_for_bit(samples):
    rng = np.random.default_rng(50 + samples)
    n = 41
    pts = random_points(rng, n)
    rays = capi.debug_bake_rays(None, pts, samples, 3, 1e-3, 2.0)
    occ = (rng.uniform(size=(n, samples)) < rng.uniform(0, 1, (n, 1))).astype(u32) * rng.integers(1, 9, (n, samples)).astype(u32)     # any non-zero word: occluded
    occ[0] = 0; occ[2] = 1                                        # all free; all occluded: a zero sum, a zero bent normal
    got = capi.debug_bake_reduce(rays, occ, samples)
    want = np_reduce(rays, occ, samples)
    assert got.tobytes() == want.tobytes(), [k for k in T.bake_result.names if got[k].tobytes() != want[k].tobytes()]
    assert got["unoccluded"][0] == samples and got["unoccluded"][2] == 0 and not got["bent_normal"][2].any()
    skipped = np_rays(pts, samples)[1] == False                   # noqa: E712
    assert skipped.any() and (got["unoccluded"][skipped] == INVALID).all() and not got["bent_normal"][skipped].any()
    lens = np.linalg.norm(got["bent_normal"][~skipped & (got["unoccluded"] > 0)].astype(f64), axis=1)
    assert np.abs(lens - 1).max() < 1e-6


# ---- 3. conversions and refusals

def test_from_surfaces_conversion():
    rng = np.random.default_rng(9)
    n = 37
    s = np.zeros(n, T.surface)
    s["position"] = rng.normal(size=(n, 3)); s["shading_normal"] = rng.normal(size=(n, 3))
    s["geometric_normal"] = rng.normal(size=(n, 3)); s["t"] = 5; s["primitive_id"] = np.arange(n)
    s["flags"] = np.where(np.arange(n) % 3 == 0, 3, 1)             # every third meets its back face
    s["flags"][4] = 0; s["flags"][10] = 2                          # miss records (bit 0 clear), whatever else they hold
    s["shading_normal"][7] = np.nan                                # (a zero blend of a hit, as the guide pass's)
    rows = np.zeros((n, 8), f32)
    rows[:, 0:3] = s["position"]
    rows[:, 4:7] = np.where((s["flags"] & 2)[:, None] != 0, -s["shading_normal"], s["shading_normal"])
    rows[[4, 10], 4:7] = 0
    got = capi.debug_bake_rays(None, s, 64, 5, 0.01, 2.0, from_surfaces=True)
    assert got.tobytes() == capi.debug_bake_rays(None, rows, 64, 5, 0.01, 2.0).tobytes()
    assert got.tobytes() == np_rays(s, 64, 5, 0.01, 2.0, from_surfaces=True)[0].tobytes()
    for i in (4, 7, 10):
        assert not got[i].tobytes().strip(b"\0")
    flipped = np.stack([got["direction"][q] for q in "xyz"], -1)[0].astype(f64) @ s["shading_normal"][0].astype(f64)
    assert (flipped <= 1e-6).all() and s["flags"][0] == 3           # the hemisphere is about the flipped normal
    with pytest.raises(capi.RtError, match="types.surface"):
        capi.bake_points(rows, True)
    with pytest.raises(capi.RtError, match="float32\\[n, 8\\]"):
        capi.bake_points(np.zeros((3, 6), f32))


def test_record_layout_and_exports():
    assert T.bake_result.itemsize == 16 and {k: T.bake_result.fields[k][1] for k in T.bake_result.names} == dict(bent_normal=0, unoccluded=12)
    assert C.sizeof(capi.rt_bake_desc) == 20
    header = open(capi._HERE + "/../include/rt_hip.h").read()
    assert "RT_STATIC_ASSERT(sizeof(rt_bake_result) == 16" in header and "#define RT_BAKE_FROM_SURFACES 1u" in header
    for name in ("rt_scene_bake", "rt_scene_bake_buffer", "rt_debug_bake_rays", "rt_debug_bake_reduce"):
        assert name in capi.EXPORTS and hasattr(capi.load(), name)


def test_refusals_without_a_device():
    lib = capi.load()
    pts, out, rays = random_points(np.random.default_rng(0), 4), np.zeros(4, T.bake_result), np.zeros((4, 16), T.ray)
    occ = np.zeros((4, 16), u32)
    err = lambda: lib.rt_last_error(None).decode()
    p = lambda a: a.ctypes.data
    good = capi.bake_desc(16, 0, 1e-3, 1.0)
    assert lib.rt_scene_bake(None, p(pts), 4, C.byref(good), p(out)) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_bake(None, None, 0, None, None) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_bake_buffer(None, None, 4, C.byref(good), None) != 0 and "ctx is NULL" in err()
    bad = [(capi.bake_desc(0), "power of two"), (capi.bake_desc(8), "power of two"), (capi.bake_desc(48), "power of two"), (capi.bake_desc(8192), "power of two"),
           (capi.bake_desc(16, bias=np.nan), "bias"), (capi.bake_desc(16, bias=np.inf), "bias"), (capi.bake_desc(16, radius=0.0), "radius"),
           (capi.bake_desc(16, radius=-1.0), "radius"), (capi.bake_desc(16, radius=np.inf), "radius"), (capi.bake_desc(16, radius=np.nan), "radius"),
           (capi.bake_desc(16, flags=2), "unknown flag"), (capi.bake_desc(16, flags=0x80000001), "unknown flag")]
    for d, text in bad:
        assert lib.rt_debug_bake_rays(None, p(pts), 4, 0, C.byref(d), p(rays)) != 0 and text in err(), (text, err())
    for args in ((None, 4, 0, C.byref(good), p(rays)), (p(pts), 4, 0, None, p(rays)), (p(pts), 4, 0, C.byref(good), None)):
        assert lib.rt_debug_bake_rays(None, *args) != 0 and "NULL argument" in err()
    assert lib.rt_debug_bake_rays(None, p(pts), 1 << 20, 0, C.byref(capi.bake_desc(4096)), p(rays)) != 0 and "2^28" in err()
    assert lib.rt_debug_bake_rays(None, None, 0, 0, None, None) == 0                          # n == 0 does nothing
    assert lib.rt_debug_bake_reduce(None, p(occ), 4, 16, p(out)) != 0 and "NULL argument" in err()
    assert lib.rt_debug_bake_reduce(p(rays), p(occ), 4, 24, p(out)) != 0 and "power of two" in err()
    assert lib.rt_debug_bake_reduce(None, None, 0, 16, None) == 0
    assert out.tobytes() == bytes(out.nbytes) and rays.tobytes() == bytes(rays.nbytes)        # nothing was written
    with pytest.raises(capi.RtError, match="one verdict per ray"):
        capi.debug_bake_reduce(rays, occ[:3], 16)
    try:
        ctx = capi.Context(0)
    except capi.RtError as e:
        assert "no HIP device" in str(e)
        return
    try:
        with pytest.raises(capi.RtError, match="no scene uploaded"):
            ctx.bake(pts, 16)
    finally:
        ctx.close()


# ---- 4. the bakes of the GPU tests are not vacuous

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_non_vacuity(bake_cases, name):
    """With RADIUS_FRACTION and BIAS_FRACTION the oracle's verdicts leave at least a quarter of the walked points partially occluded, and at least half of the
    points are walked: tests/test_gpu_bake.py compares against these verdicts, and could pass on neither all-zero nor all-full counts."""
    case = bake_cases[name]
    n, samples = 257, 64
    pts = case.points(n, spoiled=False)
    want = case.expected(pts, samples)
    walked = want["unoccluded"] != INVALID
    partial = walked & (want["unoccluded"] > 0) & (want["unoccluded"] < samples)
    print(name, "walked", int(walked.sum()), "partially occluded", int(partial.sum()), "of", n)
    assert 2 * walked.sum() >= n, (int(walked.sum()), n)
    assert 4 * partial.sum() >= walked.sum(), (int(partial.sum()), int(walked.sum()))
    spoiled = case.expected(case.points(n), samples)                # the batches of the GPU tests: a third of the points spoiled on top of the misses
    assert 2 * (spoiled["unoccluded"] != INVALID).sum() >= n


def back_faced(surf):
    """a copy of surface records with every third hit marked as met from behind (flags bit 1).  The walk itself culls back faces, as the reference's
    ray-triangle test does (det < 1e-8 is no hit), so no traced record carries the bit: a caller sets it, for two-sided geometry of their own."""
    s = surf.copy()
    hits = np.flatnonzero((s["flags"] & 1) != 0)
    s["flags"][hits[::3]] |= 2
    return s


def test_mixed_rays_give_misses_and_hits(bake_cases):
    """The rays tests/test_gpu_bake.py::test_buffers_from_surfaces_and_chunks traces into surface records on the device: the oracle's first hits of them
    hold miss records and hits, none of them a back face (the walk culls those); a bake from them, and one from back_faced() of them, walks at least half
    of the points and leaves a quarter of those partially occluded, and the flip changes what is computed."""
    case = bake_cases["coverage"]
    n, samples = 257, 64
    rays = case.mixed_rays(n, 77)
    surf = capi.debug_query_surface(None, case.scene["triangles"], rays, case.orc.wide_trace(case.wide, case.entry, rays, False))
    miss = (surf["flags"] & 1) == 0
    print("miss", int(miss.sum()), "of", n)
    assert (surf["primitive_id"][miss] == INVALID).all() and (surf["primitive_id"][~miss] != INVALID).all()
    assert 8 * miss.sum() >= n and not (surf["flags"] & 2).any()
    results = []
    for s in (surf, back_faced(surf)):
        want = case.expected(s, samples, seed=3, from_surfaces=True)
        walked = want["unoccluded"] != INVALID
        partial = walked & (want["unoccluded"] > 0) & (want["unoccluded"] < samples)
        print("walked", int(walked.sum()), "partially occluded", int(partial.sum()))
        assert not walked[miss].any() and 2 * walked.sum() >= n and 4 * partial.sum() >= walked.sum()
        results.append(want)
    flipped = (back_faced(surf)["flags"] & 2) != 0
    assert 8 * flipped.sum() >= n
    assert (results[0]["bent_normal"][flipped] != results[1]["bent_normal"][flipped]).any(1).all()     # the other hemisphere: another bent normal, or none
    assert results[0][~flipped].tobytes() == results[1][~flipped].tobytes()
