"""Nearest-point queries (rt_scene_nearest, raytracing_amd/csrc/nearest.h) without a GPU.

The contract is a statement about the triangles alone: per point the smallest d2 <= max_distance^2 over all triangles, ties to the lowest index, with every
operand order fixed by nearest.h.  So (1) the header is compared with a numpy restatement in float32, operation by operation, byte for byte; (2) the bound that
prunes, box_d2 <= d2 in binary32 itself, is checked over random triples; (3) the kernel's walk on the host (rt_debug_nearest_walk, child-pair and 4-wide) equals
brute force byte for byte; (4) the walk prunes; (5) the distance is close to a float64 brute force; (6) refusals and record sizes."""
import ctypes as C
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_refit import positions

f32 = np.float32
INVALID = 0xFFFFFFFF
FOUND, BACK_SIDE, SHIFT = 1, 2, 2
FACE, EDGE, VERTEX = 0, 1, 2
CLASSES = 8           # a batch's point i is of class i % CLASSES (make_points)
NOT_SEARCHED = 6
# test 5: the largest |distance - d64| / max(|p|, |corners|) measured over test 3's inputs is 1.27e-7 (the Cornell box); the gate is four times it
ACCURACY_MEASURED = 1.27e-7


# ---- nearest.h in numpy: float32 arrays throughout, one rounding per operation, no contraction

def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def np_triangle(p, p1, p2, p3):
    """nearest_point_triangle over broadcastable [..., 3] arrays of one float type: (q clamped, d, d2, bu, bv, region)"""
    one, zero = p.dtype.type(1), p.dtype.type(0)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = p2 - p1, p3 - p1, p - p1, p - p2, p - p3
        d1, d2, d3, d4, d5, d6 = dot3(ab, ap), dot3(ac, ap), dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        s = (va + vb) + vc
        O, I = np.zeros_like(d1), np.ones_like(d1)
        bu = np.select(conds, [O, I, d1 / (d1 - d3), O, O, one - w], vb / s)
        bv = np.select(conds, [O, O, O, I, d2 / (d2 - d6), w], vc / s)
        region = np.select(conds, [VERTEX, VERTEX, EDGE, VERTEX, EDGE, EDGE], FACE).astype(np.uint32)
        w0 = one - bu - bv
        q = p1 * w0[..., None] + p2 * bu[..., None] + p3 * bv[..., None]
        lo = np.where(p2 < p1, p2, p1); lo = np.where(p3 < lo, p3, lo)
        hi = np.where(p2 > p1, p2, p1); hi = np.where(p3 > hi, p3, hi)
        q = np.where(q < lo, lo, q)
        q = np.where(q > hi, hi, q)
        d = p - q
        return q, d, dot3(d, d), bu, bv, region


def np_box_d2(p, lo, hi):
    with np.errstate(all="ignore"):
        g = lo - p
        t = p - hi
        g = np.where(t > g, t, g)
        g = np.where(g > 0, g, p.dtype.type(0))
        return dot3(g, g)


def np_nearest(P, pts, chunk=64):
    """rt_debug_nearest(NULL, ...) in numpy: P float32[nt, 3, 3], pts types.point[n]"""
    out = np.zeros(len(pts), T.nearest)
    out["primitive_id"] = INVALID
    pos, lim = pts["position"].astype(f32), pts["max_distance"].astype(f32)
    with np.errstate(all="ignore"):
        searched = np.isfinite(pos).all(1) & (lim >= 0)
        r2 = lim * lim
    for first in range(0, len(pts), chunk):
        sl = slice(first, first + chunk)
        p = pos[sl][:, None, :]
        q, d, d2, bu, bv, region = np_triangle(p, P[None, :, 0], P[None, :, 1], P[None, :, 2])
        valid = ~np.isnan(d2) & (d2 <= r2[sl][:, None]) & searched[sl][:, None]
        key = np.where(valid, d2, f32(np.inf))
        idx = np.argmin(key, axis=1)                      # the first of the smallest: the lowest index among ties
        rows = np.arange(len(idx))
        late = ~valid[rows, idx] & valid.any(1)           # every accepted d2 is +inf and an earlier triangle was not accepted
        idx[late] = np.argmax(valid[late], axis=1)
        found = valid[rows, idx]
        a, b = P[idx, 1] - P[idx, 0], P[idx, 2] - P[idx, 0]
        with np.errstate(all="ignore"):
            g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
            back = dot3(d[rows, idx], g) < 0
            dist = np.sqrt(d2[rows, idx])
        o = out[sl]
        o["position"][found] = q[rows, idx][found]
        o["distance"][found] = dist[found]
        o["bc"][found] = np.stack([bu[rows, idx], bv[rows, idx]], -1)[found]
        o["primitive_id"][found] = idx[found]
        o["flags"][found] = (FOUND | np.where(back, BACK_SIDE, 0) | (region[rows, idx] << SHIFT))[found]
        out[sl] = o
    return out


def triangles_of(P):
    """types.triangle with the corners P float32[nt, 3, 3] (normals and the rest zero: a nearest query reads the corners only)"""
    tris = np.zeros(len(P), T.triangle)
    for vi, v in enumerate(("v1", "v2", "v3")):
        for ci, c in enumerate("xyz"):
            tris[v]["position"][c] = P[:, vi, ci]
    return tris


def points_of(pos, lim=np.inf):
    pts = np.zeros(len(pos), T.point)
    pts["position"] = pos
    pts["max_distance"] = lim
    return pts


def same_records(got, want, what=""):
    assert got.tobytes() == want.tobytes(), (what, [k for k in T.nearest.names if got[k].tobytes() != want[k].tobytes()],
                                             np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(want))])[:8])


def blend(P, rng, n, on_edges=False):
    """n points on random triangles of P (float64 blends rounded to float32): (points, triangle indices)"""
    t = rng.integers(0, len(P), n)
    w = rng.dirichlet((1, 1, 1), n)
    if on_edges:
        w[np.arange(n), rng.integers(0, 3, n)] = 0.0
        w /= w.sum(1, keepdims=True)
    return (P[t].astype(np.float64) * w[:, :, None]).sum(1).astype(f32), t


# ---- 1. the header against numpy

def header_case():
    """random triangles and points with every special input of the contract: (P, points, index ranges by name)"""
    rng = np.random.default_rng(71)
    P = rng.uniform(-1, 1, (160, 3, 3)).astype(f32)
    P[100:110, 1] = P[100:110, 0]                                          # two equal corners
    P[110:115, 2] = P[110:115, 1]
    P[115:120, 1] = P[115:120, 0]; P[115:120, 2] = P[115:120, 0]           # three equal corners
    P[120:130, 2] = (P[120:130, 0] + (P[120:130, 1] - P[120:130, 0]) * f32(0.25)).astype(f32)      # collinear corners (up to rounding)
    P[130:135, 2] = P[130:135, 0] + (P[130:135, 1] - P[130:135, 0]) * f32(2.0)
    P[135:145] += f32(1e4)                                                 # offset by 1e4
    P[145:150] *= f32(3e19)                                                # squares overflow
    # quads whose corners and points are dyadic, so that the two triangles' d2 on the shared diagonal are computed exactly: ties
    quads = []
    for k in range(5):
        o = np.array([8.0 + 4 * k, -3.0, 2.0 + k])
        quads.append(S.quad(o, o + [4, 0, 0], o + [4, 4, 0], o + [0, 4, 0])[0])
    for k in range(5):
        c = rng.uniform(-1, 1, 3) + [30, 0, 0]
        e1, e2 = rng.normal(size=3), rng.normal(size=3)
        quads.append(S.quad(c, c + e1, c + e1 + e2, c + e2)[0])
    first_quad = len(P)
    P = np.concatenate([P] + quads).astype(f32)
    parts = {}

    def add(name, pos, lim=np.inf):
        parts[name] = points_of(np.asarray(pos, f32), lim)

    add("random", rng.uniform(-1.5, 1.5, (500, 3)))
    add("limited", rng.uniform(-1.5, 1.5, (300, 3)), rng.uniform(0.0, 0.3, 300).astype(f32))
    add("on_faces", blend(P[:100], rng, 200)[0])
    add("on_edges", blend(P[:100], rng, 200, on_edges=True)[0])
    add("on_vertices", P[rng.integers(0, 100, 100), rng.integers(0, 3, 100)])
    add("near_offset", blend(P[135:145], rng, 100)[0] + rng.normal(size=(100, 3)).astype(f32) * f32(1e-3))
    add("huge", rng.uniform(-1, 1, (60, 3)) * 3e19)
    add("zero_limit_on_vertex", P[rng.integers(0, 100, 20), 0], 0.0)
    diag = []
    for k in range(10):
        q = P[first_quad + 2 * k]                                              # (p0, p1, p2): the diagonal is p0 .. p2
        n = np.cross(q[1] - q[0], q[2] - q[0]).astype(np.float64)
        for t in (0.125, 0.25, 0.5, 0.625, 0.875):
            for h in (0.0, 0.5, -0.25, 1.0):
                diag.append(q[0] + (q[2] - q[0]) * t + (n / np.linalg.norm(n)) * h)
    add("on_diagonals", diag)
    names = list(parts)
    pts = np.concatenate([parts[k] for k in names])
    bad = np.zeros(8, T.point)
    bad["position"] = 0.25
    bad["max_distance"] = np.inf
    bad["position"][0, 0] = np.nan; bad["position"][1, 2] = np.inf; bad["position"][2, 1] = -np.inf
    bad["max_distance"][3] = np.nan; bad["max_distance"][4] = -1.0; bad["max_distance"][5] = -np.inf; bad["max_distance"][6] = -1e-30
    bad = bad[:7]
    return P, np.concatenate([pts, bad]), len(pts), first_quad


def test_header_equals_numpy_restatement_byte_for_byte():
    P, pts, n_good, first_quad = header_case()
    tris = triangles_of(P)
    got = capi.debug_nearest(None, tris, pts)
    want = np_nearest(P, pts)
    same_records(got, want, "nearest.h against numpy")
    # non-vacuity
    found = got["primitive_id"] != INVALID
    regions = (got["flags"][found] >> SHIFT) & 3
    assert all((regions == r).sum() >= 20 for r in (FACE, EDGE, VERTEX)), np.bincount(regions)
    assert found.sum() >= 100 and (~found[:n_good]).sum() >= 50                    # some points are found and some are not (the limited ones)
    assert not found[n_good:].any()                                                # not searched
    none = np.zeros(1, T.nearest); none["primitive_id"] = INVALID
    assert all(got[i].tobytes() == none[0].tobytes() for i in np.flatnonzero(~found))       # nothing found / not searched: the id and zeros
    assert (got["flags"][found] & BACK_SIDE).any() and not (got["flags"][found] & BACK_SIDE).all()
    assert (got["distance"][found] == 0).any()                                    # points exactly on the surface
    # an exact tie in d2 between two triangles goes to the lower id
    pos = pts["position"][:n_good]
    with np.errstate(all="ignore"):
        d2 = np_triangle(pos[:, None, :], P[None, :, 0], P[None, :, 1], P[None, :, 2])[2]
    best = got["primitive_id"][:n_good]
    ok = best != INVALID
    rows = np.flatnonzero(ok)
    tie = (d2[rows] == d2[rows, best[rows]][:, None]).sum(1) >= 2
    assert tie.sum() >= 10, "no exact tie in d2 among the points on the quads' diagonals"
    for r in rows[tie]:
        assert best[r] == np.flatnonzero(d2[r] == d2[r, best[r]])[0]
    assert (best[rows[tie]] >= first_quad).any()                                   # (ties on the shared diagonals are among them)


# ---- 2. the bound

def test_box_bound_never_exceeds_the_distance():
    rng = np.random.default_rng(72)
    n = 120_000
    scale = np.exp2(rng.integers(-8, 12, n)).astype(f32)[:, None, None]
    P = (rng.uniform(-1, 1, (n, 3, 3)) * scale + rng.uniform(-1, 1, (n, 1, 3)) * scale * 4).astype(f32)
    P[: n // 20, 1] = P[: n // 20, 0]                                           # degenerate ones too
    lo, hi = P.min(1), P.max(1)
    kind = np.arange(n) % 3
    grow = (rng.uniform(0, 1, (n, 3)) * scale[:, 0] * rng.choice([1e-6, 1e-2, 1.0], (n, 1))).astype(f32)
    lo = np.where((kind == 1)[:, None], lo - grow, lo).astype(f32)
    hi = np.where((kind == 1)[:, None], hi + grow, hi).astype(f32)
    # a power-of-two grid as wide_quantise makes it: planes origin + k * cell, rounded outward
    cell = np.exp2(np.ceil(np.log2((hi - lo).max(1) / 200 + 1e-30)) + rng.integers(0, 4, n))[:, None]
    glo = (np.floor(lo.astype(np.float64) / cell) * cell).astype(f32)
    ghi = (np.ceil(hi.astype(np.float64) / cell) * cell).astype(f32)
    exact = (glo <= lo).all(1) & (ghi >= hi).all(1)                             # (the grid points are exact in binary32 at these magnitudes)
    assert exact.all()
    lo = np.where((kind == 2)[:, None], glo, lo)
    hi = np.where((kind == 2)[:, None], ghi, hi)
    where = np.arange(n) // 3 % 5
    u = rng.uniform(0, 1, (n, 3))
    inside = (lo + (hi - lo) * u).astype(f32)
    on_face = inside.copy()
    ax = rng.integers(0, 3, n)
    on_face[np.arange(n), ax] = np.where((rng.integers(0, 2, n) == 1)[:, None], hi, lo)[np.arange(n), ax]
    near = (inside + rng.normal(size=(n, 3)) * (hi - lo).max(1, keepdims=True) * 2).astype(f32)
    far = rng.normal(size=(n, 3)); far = (far / np.linalg.norm(far, axis=1, keepdims=True) * 2.0 ** 30).astype(f32)
    huge = (rng.normal(size=(n, 3)) * 1e25).astype(f32)                         # gaps whose squares overflow
    p = np.select([(where == k)[:, None] for k in range(4)], [inside, on_face, near, far], huge).astype(f32)
    with np.errstate(all="ignore"):
        d2 = np_triangle(p, P[:, 0], P[:, 1], P[:, 2])[2]
        b2 = np_box_d2(p, lo, hi)
    ok = ~np.isnan(d2)
    assert ok.sum() > 0.9 * n and not np.isnan(b2).any()
    assert (b2[ok] <= d2[ok]).all(), int((b2[ok] > d2[ok]).sum())
    assert (b2[where == 0] == 0).all() and (b2[where == 3] > 0).all() and np.isinf(b2[where == 4]).any()
    assert ((b2 == d2) & (b2 > 0)).any()                                        # the bound is attained: a strict comparison is what the tie rule needs


# ---- 3. the walk equals brute force

@pytest.fixture(scope="module")
def city():
    """S.city_block(40_000) as tests/test_gpu_pose.py's `city` fixture builds it"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = host.Scene(arrays=S.city_block(40_000))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.set_env_path(os.path.join(root, "assets", "ibl", "CGSkies_0036_free.hdr"))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}


def make_points(tris, n, seed):
    """the mixed batch: class of point i = i % 8 -- 0 uniform inside the bounds; 1 on a surface (a blend of a random triangle's corners); 2 a bounds' diagonal
    outside; 3 2^30 away; 4 / 5 inside, max_distance at half / at twice the brute-force distance; 6 not searched (NaN, Inf, negative and NaN max_distance);
    7 a surface point pushed off by a thousandth of the diagonal"""
    rng = np.random.default_rng(seed)
    P = positions(tris)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    centre, diagonal = ((lo + hi) / 2).astype(f32), float(np.linalg.norm(hi - lo))
    cls = np.arange(n) % CLASSES
    inside = (lo[None] + rng.uniform(0.02, 0.98, (n, 3)) * (hi - lo)[None]).astype(f32)
    rnd = rng.normal(size=(n, 3)); rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    surface = blend(P, rng, n)[0]
    pos = inside.copy()
    pos[cls == 1] = surface[cls == 1]
    pos[cls == 2] = (centre[None] + rnd * diagonal * 1.5).astype(f32)[cls == 2]
    pos[cls == 3] = (centre[None] + rnd * 2.0 ** 30).astype(f32)[cls == 3]
    pos[cls == 7] = (surface + rnd * diagonal * 1e-3).astype(f32)[cls == 7]
    pts = points_of(pos)
    lim = (cls == 4) | (cls == 5)
    if lim.any():
        d = capi.debug_nearest(None, tris, pts[lim])["distance"]
        pts["max_distance"][lim] = np.where(cls[lim] == 4, d * f32(0.5), d * f32(2.0)).astype(f32)
    for k, i in enumerate(np.flatnonzero(cls == NOT_SEARCHED)):
        kind = k % 4
        if kind == 0: pts["position"][i, 1] = np.nan
        elif kind == 1: pts["position"][i, 0] = np.inf
        elif kind == 2: pts["max_distance"][i] = -1.0
        else: pts["max_distance"][i] = np.nan
    return pts


class Case:
    """a scene, its batches and their brute-force answers (computed once, shared, never changed)"""

    def __init__(self, name, scene):
        self.name, self.scene = name, scene
        self.batches = {}

    def batch(self, n):
        if n not in self.batches:
            pts = make_points(self.scene["triangles"], n, 2000 + n)
            want = capi.debug_nearest(None, self.scene["triangles"], pts)
            want.setflags(write=False)
            self.batches[n] = (pts, want)
        return self.batches[n]


def check_batch(pts, want):
    """what the classes promise of a batch's brute-force answer (non-vacuity of everything compared with it)"""
    cls = np.arange(len(pts)) % CLASSES
    found = want["primitive_id"] != INVALID
    assert found[np.isin(cls, (0, 1, 2, 3, 5, 7))].all()
    assert not found[cls == NOT_SEARCHED].any()
    half = cls == 4
    assert (~found[half] | (want["distance"][half] == 0)).all()                 # half the distance finds nothing (unless the point lies on the surface)
    if len(pts) >= 64:
        assert (want["distance"][cls == 1] <= want["distance"][cls == 0].max()).all() and (~found[half]).any()


@pytest.fixture(scope="module")
def cases(golden_scenes, city):
    return {"cornell": Case("cornell", golden_scenes["cornell"]), "coverage": Case("coverage", golden_scenes["coverage"]), "city": Case("city", city)}


@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_walk_equals_brute_force_byte_for_byte(cases, name):
    case = cases[name]
    for n in (1, 65, 1031):
        pts, want = case.batch(n)
        check_batch(pts, want)
        for wide in (False, True):
            same_records(capi.debug_nearest_walk(case.scene["nodes"], case.scene["triangles"], pts, wide=wide), want, (name, n, wide))
    # float rows: the same rule (three columns = no limit)
    pts, want = case.batch(65)
    rows = np.concatenate([pts["position"], pts["max_distance"][:, None]], 1)
    same_records(capi.debug_nearest_walk(case.scene["nodes"], case.scene["triangles"], rows), want)
    unlimited = capi.debug_nearest(None, case.scene["triangles"], rows[:, :3])
    assert unlimited.tobytes() == capi.debug_nearest(None, case.scene["triangles"], points_of(rows[:, :3])).tobytes()


# ---- 4. the walk prunes

def test_walk_prunes(cases):
    case = cases["city"]
    pts, want = case.batch(1031)
    inside = pts[np.arange(len(pts)) % CLASSES == 0]
    nt = len(case.scene["triangles"])
    for wide in (False, True):
        got, tested = capi.debug_nearest_walk(case.scene["nodes"], case.scene["triangles"], inside, wide=wide, counts=True)
        share = tested.sum() / (len(inside) * nt)
        print("share of point x triangle pairs tested, wide =", wide, ":", share)
        assert 0 < tested.min() and share < 0.5, share
    _, none = capi.debug_nearest_walk(case.scene["nodes"], case.scene["triangles"], pts[np.arange(len(pts)) % CLASSES == NOT_SEARCHED], counts=True)
    assert not none.any()                                                       # a point that is not searched is not walked


# ---- 5. accuracy sanity

def np_distance64(P, pos, chunk=16):
    """float64 brute force with the same region logic: the distance to the nearest triangle"""
    P64 = P.astype(np.float64)
    out = np.zeros(len(pos))
    for first in range(0, len(pos), chunk):
        p = pos[first:first + chunk].astype(np.float64)[:, None, :]
        d2 = np_triangle(p, P64[None, :, 0], P64[None, :, 1], P64[None, :, 2])[2]
        out[first:first + chunk] = np.sqrt(np.nanmin(d2, axis=1))
    return out


@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_distance_is_close_to_float64(cases, name):
    case = cases[name]
    pts, want = case.batch(1031)
    cls = np.arange(len(pts)) % CLASSES
    pick = np.flatnonzero(np.isin(cls, (0, 1, 2, 3, 7)))                        # no limit: the answer is the nearest triangle
    if name == "city":
        pick = pick[:160]
    P = positions(case.scene["triangles"])
    d64 = np_distance64(P, pts["position"][pick])
    magnitude = np.maximum(np.abs(pts["position"][pick]).max(1), np.abs(P).max())
    err = np.abs(want["distance"][pick].astype(np.float64) - d64) / magnitude
    print("largest |distance - d64| / max(|p|, |corners|):", name, err.max())
    assert err.max() <= 4 * ACCURACY_MEASURED, err.max()


# ---- 6. refusals and record sizes

def test_refusals_and_record_sizes(golden_scenes):
    assert T.point.itemsize == 16 and T.nearest.itemsize == 32
    lib = capi.load()
    sc = golden_scenes["cornell"]
    tris, nodes = np.ascontiguousarray(sc["triangles"]), np.ascontiguousarray(sc["nodes"])
    pts, out = points_of(np.zeros((4, 3), f32)), np.zeros(4, T.nearest)
    surf = np.zeros(4, T.surface)
    p = lambda a: a.ctypes.data

    def refused(rc, text):
        assert rc != 0 and text in lib.rt_last_error(None).decode(), (rc, lib.rt_last_error(None).decode())

    refused(lib.rt_scene_nearest(None, p(pts), 4, p(out), None), "ctx is NULL")
    refused(lib.rt_scene_nearest_buffer(None, None, 4, None, None), "ctx is NULL")
    refused(lib.rt_scene_nearest(None, None, 0, None, None), "ctx is NULL")
    refused(lib.rt_debug_nearest(None, p(tris), len(tris), None, 4, p(out)), "NULL argument")
    refused(lib.rt_debug_nearest(None, p(tris), len(tris), p(pts), 4, None), "NULL argument")
    refused(lib.rt_debug_nearest(None, None, len(tris), p(pts), 4, p(out)), "NULL argument")
    refused(lib.rt_debug_nearest_walk(None, len(nodes), p(tris), len(tris), 1, p(pts), 4, p(out), None), "NULL argument")
    refused(lib.rt_debug_nearest_walk(p(nodes), len(nodes), p(tris), len(tris), 2, p(pts), 4, p(out), None), "wide must be")
    refused(lib.rt_debug_nearest_walk(p(nodes), len(nodes), p(tris), len(tris) - 1, 0, p(pts), 4, p(out), None), "outside the array")
    assert out.tobytes() == bytes(out.nbytes) and surf.tobytes() == bytes(surf.nbytes)       # nothing was written by any of them
    assert lib.rt_debug_nearest(None, None, 0, None, 0, None) == 0                         # n == 0: RT_OK, nothing done
    assert lib.rt_debug_nearest_walk(p(nodes), len(nodes), p(tris), len(tris), 1, None, 0, None, None) == 0
    none = capi.debug_nearest(None, tris[:0], pts)                                         # no triangles: nothing found
    assert (none["primitive_id"] == INVALID).all() and not none["flags"].any()
    with pytest.raises(capi.RtError, match="points must be"):
        capi.point_records(np.zeros((3, 5), f32))
    assert np.isinf(capi.point_records(np.zeros((3, 3), f32))["max_distance"]).all()
