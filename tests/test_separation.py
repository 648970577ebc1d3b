"""Separation queries (rt_scene_separation / rt_scene_separation_self, raytracing_amd/csrc/separation.h) without a GPU.

The contract is a statement about the triangles alone: SEP(Q, T) is 0 where the two cross (cross.h's verdict), else the least of fifteen candidates -- three
probe corners against T, three corners of T against the probe, nine edge pairs -- and a probe's answer is the triangle with the least SEP within
max_distance, the lowest id among equal ones.  So (1) on small-integer coordinates the header's distance equals exact rational arithmetic within a derived
bound and its CROSSING flag equals the exact verdict; (2) the header (rt_debug_separation's host brute force) is compared with a numpy restatement with the
same operand order, byte for byte; (3) the bound that prunes never exceeds the distance, for every kind of box a walk meets; (4) the kernel's walk on the
host (rt_debug_separation_walk, child-pair and 4-wide) equals the brute force on the scenes and on the tree corpus; (5) the self form skips neighbours
and, on request, pairs of one object."""
import random
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_nearest import INVALID, city, triangles_of, np_triangle, dot3          # noqa: F401 (fixtures)
from tests.test_refit import positions
from tests.test_within import STACK_CHAINS, corpus_triangles
from tests.test_region import rotation
from tests.test_cross import np_pair, corners_of, exact_pairs, tetra_pair
from tests.test_wide_bvh import wide_of, LEAF, EMPTY

f32 = np.float32
INF = float("inf")
SEARCHED, FOUND, CROSSING = 1, 2, 4
FEATURE_CROSSING = 15


# ---- separation.h in numpy (binary32, every operation rounded once, separation.h's operand order)

def _clamp01(x):
    x = np.where(x < 0, f32(0), x)
    return np.where(x > 1, f32(1), x)


def np_segments(a1, b1, a2, b2):
    """sep_segments over broadcastable float32[..., 3]: (d2, c1, c2)"""
    with np.errstate(all="ignore"):
        d1, d2, r = b1 - a1, b2 - a2, a1 - a2
        a, e, f, c, b = dot3(d1, d1), dot3(d2, d2), dot3(d2, r), dot3(d1, r), dot3(d1, d2)
        denom = a * e - b * b
        s = np.where((denom > 0) | (denom < 0), _clamp01((b * f - c * e) / denom), f32(0))
        t = (b * s + f) / e
        s = np.where(t < 0, _clamp01(-c / a), np.where(t > 1, _clamp01((b - c) / a), s))
        t = np.where(t < 0, f32(0), np.where(t > 1, f32(1), t))
        s = np.where(e == 0, _clamp01(-c / a), s); t = np.where(e == 0, f32(0), t)
        s = np.where(a == 0, f32(0), s); t = np.where(a == 0, np.where(e == 0, f32(0), _clamp01(f / e)), t)
        x, y = a1 + s[..., None] * d1, a2 + t[..., None] * d2
        lo1, hi1, lo2, hi2 = np.where(b1 < a1, b1, a1), np.where(b1 > a1, b1, a1), np.where(b2 < a2, b2, a2), np.where(b2 > a2, b2, a2)
        x = np.where(x < lo1, lo1, x); x = np.where(x > hi1, hi1, x)
        y = np.where(y < lo2, lo2, y); y = np.where(y > hi2, hi2, y)
        d = x - y
        return dot3(d, d), x, y


def np_candidates(Q, P):
    """the fifteen candidates of broadcastable corner arrays Q, P float32[..., 3, 3] (no crossing step): (d2, on_probe, on_scene, feature), a NaN never wins"""
    Q, P = np.broadcast_arrays(Q.astype(f32), P.astype(f32))
    shape = Q.shape[:-2]
    best = np.full(shape, np.nan, f32)
    A, B = np.zeros(shape + (3,), f32), np.zeros(shape + (3,), f32)
    feature = np.zeros(shape, np.uint32)
    have = np.zeros(shape, bool)

    def offer(d2, a, b, k):
        nonlocal best, A, B, feature, have
        with np.errstate(all="ignore"):
            wins = np.where(have, d2 < best, ~np.isnan(d2))
        best = np.where(wins, d2, best)
        A, B = np.where(wins[..., None], a, A), np.where(wins[..., None], b, B)
        feature = np.where(wins, np.uint32(k), feature)
        have = have | wins

    for k in range(3):
        q, _, d2, _, _, _ = np_triangle(Q[..., k, :], P[..., 0, :], P[..., 1, :], P[..., 2, :])
        offer(d2, Q[..., k, :], q, k)
    for k in range(3):
        q, _, d2, _, _, _ = np_triangle(P[..., k, :], Q[..., 0, :], Q[..., 1, :], Q[..., 2, :])
        offer(d2, q, P[..., k, :], 3 + k)
    for i in range(3):
        for j in range(3):
            d2, c1, c2 = np_segments(Q[..., i, :], Q[..., (i + 1) % 3, :], P[..., j, :], P[..., (j + 1) % 3, :])
            offer(d2, c1, c2, 6 + 3 * i + j)
    return best, A, B, feature


def np_box_gap2(qlo, qhi, lo, hi):
    """sep_box_d2"""
    with np.errstate(all="ignore"):
        g, t = lo - qhi, qlo - hi
        g = np.where(t > g, t, g)
        g = np.where(g > 0, g, f32(0))
        return dot3(g, g)


def np_separation(P, probes, max_distance=INF, self_first=None, ids=None):
    """rt_debug_separation(NULL, ...) (self_first None) or rt_debug_separation_self(NULL, ...) in numpy: P float32[nt, 3, 3] -> types.separation[n]"""
    C = corners_of(probes).astype(f32) if self_first is None else P[self_first:self_first + len(probes)]
    out = np.zeros(len(C), T.separation)
    out["primitive_id"] = INVALID
    lim = f32(max_distance)
    with np.errstate(all="ignore"):
        r2 = lim * lim
    for i, q in enumerate(C):
        if not (np.isfinite(q).all() and lim >= 0):
            continue
        out["flags"][i] = SEARCHED
        flags, c0, _ = np_pair(q, P)
        d2, A, B, feature = np_candidates(q[None], P)
        cross = flags != 0
        d2 = np.where(cross, f32(0), d2)
        with np.errstate(all="ignore"):
            valid = ~np.isnan(d2) & (d2 <= r2)
        if self_first is not None:
            shared = (q[:, None, None, :] == P[None, :, :, :]).all(-1).any(0).any(-1)
            valid &= ~shared
            valid[self_first + i] = False
            if ids is not None:
                valid &= ids != ids[self_first + i]
        if not valid.any():
            continue
        t = int(np.argmin(np.where(valid, d2, f32(np.inf))))
        if not valid[t]:
            t = int(np.argmax(valid))                                    # every accepted d2 is +inf: the first accepted one
        with np.errstate(all="ignore"):
            out[i] = (c0[t] if cross[t] else A[t], np.sqrt(d2[t]), c0[t] if cross[t] else B[t], t, SEARCHED | FOUND | (CROSSING if cross[t] else 0),
                      FEATURE_CROSSING if cross[t] else feature[t], (0, 0))
    return out


def same(got, want, what=""):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, [k for k in T.separation.names if got[k].tobytes() != want[k].tobytes()],
                                                                        np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])


# ---- 1. exact arithmetic on small integers

def _idot(a, b):
    return (a * b).sum(-1)


def _point_segment(p, a, b):
    """exact squared distance of integer points p to segments a b, as a float64 quotient of two exact integers"""
    ab, ap = b - a, p - a
    L, u = _idot(ab, ab), _idot(ap, ab)
    inner = (L > 0) & (u > 0) & (u < L)
    num = np.where(inner, _idot(ap, ap) * L - u * u, np.where((L > 0) & (u >= L), _idot(p - b, p - b), _idot(ap, ap)))
    return num / np.where(inner, L, 1)


def _point_face(p, a, b, c):
    """the same to the triangle's interior where the projection falls inside it (+inf elsewhere: the edges answer there)"""
    n = np.cross(b - a, c - a)
    nn = _idot(n, n)
    inside = (nn > 0) & (_idot(np.cross(b - a, p - a), n) >= 0) & (_idot(np.cross(c - b, p - b), n) >= 0) & (_idot(np.cross(a - c, p - c), n) >= 0)
    return np.where(inside, _idot(n, p - a) ** 2 / np.where(nn > 0, nn, 1), np.inf)


def _line_line(a1, b1, a2, b2):
    """the same between two segments where the closest points of their LINES fall inside both (+inf elsewhere: the end points answer there)"""
    d1, d2, r = b1 - a1, b2 - a2, a1 - a2
    a, e, f, c, b = _idot(d1, d1), _idot(d2, d2), _idot(d2, r), _idot(d1, r), _idot(d1, d2)
    denom = a * e - b * b
    sn, tn = b * f - c * e, a * f - b * c
    inside = (denom > 0) & (sn >= 0) & (sn <= denom) & (tn >= 0) & (tn <= denom)
    n = np.cross(d1, d2)
    return np.where(inside, _idot(n, r) ** 2 / np.where(denom > 0, denom, 1), np.inf)


def exact_d2(Q, P):
    """the exact squared distance of the triangle pairs (Q[i], P[i]), int64[n, 3, 3], that do not intersect: every term is a quotient of two exact integers
    below 2^53, formed in int64 and divided once in binary64 (relative error 2^-53).  The minimum over the six point-face terms, the nine line-line terms
    and the eighteen corner-edge terms is the minimum over the issue's six point-triangle and nine segment-segment distances: each of those is one of these."""
    terms = []
    for X, Y in ((Q, P), (P, Q)):
        for k in range(3):
            terms.append(_point_face(X[:, k], Y[:, 0], Y[:, 1], Y[:, 2]))
            for j in range(3):
                terms.append(_point_segment(X[:, k], Y[:, j], Y[:, (j + 1) % 3]))
    for i in range(3):
        for j in range(3):
            terms.append(_line_line(Q[:, i], Q[:, (i + 1) % 3], P[:, j], P[:, (j + 1) % 3]))
    return np.min(terms, axis=0)


# the derived bound of test_exact_fixture_distance_and_verdict (see its docstring)
EXACT_BOUND = 1222 * 2.0 ** -24


def test_exact_fixture_distance_and_verdict():
    """20 000 pairs with integer corners, |coordinate| <= 16 (tests/test_cross.py's exact fixture).  The header's distance against sqrt of the exact squared
    distance (0 where the exact crossing test accepts), within EXACT_BOUND = 1222 * 2^-24 (2^-13.75) absolute.  The derivation, u = 2^-24, for this coordinate range:
      * edge vectors have components <= 32 and length <= 32 sqrt 3 < 55.5; differences of points <= 64 per component, distances < 111; every dot product
        of two edge or difference vectors is an integer below 2^24: exact.  Products of two of them (a e, b b, b f, c e, d1 d4, ...) are below 2^24 too;
        only their sums and differences may exceed 2^24 and round once (relative u).  So every branch of nearest_point_triangle is decided exactly (signs and
        zeros survive one rounding), and sep_segments' denominator is zero exactly when the edges are parallel.
      * moving a witness point by delta inside its (convex) triangle changes the distance between the two witnesses by at most delta, and the true minimum is
        attained at exact witnesses; so the error is at most the sum of the witnesses' displacements plus the rounding of d = c1 - c2, dot3 and sqrtf.
      * an edge pair: s = clamp(num / denom) carries 3 u (numerator's difference, the quotient, s <= 1): the probe's witness moves by <= 55.5 * 3 u.
        t = (b s + f) / e: |d2| dt <= |d1| (ds + 2 u) + |d2| 2 u <= 55.5 * 7 u (b / |d2| <= |d1|; the product, the sum, the quotient).  A t within 7 u of 0 or 1
        may take the other branch; both branches are continuous there, so the same budget covers it.  Subtotal <= 55.5 * 10 u = 555 u.
      * a corner against a triangle: bu = vb / s carries 5 u (vb, va + vb + vc without cancellation in the face region, the quotient), w0 = 1 - bu - bv 12 u,
        the witness p1 w0 + p2 bu + p3 bv with |p| <= 16 moves by <= 16 (12 + 5 + 5) u + 5 * 16 u = 432 u per component, <= 749 u in norm.  (This is the
        larger of the two subtotals.)
      * c = a + s d per component: <= (32 + 48) u for each of the two witnesses (clamping into the segment's box only moves it towards the exact point):
        <= 2 * 80 sqrt 3 u < 278 u for an edge pair, so 555 + 278 = 833 u there.
      * d = c1 - c2: <= 64 u per component, 111 u in norm; dot3 and sqrtf: relative 2.5 u of a distance < 111: 278 u.
      total <= 833 + 111 + 278 = 1222 u = 2^-13.75, which is what is asserted.
    The issue's own estimate was 2^-14 (about 1000 u); the corner-triangle witness and the final dot3 / sqrtf terms it left out account for the difference.
    RT_SEPARATION_CROSSING must equal the exact verdict on every strict pair (no determinant and no barycentric exactly 0 in the six segment tests)."""
    random.seed(1)
    n = 20000
    C = np.array([random.randint(-16, 16) for _ in range(n * 18)], np.int64).reshape(n, 2, 3, 3)
    cross_flags, strict = exact_pairs(C[:, 0], C[:, 1])
    crossing = cross_flags != 0
    want = np.sqrt(np.where(crossing, 0.0, exact_d2(C[:, 0], C[:, 1])))
    assert (~crossing).mean() > 0.5 and (want[~crossing] > 0).mean() > 0.9
    lib = capi.load()
    probes = T.probes_from_corners(C[:, 0])
    tris = np.ascontiguousarray(triangles_of(C[:, 1].astype(f32)))
    out = np.zeros(n, T.separation)
    pp, tp, op = probes.ctypes.data, tris.ctypes.data, out.ctypes.data
    for i in range(n):                                               # pair i on its own: one probe against one triangle
        assert lib.rt_debug_separation(None, tp + 160 * i, 1, pp + 48 * i, 1, INF, op + 48 * i) == 0
    assert (out["flags"] & (SEARCHED | FOUND) == SEARCHED | FOUND).all() and (out["primitive_id"] == 0).all()
    err = np.abs(out["distance"].astype(np.float64) - want)
    print("largest error %.3g = %.1f u; crossing %.2f %%; features %s" % (err.max(), err.max() * 2 ** 24, 100 * crossing.mean(), np.bincount(out["feature"], minlength=16)))
    assert err.max() <= EXACT_BOUND, (err.max(), int(err.argmax()))
    got_cross = (out["flags"] & CROSSING) != 0
    assert np.array_equal(got_cross[strict], crossing[strict])
    assert np.array_equal(got_cross, out["feature"] == FEATURE_CROSSING) and (out["distance"][got_cross] == 0).all()
    # the witnesses are the distance apart (to rounding) and lie on their triangles' boxes
    gap = np.linalg.norm(out["on_probe"].astype(np.float64) - out["on_scene"], axis=1)
    assert np.abs(gap - out["distance"]).max() <= 2.0 ** -18
    for name, X in (("on_probe", C[:, 0]), ("on_scene", C[:, 1])):
        ok = ~got_cross
        assert ((out[name][ok] >= X[ok].min(1)) & (out[name][ok] <= X[ok].max(1))).all()
    assert all((out["feature"] == k).any() for k in range(16))


# ---- 2. the header against numpy on the scenes

def coplanar_pairs(P):
    """pairs (t, u) of triangles that share two corners and lie in one axis-aligned plane -- the two halves of a wall or a box's face: [(t, u, axis)]"""
    found = []
    flat = [(a, np.flatnonzero((P[:, :, a] == P[:, :1, a]).all(1))) for a in range(3)]
    for a, idx in flat:
        keys = {}
        for t in idx[:4000]:
            for i in range(3):
                e = tuple(sorted((tuple(P[t, i]), tuple(P[t, (i + 1) % 3]))))
                keys.setdefault((float(P[t, 0, a]), e), []).append(int(t))
        found += [(v[0], v[1], a) for v in keys.values() if len(v) == 2]
    return found


def make_probes(tris, n, seed):
    """the mixed batch.  By index % 13: 0..3 a scene triangle turned and moved a little (most cross something); 4..8 the same shrunk and pushed off its
    surface (apart from the scene: a corner, an edge or the face is nearest); 9 a probe with a NaN, 10 one with an inf (not searched), 11 a zero-area probe
    (three points on a line), 12 coordinates near FLT_MAX (squares overflow).  Probe 0 spans the whole scene; probe 1 lies parallel to a wall above the
    shared diagonal of its two triangles, exactly as far from both; probe 2 is a scene triangle's own corners moved off along an axis (a corner of the
    scene nearest the probe's face is likely among 3..8)."""
    rng = np.random.default_rng(seed)
    P = positions(tris).astype(np.float64)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    diag = float(np.linalg.norm(hi - lo))
    C = np.zeros((n, 3, 3))
    for i in range(n):
        t = P[rng.integers(0, len(P))]
        c = t.mean(0)
        size = max(float(np.abs(t - c).max()), 1e-3 * diag)
        scale = rng.uniform(0.5, 2.0) * min(1.0, 0.15 * diag / size)
        k = i % 13
        if 4 <= k <= 8:
            nrm = np.cross(t[1] - t[0], t[2] - t[0])
            nrm = nrm / (np.linalg.norm(nrm) + 1e-300)
            big = rng.uniform(1.0, 6.0) if k >= 7 else rng.uniform(0.05, 0.3)        # 7, 8: larger than the triangle below it: its corners are nearest
            C[i] = (t - c) @ rotation(rng.normal(size=3), rng.uniform(0.0, 0.6)).T * big + c + nrm * rng.uniform(0.01, 0.05) * diag * (1 + 3 * (k >= 7))
        else:
            C[i] = (t - c) @ rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)).T * scale + c + rng.normal(size=3) * 0.02 * diag
        if k == 11:
            C[i, 2] = (C[i, 0] + C[i, 1]) / 2
        elif k == 12:
            C[i] *= 3.0e38 / np.abs(C[i]).max() * rng.uniform(0.3, 1.0)
    u, v, m = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0), (lo + hi) / 2
    C[0] = [m + 4 * diag * u, m - 2 * diag * u + 3.6 * diag * v, m - 2 * diag * u - 3.6 * diag * v]
    probes = T.probes_from_corners(C)
    for i in range(n):
        if i % 13 == 9:
            probes[("p1", "p2", "p3")[i % 3]][i, rng.integers(0, 3)] = np.nan
        elif i % 13 == 10:
            probes[("p1", "p2", "p3")[i % 3]][i, rng.integers(0, 3)] = np.inf if i % 2 else -np.inf
    for name in ("p1", "p2", "p3"):
        probes[name][:, 3] = rng.normal(size=n)                      # ignored
    return probes


def equidistant_probe(tris):
    """(probe corners float32[3, 3], t, u): a small triangle parallel to an axis-aligned wall, centred above the middle of the diagonal its two triangles t < u
    share, at a height that is exact in binary32 -- the same distance from both, to the bit -- chosen among the scene's walls so that nothing else is nearer"""
    P = positions(tris).astype(f32)
    for t, u, a in coplanar_pairs(P):
        shared = [c for c in map(tuple, P[t]) if c in set(map(tuple, P[u]))]
        mid = (np.array(shared[0], np.float64) + np.array(shared[1], np.float64)) / 2
        edge = float(np.linalg.norm(np.array(shared[0], np.float64) - shared[1]))
        if edge == 0:
            continue
        for sign in (1.0, -1.0):
            h = sign * float(f32(2.0 ** np.floor(np.log2(edge / 64))))
            q = np.repeat(mid[None], 3, 0)
            b, c = (a + 1) % 3, (a + 2) % 3
            r = abs(h) / 4
            q[:, a] += h
            q[0, b] += r; q[1, b] -= r; q[2, c] += r
            q = q.astype(f32)
            both = capi.debug_separation(None, tris[[t, u]], q[None])
            each = [capi.debug_separation(None, tris[[k]], q[None])[0] for k in (t, u)]
            whole = capi.debug_separation(None, tris, q[None])[0]
            if each[0]["distance"] == each[1]["distance"] > 0 and whole["primitive_id"] == min(t, u) and whole["distance"] == each[0]["distance"] and both[0]["primitive_id"] == 0:
                return q, min(t, u), max(t, u)
    raise AssertionError("no wall found")


class SepCase:
    """a scene, its probes and their brute-force answers per max_distance -- computed once, shared, never changed"""

    def __init__(self, name, scene, n=130):
        self.name, self.scene = name, scene
        self.probes = make_probes(scene["triangles"], n, 9000 + n)
        q, self.tie_low, self.tie_high = equidistant_probe(scene["triangles"])
        for k, key in enumerate(("p1", "p2", "p3")):
            self.probes[key][1, :3] = q[k]
        self.wants = {}
        d = self.want(INF)
        d = d["distance"][(d["flags"] & FOUND != 0) & (d["distance"] > 0) & np.isfinite(d["distance"])]
        self.tight = float(np.median(d))

    def want(self, max_distance):
        if max_distance not in self.wants:
            w = capi.debug_separation(None, self.scene["triangles"], self.probes, max_distance)
            w.setflags(write=False)
            self.wants[max_distance] = w
        return self.wants[max_distance]

    def radii(self):
        return (INF, self.tight, 0.0)


def check_probes(case):
    """what the batch promises of its brute-force answer (asserted on the HOST's brute force)"""
    out, tight = case.want(INF), case.want(case.tight)
    k = np.arange(len(out)) % 13
    dead = np.isin(k, (9, 10))
    assert dead.sum() >= 2 and out[dead].tobytes() == np_none(dead.sum()).tobytes()
    live = out[~dead]
    assert (live["flags"] & SEARCHED != 0).all() and (live["flags"] & FOUND != 0).all()
    assert ((live["distance"] > 0).sum()) * 4 >= len(live), (live["distance"] > 0).mean()
    assert (live["flags"] & CROSSING != 0).any() and out["flags"][0] & CROSSING
    nothing = (tight["flags"] == SEARCHED) & (tight["primitive_id"] == INVALID)
    assert nothing.any() and (tight["flags"] & FOUND != 0).any() and not tight["distance"][nothing].any()
    f = live["feature"]
    assert (f <= 2).any() and ((f >= 3) & (f <= 5)).any() and ((f >= 6) & (f <= 14)).any() and (f == FEATURE_CROSSING).any(), np.bincount(f, minlength=16)
    # probe 1 is exactly as far from two triangles: the lower id wins whichever is met first
    tris = case.scene["triangles"]
    each = [capi.debug_separation(None, tris[[t]], case.probes[1:2])[0]["distance"] for t in (case.tie_low, case.tie_high)]
    assert each[0] == each[1] == out["distance"][1] > 0 and out["primitive_id"][1] == case.tie_low < case.tie_high
    zero = case.want(0.0)
    assert np.array_equal(zero["flags"] & FOUND != 0, (out["distance"] == 0) & (out["flags"] & FOUND != 0))


def np_none(n):
    out = np.zeros(n, T.separation)
    out["primitive_id"] = INVALID
    return out


@pytest.fixture(scope="module")
def scases(golden_scenes, city):
    return {"cornell": SepCase("cornell", golden_scenes["cornell"]), "coverage": SepCase("coverage", golden_scenes["coverage"]),
            "city": SepCase("city", city)}


@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_header_equals_numpy_restatement_byte_for_byte(scases, name):
    case = scases[name]
    P = positions(case.scene["triangles"]).astype(f32)
    for r in case.radii():
        same(case.want(r), np_separation(P, case.probes, r), (name, r))
    check_probes(case)
    with np.errstate(all="ignore"):
        assert (np.abs(corners_of(case.probes)).max((1, 2)) > 1e38).sum() >= 2
    # a negative or NaN max_distance searches nothing
    for bad in (-1.0, float("nan")):
        assert capi.debug_separation(None, case.scene["triangles"], case.probes, bad).tobytes() == np_none(len(case.probes)).tobytes()


# ---- 3. the bound

def test_box_bound_never_exceeds_the_distance():
    """sep_box_d2(box Q, B) <= d2 for every box B that holds T's corners, wherever d2 is no NaN: T's own box, that box grown by random non-negative amounts,
    and (below) the decoded slots of a folded tree.  d2 is the numpy restatement's, tied to the header through sqrtf(d2) == distance, byte for byte."""
    rng = np.random.default_rng(5)
    n = 30000
    mag = 10.0 ** rng.uniform(-20, 18, n)
    Q = rng.normal(size=(n, 3, 3)) * mag[:, None, None]
    P = rng.normal(size=(n, 3, 3)) * mag[:, None, None] + rng.normal(size=(n, 1, 3)) * (mag * rng.choice([0.0, 1.0, 30.0], n))[:, None, None]
    kind = np.arange(n) % 10
    P[kind == 1, 2] = P[kind == 1, 1]                                  # a zero-length edge
    P[kind == 2, 1:] = P[kind == 2, :1]                                # a point
    Q[kind == 3, 2] = (Q[kind == 3, 0] + Q[kind == 3, 1]) / 2          # zero area
    Q[kind == 4, 1] = Q[kind == 4, 0]
    big = kind == 5
    P[big] *= (3e38 / np.abs(P[big]).max((1, 2)))[:, None, None]       # squares, then differences, overflow to +inf
    Q[kind == 6] *= (1e30 / np.abs(Q[kind == 6]).max((1, 2)))[:, None, None]
    Q, P = Q.astype(f32), P.astype(f32)
    lib = capi.load()
    probes, tris = T.probes_from_corners(Q), np.ascontiguousarray(triangles_of(P))
    out = np.zeros(n, T.separation)
    for i in range(n):
        assert lib.rt_debug_separation(None, tris.ctypes.data + 160 * i, 1, probes.ctypes.data + 48 * i, 1, INF, out.ctypes.data + 48 * i) == 0
    crossing = out["flags"] & CROSSING != 0
    d2 = np.where(crossing, f32(0), np_candidates(Q, P)[0])
    found = out["flags"] & FOUND != 0
    assert np.array_equal(found, ~np.isnan(d2))
    with np.errstate(all="ignore"):
        assert np.sqrt(d2[found]).tobytes() == out["distance"][found].tobytes()
    qlo, qhi, lo, hi = Q.min(1), Q.max(1), P.min(1), P.max(1)
    ok = ~np.isnan(d2)
    assert ok.mean() > 0.9 and np.isinf(d2[ok]).any() and crossing.any() and (d2[ok] > 0).mean() > 0.5
    own = np_box_gap2(qlo, qhi, lo, hi)
    assert (own[ok] <= d2[ok]).all(), int((own[ok] > d2[ok]).sum())
    assert ((own == d2) & (own > 0) & ok).any()                        # the bound is attained: a strict comparison is what the tie rule needs
    with np.errstate(all="ignore"):
        for share in (1e-7, 1e-3, 1.0, 1e3):
            grow = (rng.uniform(0, 1, (n, 3)) * mag[:, None] * share).astype(f32)
            glo, ghi = (lo - grow * (rng.uniform(size=(n, 3)) < 0.7)).astype(f32), (hi + grow * (rng.uniform(size=(n, 3)) < 0.7)).astype(f32)
            assert (glo <= lo).all() and (ghi >= hi).all()
            grown = np_box_gap2(qlo, qhi, glo, ghi)
            assert (grown[ok] <= own[ok]).all() and (grown[ok] <= d2[ok]).all()


def test_box_bound_on_the_decoded_slots_of_a_folded_tree():
    c = _trees.case(next(name for name in _trees.names("built") if _trees.case(name).folds and len(_trees.case(name).nodes) > 200))
    tris = corpus_triangles(c)
    P = positions(tris).astype(f32)
    wide, entry = wide_of(c.nodes)
    count_at = {int(nd["offset"]): int(nd["num_primitives_axis"]) >> 16 for nd in c.nodes if int(nd["num_primitives_axis"]) >> 16}
    cells = np.stack([np.ldexp(f32(1.0), (((wide["meta"] >> (8 * a)) & 0xFF).astype(np.int32) - 127)) for a in range(3)], 1).astype(f32)
    slots = []                                                          # (lo, hi, first triangle, count) of every slot that is a leaf
    for w, rec in enumerate(wide):
        for k in range(4):
            ref = int(rec["ref"][k])
            if ref == EMPTY or not ref & LEAF:
                continue
            lo = (((rec["lo"] >> (8 * k)) & 0xFF).astype(f32) * cells[w] + rec["origin"]).astype(f32)
            hi = (((rec["hi"] >> (8 * k)) & 0xFF).astype(f32) * cells[w] + rec["origin"]).astype(f32)
            first = ref & ~LEAF
            for t in range(first, first + count_at[first]):
                slots.append((lo, hi, t))
    assert len(slots) == len(P)
    lo, hi, t = np.array([s[0] for s in slots]), np.array([s[1] for s in slots]), np.array([s[2] for s in slots])
    assert (lo <= P[t].min(1)).all() and (hi >= P[t].max(1)).all()
    rng = np.random.default_rng(11)
    ext = P.reshape(-1, 3).max(0) - P.reshape(-1, 3).min(0)
    for scale in (0.02, 0.5, 5.0):
        Q = (P[rng.integers(0, len(P), len(t))] + rng.normal(size=(len(t), 1, 3)) * ext * scale).astype(f32)
        d2 = np_candidates(Q, P[t])[0]                                  # (a crossing pair's 0 is below this, and its boxes overlap: the bound is 0 there)
        bound = np_box_gap2(Q.min(1), Q.max(1), lo, hi)
        ok = ~np.isnan(d2)
        assert ok.all() and (bound <= d2).all() and (bound > 0).any()
        flags = np.array([np_pair(Q[i], P[t[i]][None])[0][0] for i in range(0, len(t), 7)])
        assert not bound[::7][flags != 0].any()


# ---- 4. the walk equals brute force

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_walk_equals_brute_force_byte_for_byte(scases, name):
    case = scases[name]
    nodes, tris = case.scene["nodes"], case.scene["triangles"]
    for wide in (False, True):
        for r in case.radii():
            same(capi.debug_separation_walk(nodes, tris, case.probes, r, wide=wide), case.want(r), (name, r, wide))
    # the walk prunes: a probe that is not searched is not walked, and a tight radius tests far fewer triangles than there are
    _, tested = capi.debug_separation_walk(nodes, tris, case.probes, case.tight, counts=True)
    assert not tested[np.isin(np.arange(len(tested)) % 13, (9, 10))].any()
    small = np.arange(len(tested)) % 13 < 9
    small[0] = False
    assert int(tested[small].sum()) < small.sum() * len(tris)
    if name == "city":
        assert int(tested[small].sum()) * 20 < small.sum() * len(tris)


def corpus_probes(tris, n=48):
    """probes of the corpus scenes: triangles of the scene turned, shrunk or grown and moved; every fourth one spans the whole scene (the most entries pending)"""
    P = positions(tris).astype(np.float64)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    rng = np.random.default_rng(len(P) + n + 1)
    C = np.zeros((n, 3, 3))
    for i in range(n):
        t = P[rng.integers(0, len(P))]
        c = t.mean(0)
        C[i] = (t - c) @ rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)).T * rng.uniform(0.1, 3.0) + c + rng.normal(size=3) * (0.05, 0.5, 3.0)[i % 3] * ext
        if i % 4 == 0:
            nrm = rng.normal(size=3)
            u = np.cross(nrm, [1.0, 0.3, 0.2]); u /= np.linalg.norm(u)
            v = np.cross(nrm, u); v /= np.linalg.norm(v)
            m, r = lo + rng.uniform(0.3, 0.7, 3) * ext, 4.0 * float(np.linalg.norm(ext))
            C[i] = [m + r * u, m - 0.5 * r * u + 0.9 * r * v, m - 0.5 * r * u - 0.9 * r * v]
    return T.probes_from_corners(C)


def corpus_radius(tris):
    flat = positions(tris).reshape(-1, 3).astype(np.float64)
    return float(f32(0.05 * np.linalg.norm(np.maximum(flat.max(0) - flat.min(0), 1e-3))))


@pytest.mark.parametrize("name", _trees.names())
def test_walk_equals_brute_force_on_the_tree_corpus(name):
    c = _trees.case(name)
    tris = corpus_triangles(c)
    probes = corpus_probes(tris)
    for r in (INF, corpus_radius(tris), 0.0):
        want = capi.debug_separation(None, tris, probes, r)
        for wide in (False, True):
            if wide and not c.folds:
                with pytest.raises(capi.RtError):
                    capi.debug_separation_walk(c.nodes, tris, probes, r, wide=True)
                continue
            try:
                got = capi.debug_separation_walk(c.nodes, tris, probes, r, wide=wide)
            except capi.RtError as e:
                # a chain of 120 interior nodes can leave more children pending than the walk's stack holds: refused, never answered wrongly
                assert name in STACK_CHAINS and not wide and "deeper than the walk's stack" in str(e), (name, r, wide, str(e))
                continue
            same(got, want, (name, r, wide))


# ---- 5. the self form

def np_self_loop(P, first, n, max_distance, ids=None):
    """the self form from its definition, one pair at a time through the header's own pair answer (rt_debug_separation on a single triangle)"""
    tris = triangles_of(P)
    out = np_none(n)
    for i in range(n):
        q = P[first + i]
        if not np.isfinite(q).all():
            continue
        out["flags"][i] = SEARCHED
        best = None
        for t in range(len(P)):
            if t == first + i or (q[:, None, :] == P[t][None, :, :]).all(-1).any() or (ids is not None and ids[t] == ids[first + i]):
                continue
            r = capi.debug_separation(None, tris[[t]], q[None], max_distance)[0]
            if r["flags"] & FOUND and (best is None or r["distance"] < best["distance"]):
                best = r.copy()
                best["primitive_id"] = t
        if best is not None:
            out[i] = best
    return out


def test_self_form_skips_neighbours_and_measures_two_tetrahedra():
    apart, ids = tetra_pair([20, 0, 0])
    P = apart.astype(f32)
    tris = triangles_of(P)
    out = capi.debug_separation_self(None, tris)
    # every face of a closed tetrahedron shares corners with the other three: they are skipped, so each face's nearest is a face of the OTHER tetrahedron
    assert (out["flags"] == SEARCHED | FOUND).all() and (out["primitive_id"][:4] >= 4).all() and (out["primitive_id"][4:] < 4).all() and (out["distance"] > 0).all()
    assert out["distance"].min() == 12.0                                        # the corner (8, 0, 0) against the face x = 20
    same(out, np_self_loop(P, 0, 8, INF), "loop")
    same(out, np_separation(P, np.zeros(8, T.probe), INF, self_first=0), "numpy")
    assert (capi.debug_separation(None, tris, T.probes_from_corners(apart))["distance"] == 0).all()   # (as plain probes each finds itself)
    # a sub-range, a radius that leaves some with nothing
    same(capi.debug_separation_self(None, tris, 2, 5, 13.0), np_separation(P, np.zeros(5, T.probe), 13.0, self_first=2), "range")
    got = capi.debug_separation_self(None, tris, 0, 8, 12.0)
    assert 0 < (got["primitive_id"] == INVALID).sum() < 8 and (got["flags"] & SEARCHED != 0).all()
    # RT_SEPARATION_OTHER_OBJECTS: one object for all eight leaves nothing to find, the two tetrahedra as objects change nothing here
    one = np.zeros(8, np.uint32)
    got = capi.debug_separation_self(None, tris, options=capi.SEPARATION_OTHER_OBJECTS, object_of_triangle=one)
    assert (got["primitive_id"] == INVALID).all() and (got["flags"] == SEARCHED).all()
    same(capi.debug_separation_self(None, tris, options=capi.SEPARATION_OTHER_OBJECTS, object_of_triangle=ids), out, "two objects")
    mixed = np.array([0, 0, 1, 1, 1, 1, 0, 0], np.uint32)
    got = capi.debug_separation_self(None, tris, options=capi.SEPARATION_OTHER_OBJECTS, object_of_triangle=mixed)
    same(got, np_self_loop(P, 0, 8, INF, mixed), "mixed objects, loop")
    # interlocked: the faces that cut each other report a crossing at distance 0
    locked, ids = tetra_pair([1, 2, 1])
    out = capi.debug_separation_self(None, triangles_of(locked.astype(f32)), options=capi.SEPARATION_OTHER_OBJECTS, object_of_triangle=ids)
    want = capi.debug_cross_self(None, triangles_of(locked.astype(f32)), max_list=0, options=capi.CROSS_OTHER_OBJECTS, object_of_triangle=ids)
    assert np.array_equal(out["flags"] & CROSSING != 0, want["count"] > 0) and (want["count"] > 0).any()
    assert np.array_equal(out["primitive_id"][want["count"] > 0], want["first_primitive"][want["count"] > 0])


def test_self_form_on_a_scene_equals_numpy(golden_scenes):
    tris = golden_scenes["coverage"]["triangles"]
    P = positions(tris).astype(f32)
    n = min(len(P), 120)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 5, len(P)).astype(np.uint32)
    same(capi.debug_separation_self(None, tris, 0, n), np_separation(P, np.zeros(n, T.probe), INF, self_first=0), "self")
    same(capi.debug_separation_self(None, tris, 0, n, INF, capi.SEPARATION_OTHER_OBJECTS, ids),
         np_separation(P, np.zeros(n, T.probe), INF, self_first=0, ids=ids), "other objects")
    m = min(len(P), 24)
    same(capi.debug_separation_self(None, tris, 3, m, INF, capi.SEPARATION_OTHER_OBJECTS, ids), np_self_loop(P, 3, m, INF, ids), "loop")
