"""Crossing queries (rt_scene_cross / rt_scene_cross_self, raytracing_amd/csrc/cross.h) without a GPU.

The contract is a statement about the triangles alone: a probe Q crosses a scene triangle T when their closed boxes overlap, Q's plane does not have T's three
corners strictly on one side, and one of six segment-triangle tests accepts (Q's edges against T: bits 0..2, T's edges against Q: bits 3..5).  So (1) on
small-integer coordinates, where every intermediate up to the divisions is exact, the header's verdict and its six bits equal exact integer arithmetic;
(2) the header (rt_debug_cross's host brute force) is compared with a numpy restatement with the same operand order, byte for byte, records, members and
contact points; (3) the kernel's walk on the host (rt_debug_cross_walk, child-pair and 4-wide) equals the brute force on the scenes and on the tree corpus;
(4) the self form skips neighbours and, on request, pairs of one object."""
import random
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_nearest import INVALID, city, triangles_of          # noqa: F401 (fixtures)
from tests.test_refit import positions
from tests.test_within import STACK_CHAINS, corpus_triangles
from tests.test_region import rotation

f32 = np.float32
SEARCHED, ANY_MODE = 1, 2
MAX_LISTS = (0, 1, 3, 8)


# ---- cross.h in numpy (binary32, every operation rounded once, cross.h's operand order)

def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(x < y, y, x)


def np_segment(a, b, o, e1, e2):
    """cross_segment over broadcastable float32[..., 3]: (accepted, a + t * dir)"""
    d = b - a
    pv = _cross3(d, e2)
    det = _dot3(e1, pv)
    ok = (det > 0) | (det < 0)
    inv = f32(1.0) / det
    tv = a - o
    u = _dot3(tv, pv) * inv
    ok &= ~((u < 0) | (u > 1))
    qv = _cross3(tv, e1)
    v = _dot3(d, qv) * inv
    ok &= ~((v < 0) | (u + v > 1))
    t = _dot3(e2, qv) * inv
    ok &= (t >= 0) & (t <= 1)
    return ok, a + t[..., None] * d


def np_pair(q, P):
    """cross_pair of one probe q float32[3, 3] against triangles P float32[nt, 3, 3]: (flags uint32[nt], c0 float32[nt, 3], c1 float32[nt, 3]).  Steps 2 and
    3 are evaluated on the triangles that pass step 1 only (the others are no members whatever they would give)."""
    with np.errstate(all="ignore"):
        q = q.astype(f32)
        P_all = P.astype(f32)
        q1, q2, q3 = q
        qlo, qhi = _min(_min(q1, q2), q3), _max(_max(q1, q2), q3)
        tlo, thi = _min(_min(P_all[:, 0], P_all[:, 1]), P_all[:, 2]), _max(_max(P_all[:, 0], P_all[:, 1]), P_all[:, 2])
        boxes = np.flatnonzero(((qlo <= thi) & (tlo <= qhi)).all(1))
        P = P_all[boxes]
        p1, p2, p3 = P[:, 0], P[:, 1], P[:, 2]
        alive = np.ones(len(P), bool)
        qe1, qe2 = q2 - q1, q3 - q1
        n = _cross3(qe1, qe2)
        d = -_dot3(n, q1)
        if np.isfinite(n).all() and np.isfinite(d):
            s = ((n[0] * P[..., 0] + n[1] * P[..., 1]) + n[2] * P[..., 2]) + d               # [nt, 3]
            alive &= ~((s > 0).all(1) | (s < 0).all(1))
        te1, te2 = p2 - p1, p3 - p1
        Q = np.broadcast_to(q, P.shape)
        tests = [(Q[:, 0], Q[:, 1], p1, te1, te2), (Q[:, 1], Q[:, 2], p1, te1, te2), (Q[:, 2], Q[:, 0], p1, te1, te2),
                 (p1, p2, q1, qe1, qe2), (p2, p3, q1, qe1, qe2), (p3, p1, q1, qe1, qe2)]
        flags = np.zeros(len(P), np.uint32)
        seen = np.zeros(len(P), np.int64)
        c0, c1 = np.zeros((len(P), 3), f32), np.zeros((len(P), 3), f32)
        for k, (a, b, o, e1, e2) in enumerate(tests):
            ok, x = np_segment(a, b, o, e1, e2)
            ok &= alive
            c0[ok & (seen == 0)] = x[ok & (seen == 0)]
            c1[ok & (seen <= 1)] = x[ok & (seen <= 1)]
            flags[ok] |= np.uint32(1 << k)
            seen += ok
        F, C0, C1 = np.zeros(len(P_all), np.uint32), np.zeros((len(P_all), 3), f32), np.zeros((len(P_all), 3), f32)
        F[boxes], C0[boxes], C1[boxes] = flags, c0, c1
        return F, C0, C1


def corners_of(probes):
    return np.stack([probes["p1"][:, :3], probes["p2"][:, :3], probes["p3"][:, :3]], 1)


def np_cross(P, probes, max_list, any_mode=False, self_first=None, ids=None):
    """rt_debug_cross(NULL, ...) (self_first None) or rt_debug_cross_self(NULL, ...) in numpy: P float32[nt, 3, 3] -> (types.probe_hits[n], types.cross_member[n, max_list])"""
    C = corners_of(probes) if self_first is None else P[self_first:self_first + len(probes)]
    n = len(C)
    out = np.zeros(n, T.probe_hits)
    out["first_primitive"] = INVALID
    members = np.zeros((n, max_list), T.cross_member)
    members["primitive_id"] = INVALID
    for i, q in enumerate(C):
        if not np.isfinite(q).all():
            continue
        flags, c0, c1 = np_pair(q, P)
        member = flags != 0
        if self_first is not None:
            shared = (q[:, None, None, :] == P[None, :, :, :]).all(-1).any(0).any(-1)         # some corner of q equals some corner of the triangle
            member &= ~shared
            member[self_first + i] = False
            if ids is not None:
                member &= ids != ids[self_first + i]
        found = np.flatnonzero(member)
        if any_mode:
            out[i] = (min(len(found), 1), 0, INVALID, SEARCHED | ANY_MODE)
            continue
        out[i] = (len(found), min(len(found), max_list), found[0] if len(found) else INVALID, SEARCHED)
        for j, t in enumerate(found[:max_list]):
            members[i, j] = (t, flags[t], c0[t], c1[t])
    return out, members


def same(got, want, what=""):
    for g, w, names in ((got[0], want[0], T.probe_hits.names), (got[1], want[1], T.cross_member.names)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, [k for k in names if g[k].tobytes() != w[k].tobytes()],
                                                                    np.argwhere(np.array([a.tobytes() != b.tobytes() for a, b in zip(g.reshape(-1), w.reshape(-1))]))[:8].ravel())


def cross(fn, *args, max_list, options=0, **kw):
    """a capi cross function as (records, members): where nothing is listed the members are an empty [n, 0] array"""
    got = fn(*args, max_list=max_list, options=options, **kw)
    return got if isinstance(got, tuple) else (got, np.zeros((len(got), 0), T.cross_member))


# ---- 1. exact arithmetic on small integers

def exact_pairs(Q, P):
    """CROSS on integer corners Q, P int64[n, 3, 3], pair i = (Q[i], P[i]), in exact integer arithmetic -- numpy int64, not arbitrary precision: every magnitude is asserted to stay below 2^24, so nothing can wrap --:
    (flags int[n], strict bool[n]).  strict: no determinant is 0 and none of u, v, 1 - u - v, t, 1 - t is exactly 0 in any of the six tests."""
    Q, P = Q.astype(np.int64), P.astype(np.int64)
    dot = lambda a, b: (a * b).sum(-1)
    alive = ((Q.min(1) <= P.max(1)) & (P.min(1) <= Q.max(1))).all(1)
    qe1, qe2 = Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0]
    nrm = np.cross(qe1, qe2)
    s = (nrm[:, None, :] * P).sum(-1) - dot(nrm, Q[:, 0])[:, None]
    alive &= ~((s > 0).all(1) | (s < 0).all(1))
    te1, te2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    tests = [(Q[:, 0], Q[:, 1], P[:, 0], te1, te2), (Q[:, 1], Q[:, 2], P[:, 0], te1, te2), (Q[:, 2], Q[:, 0], P[:, 0], te1, te2),
             (P[:, 0], P[:, 1], Q[:, 0], qe1, qe2), (P[:, 1], P[:, 2], Q[:, 0], qe1, qe2), (P[:, 2], P[:, 0], Q[:, 0], qe1, qe2)]
    flags = np.zeros(len(Q), np.int64)
    strict = np.ones(len(Q), bool)
    biggest = 0
    for k, (a, b, o, e1, e2) in enumerate(tests):
        d = b - a
        pv = np.cross(d, e2)
        det = dot(e1, pv)
        tv = a - o
        qv = np.cross(tv, e1)
        sg = np.sign(det)
        un, vn, tn, m = dot(tv, pv) * sg, dot(d, qv) * sg, dot(e2, qv) * sg, np.abs(det)          # u = un / m, v = vn / m, t = tn / m where m > 0
        ok = (det != 0) & (un >= 0) & (un <= m) & (vn >= 0) & (un + vn <= m) & (tn >= 0) & (tn <= m)
        strict &= (det != 0) & (un != 0) & (vn != 0) & (un + vn != m) & (tn != 0) & (tn != m)
        flags |= (ok & alive).astype(np.int64) << k
        biggest = max(biggest, int(np.abs(np.stack([un, vn, tn, m])).max()), int(np.abs(pv).max()), int(np.abs(qv).max()))
    assert biggest < 2**24 and int(np.abs(s).max()) < 2**24
    return flags, strict


def test_exact_fixture_verdict_and_bits_equal_integer_arithmetic():
    random.seed(1)
    n = 20000
    C = np.array([random.randint(-16, 16) for _ in range(n * 18)], np.int64).reshape(n, 2, 3, 3)
    want, strict = exact_pairs(C[:, 0], C[:, 1])
    assert (~strict).mean() <= 0.05 and (want != 0).mean() >= 0.20, ((~strict).mean(), (want != 0).mean())
    assert all(((want >> k) & 1).any() for k in range(6))
    lib = capi.load()
    probes = T.probes_from_corners(C[:, 0])
    tris = np.ascontiguousarray(triangles_of(C[:, 1].astype(f32)))
    out, members = np.zeros(n, T.probe_hits), np.zeros(n, T.cross_member)
    pp, tp, op, mp = probes.ctypes.data, tris.ctypes.data, out.ctypes.data, members.ctypes.data
    for i in range(n):                                               # pair i on its own: one probe against one triangle
        assert lib.rt_debug_cross(None, tp + 160 * i, 1, pp + 48 * i, 1, 1, 0, op + 16 * i, mp + 32 * i) == 0
    got = np.where(out["count"] == 1, members["flags"], 0).astype(np.int64)
    assert ((out["count"] == 1) == (members["primitive_id"] == 0)).all() and (out["flags"] == SEARCHED).all()
    bad = np.flatnonzero(strict & (got != want))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    print("non-strict %.2f %%, crossing %.2f %%" % (100 * (~strict).mean(), 100 * (want != 0).mean()))


# ---- 2. the header against numpy on the scenes

def make_probes(tris, n, seed):
    """the mixed batch: scene triangles rotated about their centroid and displaced a little; then by index % 13: 9 a probe with a NaN, 10 one with an inf
    (not searched), 11 a zero-area probe (three points on a line), 12 coordinates near FLT_MAX (products overflow: the plane is not used); probe 0 spans the
    whole scene"""
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
        C[i] = (t - c) @ rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)).T * scale + c + rng.normal(size=3) * 0.02 * diag
        k = i % 13
        if k == 11:
            C[i, 2] = (C[i, 0] + C[i, 1]) / 2
        elif k == 12:
            C[i] *= 3.0e38 / np.abs(C[i]).max() * rng.uniform(0.3, 1.0)
    u, v, m = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0), (lo + hi) / 2                # a plane through the middle
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


def check_probes(out, n_tris):
    """what the batch promises of its brute-force answer (asserted on the HOST's brute force)"""
    k = np.arange(len(out)) % 13
    dead = np.isin(k, (9, 10))
    assert dead.sum() >= 2 and not out["count"][dead].any() and not out["flags"][dead].any() and (out["first_primitive"][dead] == INVALID).all()
    assert (out["flags"][~dead] == SEARCHED).all()
    assert (out["count"][~dead] >= 1).sum() * 4 >= (~dead).sum(), (out["count"][~dead] >= 1).mean()
    assert (out["count"] > 8).any() and out["count"][0] >= 1 and out["count"].max() < n_tris


class CrossCase:
    """a scene, its probes and their brute-force answers per (max_list, options) -- computed once, shared, never changed"""

    def __init__(self, name, scene, n=130):
        self.name, self.scene = name, scene
        self.probes = make_probes(scene["triangles"], n, 7000 + n)
        self.wants = {}

    def want(self, max_list, options=0):
        if (max_list, options) not in self.wants:
            w = cross(capi.debug_cross, None, self.scene["triangles"], self.probes, max_list=max_list, options=options)
            for a in w:
                a.setflags(write=False)
            self.wants[(max_list, options)] = w
        return self.wants[(max_list, options)]


@pytest.fixture(scope="module")
def ccases(golden_scenes, city):
    return {"cornell": CrossCase("cornell", golden_scenes["cornell"]), "coverage": CrossCase("coverage", golden_scenes["coverage"]),
            "city": CrossCase("city", city)}


@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_header_equals_numpy_restatement_byte_for_byte(ccases, name):
    case = ccases[name]
    P = positions(case.scene["triangles"]).astype(f32)
    ref = np_cross(P, case.probes, 8)                                 # once; a shorter list is its prefix
    for max_list in MAX_LISTS:
        cut = ref[0].copy()
        cut["stored"] = np.minimum(cut["count"], max_list)
        same(case.want(max_list), (cut, np.ascontiguousarray(ref[1][:, :max_list])), (name, max_list))
    hit = ref[0].copy()
    hit["count"], hit["stored"], hit["first_primitive"] = np.minimum(hit["count"], 1), 0, INVALID
    hit["flags"] = np.where(hit["flags"] != 0, SEARCHED | ANY_MODE, 0)
    same(case.want(0, capi.CROSS_ANY), (hit, ref[1][:, :0]), (name, "any"))
    out, members = case.want(8)
    check_probes(out, len(P))
    # a smaller list is a prefix; listed ids ascend; entries beyond `stored` are invalid and zero; first_primitive is the list's first
    for max_list in (1, 3):
        assert case.want(max_list)[1].tobytes() == members[:, :max_list].tobytes()
    listed = members["primitive_id"] != INVALID
    assert np.array_equal(listed.sum(1), out["stored"]) and np.array_equal(out["stored"], np.minimum(out["count"], 8))
    ids = np.where(listed, members["primitive_id"].astype(np.int64), 2**40)
    empty = members[~listed]
    assert (np.diff(ids, axis=1) >= 0).all() and not empty["flags"].any() and not empty["c0"].any() and not empty["c1"].any()
    assert np.array_equal(out["first_primitive"][out["count"] > 0], members["primitive_id"][out["count"] > 0, 0])
    flags = members["flags"][listed]
    assert (flags != 0).all() and (flags < 64).all() and (flags & 7).any() and (flags & 56).any()
    bits = np.array([bin(int(f)).count("1") for f in flags])
    assert (bits == 2).mean() > 0.8                                  # a generic crossing: two of the six tests, c0 c1 the intersection segment
    with np.errstate(all="ignore"):
        huge = np.abs(corners_of(case.probes)).max((1, 2)) > 1e38
    assert huge.sum() >= 2


# ---- 3. the walk equals brute force

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_walk_equals_brute_force_byte_for_byte(ccases, name):
    case = ccases[name]
    nodes, tris = case.scene["nodes"], case.scene["triangles"]
    for wide in (False, True):
        for max_list in MAX_LISTS:
            same(cross(capi.debug_cross_walk, nodes, tris, case.probes, max_list=max_list, wide=wide), case.want(max_list), (name, max_list, wide))
        same(cross(capi.debug_cross_walk, nodes, tris, case.probes, max_list=0, options=capi.CROSS_ANY, wide=wide), case.want(0, capi.CROSS_ANY), (name, "any", wide))
    # the walk prunes: summed over the batch far fewer triangles are tested than there are pairs; a probe that is not searched is not walked
    for options in (0, capi.CROSS_ANY):
        _, tested = capi.debug_cross_walk(nodes, tris, case.probes, 0, options, counts=True)
        assert int(tested.sum()) < len(case.probes) * len(tris)
        assert not tested[np.isin(np.arange(len(tested)) % 13, (9, 10))].any()
    if name == "city":
        assert int(tested.sum()) * 20 < len(case.probes) * len(tris)


def corpus_probes(tris, n=48):
    """probes of the corpus scenes: triangles of the scene turned and moved a little; every fourth one spans the whole scene (the most entries pending)"""
    P = positions(tris).astype(np.float64)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    rng = np.random.default_rng(len(P) + n)
    C = np.zeros((n, 3, 3))
    for i in range(n):
        t = P[rng.integers(0, len(P))]
        c = t.mean(0)
        C[i] = (t - c) @ rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)).T * rng.uniform(0.5, 3.0) + c + rng.normal(size=3) * 0.05 * ext
        if i % 4 == 0:
            nrm = rng.normal(size=3)
            u = np.cross(nrm, [1.0, 0.3, 0.2]); u /= np.linalg.norm(u)
            v = np.cross(nrm, u); v /= np.linalg.norm(v)
            m, r = lo + rng.uniform(0.3, 0.7, 3) * ext, 4.0 * float(np.linalg.norm(ext))
            C[i] = [m + r * u, m - 0.5 * r * u + 0.9 * r * v, m - 0.5 * r * u - 0.9 * r * v]
    return T.probes_from_corners(C)


@pytest.mark.parametrize("name", _trees.names())
def test_walk_equals_brute_force_on_the_tree_corpus(name):
    c = _trees.case(name)
    tris = corpus_triangles(c)
    probes = corpus_probes(tris)
    refused = []
    for max_list, options in ((0, 0), (1, 0), (3, 0), (8, 0), (0, capi.CROSS_ANY)):
        want = cross(capi.debug_cross, None, tris, probes, max_list=max_list, options=options)
        for wide in (False, True):
            if wide and not c.folds:
                with pytest.raises(capi.RtError):
                    capi.debug_cross_walk(c.nodes, tris, probes, max_list, options, wide=True)
                continue
            try:
                got = cross(capi.debug_cross_walk, c.nodes, tris, probes, max_list=max_list, options=options, wide=wide)
            except capi.RtError as e:
                # a chain of 120 interior nodes leaves more children pending than the walk's stack holds: refused, never answered wrongly
                assert name in STACK_CHAINS and not wide and "deeper than the walk's stack" in str(e), (name, max_list, wide, str(e))
                refused.append(max_list)
                continue
            same(got, want, (name, max_list, options, wide))
    if name not in STACK_CHAINS:
        assert not refused


def test_a_left_deep_chain_deeper_than_the_stack_is_refused():
    c = _trees.case("random, left 121")
    tris = corpus_triangles(c)
    flat = positions(tris).reshape(-1, 3).astype(np.float64)
    lo, hi = flat.min(0), flat.max(0)
    # a probe through the whole scene in a plane every leaf's box straddles is unlikely; what leaves every child pending is a probe whose plane is NOT used
    # (coordinates near FLT_MAX) and whose box holds everything
    big = T.probes_from_corners([[[-3e38, -3e38, -3e38], [3e38, 3e38, 3e38], [3e38, -3e38, 3e38]]])
    with pytest.raises(capi.RtError, match="deeper than the walk's stack"):
        capi.debug_cross_walk(c.nodes, tris, big, 8, wide=False)
    # the refusal is the stack's, not the tree's: a probe that reaches nothing leaves nothing pending and is answered on the same tree
    far = T.probes_from_corners([[hi + 10, hi + 11, hi + [10, 11, 10]]])
    same(cross(capi.debug_cross_walk, c.nodes, tris, far, max_list=8, wide=False), cross(capi.debug_cross, None, tris, far, max_list=8), "far")


# ---- 4. the self form

TETRA = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [0, 0, 8]], np.int64)
FACES = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])


def tetra_pair(offset):
    """two tetrahedra as eight triangles int64[8, 3, 3], the second one moved by `offset`; object 0 and object 1"""
    return np.concatenate([TETRA[FACES], (TETRA + np.asarray(offset))[FACES]]), np.repeat(np.arange(2, dtype=np.uint32), 4)


def test_self_form_skips_neighbours_and_finds_interlocked_tetrahedra():
    apart, ids = tetra_pair([20, 0, 0])
    tris = triangles_of(apart.astype(f32))
    # every face of a closed tetrahedron shares corners with every other one: without the skip each pair would touch along its edge
    out, members = capi.debug_cross_self(None, tris)
    assert not out["count"].any() and (out["flags"] == SEARCHED).all() and (members["primitive_id"] == INVALID).all()
    probes = T.probes_from_corners(apart)
    assert (capi.debug_cross(None, tris, probes, 8)[0]["count"] >= 3).all()                   # (the same triangles as probes: the neighbours do touch)

    locked, ids = tetra_pair([1, 2, 1])                                                       # the second one's corner region pokes through the first's faces
    tris = triangles_of(locked.astype(f32))
    P = locked.astype(f32)
    want_flags = np.zeros((8, 8), np.int64)
    for i in range(8):
        want_flags[i], strict = exact_pairs(np.broadcast_to(locked[i], locked.shape), locked)
    for i in range(8):                                                                        # the skip, from the definition
        for t in range(8):
            if i == t or (locked[i][:, None, :] == locked[t][None, :, :]).all(-1).any():
                want_flags[i, t] = 0
    assert (want_flags != 0).any() and np.array_equal(want_flags != 0, (want_flags != 0).T)
    assert not (want_flags[:4, :4] != 0).any() and not (want_flags[4:, 4:] != 0).any()       # no tetrahedron cuts itself
    out, members = capi.debug_cross_self(None, tris)
    for i in range(8):
        found = np.flatnonzero(want_flags[i])
        assert out["count"][i] == len(found) and np.array_equal(members["primitive_id"][i][:len(found)], found), (i, out[i], found)
    same((out, members), np_cross(P, np.zeros(8, T.probe), 8, self_first=0), "numpy")
    # a sub-range, a shorter list, any-mode
    same(cross(capi.debug_cross_self, None, tris, max_list=3, first=2, n=5), np_cross(P, np.zeros(5, T.probe), 3, self_first=2), "range")
    got = capi.debug_cross_self(None, tris, options=capi.CROSS_ANY)
    assert np.array_equal(got["count"], np.minimum(out["count"], 1)) and (got["flags"] == SEARCHED | ANY_MODE).all() and not got["stored"].any()
    # RT_CROSS_OTHER_OBJECTS: a mesh that cuts ITSELF no longer reports it -- one object for all eight triangles leaves nothing, two objects everything
    one = np.zeros(8, np.uint32)
    got = capi.debug_cross_self(None, tris, options=capi.CROSS_OTHER_OBJECTS, object_of_triangle=one)
    assert not got[0]["count"].any()
    same(capi.debug_cross_self(None, tris, options=capi.CROSS_OTHER_OBJECTS, object_of_triangle=ids), (out, members), "two objects")
    mixed = np.array([0, 0, 1, 1, 1, 1, 0, 0], np.uint32)
    got = capi.debug_cross_self(None, tris, options=capi.CROSS_OTHER_OBJECTS, object_of_triangle=mixed)
    same(got, np_cross(P, np.zeros(8, T.probe), 8, self_first=0, ids=mixed), "mixed objects")
    assert 0 < got[0]["count"].sum() < out["count"].sum()


def test_self_form_on_a_scene_equals_numpy(golden_scenes):
    tris = golden_scenes["coverage"]["triangles"]
    P = positions(tris).astype(f32)
    n = min(len(P), 200)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 5, len(P)).astype(np.uint32)
    same(capi.debug_cross_self(None, tris, 0, n, 8), np_cross(P, np.zeros(n, T.probe), 8, self_first=0), "self")
    same(capi.debug_cross_self(None, tris, 0, n, 8, capi.CROSS_OTHER_OBJECTS, ids), np_cross(P, np.zeros(n, T.probe), 8, self_first=0, ids=ids), "other objects")
