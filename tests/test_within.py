"""Within queries (rt_scene_within, raytracing_amd/csrc/within.h) without a GPU.

The contract is a statement about the triangles alone: per point the member set M = every triangle with d2 <= max_distance^2 (nearest.h's d2), ordered by
(d2, primitive_id); the count, and the first max_near members as rt_nearest records.  So (1) the header (rt_debug_within's host brute force) is compared with a
numpy restatement built on tests/test_nearest.py's np_triangle, byte for byte, over its header_case and the ties and edge radii of the contract; (2) the
kernel's walk on the host (rt_debug_within_walk, child-pair and 4-wide, counting and k-nearest) equals the brute force byte for byte on the scenes and on the
tree corpus; (3) the cross-checks with the nearest query; (4) the k-nearest walk prunes; (5) refusals and record sizes."""
import numpy as np
import pytest
from raytracing_amd import capi, scenes as S, types as T
from tests import _trees
from tests.test_nearest import (BACK_SIDE, CLASSES, FOUND, INVALID, NOT_SEARCHED, SHIFT, Case, city, dot3, f32, header_case, make_points, np_triangle,  # noqa: F401
                                points_of, triangles_of)
from tests.test_refit import positions

SEARCHED, K_NEAREST = 1, 2
MAX_NEARS = (0, 1, 3, 8)


# ---- within.h in numpy

def np_within(P, pts, max_near, k_nearest=False, chunk=64):
    """rt_debug_within(NULL, ...) in numpy: P float32[nt, 3, 3], pts types.point[n] -> (types.point_hits[n], types.nearest[n, max_near])"""
    n = len(pts)
    out = np.zeros(n, T.point_hits)
    out["nearest_primitive"] = INVALID
    near = np.zeros((n, max_near), T.nearest)
    near["primitive_id"] = INVALID
    pos, lim = pts["position"].astype(f32), pts["max_distance"].astype(f32)
    with np.errstate(all="ignore"):
        searched = np.isfinite(pos).all(1) & (lim >= 0)
        r2 = lim * lim
    ids = np.arange(len(P), dtype=np.uint32)
    for first in range(0, n, chunk):
        p = pos[first:first + chunk][:, None, :]
        q, d, d2, bu, bv, region = np_triangle(p, P[None, :, 0], P[None, :, 1], P[None, :, 2])
        for r in range(len(p)):
            i = first + r
            if not searched[i]:
                continue
            with np.errstate(all="ignore"):
                member = np.flatnonzero(d2[r] <= r2[i])                      # a NaN d2 fails the comparison
            # ascending (d2 as binary32, id): the bits of non-negative floats order as the floats do (+inf included)
            member = member[np.lexsort((ids[member], d2[r][member].view(np.uint32)))]
            stored = min(len(member), max_near)
            out["count"][i] = stored if k_nearest else len(member)
            out["stored"][i] = stored
            out["flags"][i] = SEARCHED | (K_NEAREST if k_nearest else 0)
            if len(member):
                out["nearest_primitive"][i] = member[0]
            for j, t in enumerate(member[:stored]):
                a, b = P[t, 1] - P[t, 0], P[t, 2] - P[t, 0]
                with np.errstate(all="ignore"):
                    g = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)
                    back = dot3(d[r, t], g) < 0
                    o = near[i, j]
                    o["position"] = q[r, t]
                    o["distance"] = np.sqrt(d2[r, t])
                    o["bc"] = (bu[r, t], bv[r, t])
                    o["primitive_id"] = t
                    o["flags"] = FOUND | (BACK_SIDE if back else 0) | (int(region[r, t]) << SHIFT)
    return out, near


def same(got, want, what=""):
    for g, w, names in ((got[0], want[0], T.point_hits.names), (got[1], want[1], T.nearest.names)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, [k for k in names if g[k].tobytes() != w[k].tobytes()],
                                                                    np.argwhere(np.array([a.tobytes() != b.tobytes() for a, b in zip(g.reshape(-1), w.reshape(-1))]))[:8].ravel())


# ---- 1. the header against numpy

def within_header_case():
    """header_case's triangles and points with finite radii on half of them, a stack of 12 coincident triangles, and the points of the contract's edges"""
    P, pts, n_good, first_quad = header_case()
    rng = np.random.default_rng(171)
    pts = pts.copy()
    some = np.flatnonzero(np.isinf(pts["max_distance"][:n_good]))[::2]
    pts["max_distance"][some] = rng.uniform(0.05, 1.5, len(some)).astype(f32)
    stack = np.tile(np.array([[[50, 0, 0], [51, 0, 0], [50, 1, 0]]], f32), (12, 1, 1))
    first_stack = len(P)
    P = np.concatenate([P, stack]).astype(f32)
    extra = np.concatenate([
        points_of(np.array([[50.25, 0.25, 0.5], [50.25, 0.25, 0.0], [49.0, -1.0, 0.25]], f32), 2.0),          # above, on and beside the stack: 12 ties
        points_of(P[[3, 17, 42, first_stack], 0], 0.0),                                                       # radius 0 exactly on a vertex
        points_of(np.array([[0.1, 0.2, 0.3], [50.0, 0.0, 1.0]], f32), np.inf),                                # radius +inf: every triangle with a d2
    ])
    return P, np.concatenate([pts[:n_good], extra, pts[n_good:]]), n_good, len(extra), first_quad, first_stack


def test_header_equals_numpy_restatement_byte_for_byte():
    P, pts, n_good, n_extra, first_quad, first_stack = within_header_case()
    tris = triangles_of(P)
    for max_near in MAX_NEARS:
        for knn in (False, True):
            if knn and max_near == 0:
                continue
            same(capi.debug_within(None, tris, pts, max_near, knn), np_within(P, pts, max_near, knn), ("within.h against numpy", max_near, knn))
    out, near = capi.debug_within(None, tris, pts, 8)
    ex = slice(n_good, n_good + n_extra)
    eo, en = out[ex], near[ex]
    # the stack of 12 coincident triangles: all counted, the 8 lowest ids listed in order
    for k in range(3):
        assert eo["count"][k] >= 12 and eo["stored"][k] == 8
        d = en["distance"][k]
        stack_ids = en["primitive_id"][k][d == d[np.flatnonzero(en["primitive_id"][k] >= first_stack)[0]]]
        assert (np.diff(stack_ids.astype(np.int64)) == 1).all() and stack_ids[0] == first_stack and len(stack_ids) >= 2
    assert (en["primitive_id"][0] == first_stack + np.arange(8)).all() and eo["count"][0] == 12              # nothing else within 2 of that point
    # radius 0 exactly on a vertex
    assert (eo["count"][3:7] >= 1).all() and (en["distance"][3:7, 0] == 0).all() and eo["count"][6] == 12
    # radius +inf: every triangle whose d2 is not NaN
    pos = pts["position"][ex][7:9]
    with np.errstate(all="ignore"):
        d2 = np_triangle(pos[:, None, :], P[None, :, 0], P[None, :, 1], P[None, :, 2])[2]
    assert (eo["count"][7:9] == (~np.isnan(d2)).sum(1)).all() and np.isnan(d2).any()
    # a point on a quad's diagonal: two members with equal d2, the lower id first
    ties = 0
    for i in range(n_good):
        ids, d = near["primitive_id"][i][:out["stored"][i]], near["distance"][i][:out["stored"][i]]
        for j in range(len(ids) - 1):
            if d[j] == d[j + 1] and ids[j] >= first_quad and ids[j + 1] == ids[j] + 1 and ids[j + 1] < first_stack:
                ties += 1
    assert ties >= 10, ties
    # not searched: NaN, non-finite and negative inputs
    bad = slice(n_good + n_extra, len(pts))
    assert len(pts[bad]) == 7 and out[bad].tobytes() == np_within(P, pts[bad], 8)[0].tobytes()
    assert not out["flags"][bad].any() and not out["count"][bad].any() and (out["nearest_primitive"][bad] == INVALID).all() and (near["primitive_id"][bad] == INVALID).all()
    # non-vacuity of the rest
    good = out[:n_good]
    assert (good["count"] == 0).sum() >= 50 and ((good["count"] >= 1) & (good["count"] <= 8)).sum() >= 50 and (good["count"] > 8).sum() >= 50


# ---- 2. the walk equals brute force

def radius_of(case_name, diagonal):
    """per scene: a radius at which the drawn points fall into all three classes of `count` (asserted on the brute force's output below)"""
    return f32(diagonal * {"cornell": 0.12, "coverage": 0.08, "city": 0.02}[case_name])


class WithinCase:
    """a scene, its points and their brute-force answers per (max_near, mode) -- computed once, shared, never changed"""

    def __init__(self, name, scene, n=1031):
        self.name, self.scene = name, scene
        tris = scene["triangles"]
        flat = positions(tris).reshape(-1, 3)
        self.diagonal = float(np.linalg.norm(flat.max(0) - flat.min(0)))
        pts = make_points(tris, n, 3000 + n).copy()
        # make_points' radii stay on classes 4 and 5 (half and twice the nearest distance) and on the not-searched ones; every other point gets the scene's
        cls = np.arange(n) % CLASSES
        free = ~np.isin(cls, (4, 5, NOT_SEARCHED))
        pts["max_distance"][free] = radius_of(name, self.diagonal)
        pts["max_distance"][np.flatnonzero(cls == 0)[::5]] = np.inf
        self.pts = pts
        self.wants = {}

    def want(self, max_near, knn):
        key = (max_near, knn)
        if key not in self.wants:
            w = capi.debug_within(None, self.scene["triangles"], self.pts, max_near, knn)
            for a in w:
                a.setflags(write=False)
            self.wants[key] = w
        return self.wants[key]


@pytest.fixture(scope="module")
def wcases(golden_scenes, city):
    return {"cornell": WithinCase("cornell", golden_scenes["cornell"]), "coverage": WithinCase("coverage", golden_scenes["coverage"]),
            "city": WithinCase("city", city, 520)}


def check_classes(out):
    c = out["count"]
    assert (c == 0).sum() >= 50 and ((c >= 1) & (c <= 8)).sum() >= 50 and (c > 8).sum() >= 50, ((c == 0).sum(), ((c >= 1) & (c <= 8)).sum(), (c > 8).sum())


@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_walk_equals_brute_force_byte_for_byte(wcases, name):
    case = wcases[name]
    check_classes(case.want(0, False)[0])
    for max_near in MAX_NEARS:
        for knn in (False, True):
            if knn and max_near == 0:
                continue
            for wide in (False, True):
                same(capi.debug_within_walk(case.scene["nodes"], case.scene["triangles"], case.pts, max_near, knn, wide=wide), case.want(max_near, knn),
                     (name, max_near, knn, wide))


# the four chains of 120 interior nodes (tests/_trees.py): a walk that prunes nothing leaves up to 120 siblings pending, over RT_W4_STACK_MAX
STACK_CHAINS = ("random, left 121", "random, right 121", "identical, left 121", "identical, right 121")


def corpus_triangles(c):
    """a corpus tree's triangles: its own, or one triangle per leaf box of a synthesised tree (corners inside the box: lo, a mixed corner, hi)"""
    if c.tris is not None:
        return c.tris
    leaves = c.nodes[_trees.is_leaf(c.nodes)]
    order = np.argsort(leaves["offset"])
    lo = np.stack([leaves["bounds_min"][k] for k in "xyz"], 1)[order]
    hi = np.stack([leaves["bounds_max"][k] for k in "xyz"], 1)[order]
    return triangles_of(np.stack([lo, np.stack([hi[:, 0], lo[:, 1], hi[:, 2]], 1), hi], 1).astype(f32))


@pytest.mark.parametrize("name", _trees.names())
def test_walk_equals_brute_force_on_the_tree_corpus(name):
    c = _trees.case(name)
    tris = corpus_triangles(c)
    P = positions(tris).astype(np.float64).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    rng = np.random.default_rng(len(c.nodes))
    n = 48
    pos = (lo + rng.uniform(-0.1, 1.1, (n, 3)) * (hi - lo)).astype(f32)
    pos[::4] = P[rng.integers(0, len(P), len(pos[::4]))].astype(f32)            # on corners
    share = rng.choice([0.0, 0.05, 0.3, np.inf], n)
    radius = np.where(np.isinf(share), np.inf, np.linalg.norm(hi - lo) * np.where(np.isinf(share), 0.0, share)).astype(f32)
    pts = points_of(pos, radius)
    refused = []
    for max_near, knn in ((0, False), (3, False), (8, False), (1, True), (8, True)):
        want = capi.debug_within(None, tris, pts, max_near, knn)
        for wide in (False, True):
            if wide and not c.folds:
                with pytest.raises(capi.RtError):
                    capi.debug_within_walk(c.nodes, tris, pts, max_near, knn, wide=True)
                continue
            try:
                got = capi.debug_within_walk(c.nodes, tris, pts, max_near, knn, wide=wide)
            except capi.RtError as e:
                # a chain of 120 interior nodes leaves more children pending than the walk's stack holds: the child-pair walk of these four trees
                # (which do not fold: the 4-wide form is refused above) may be refused, never answered wrongly; no other tree and no other message
                assert name in STACK_CHAINS and not wide and "deeper than the walk's stack" in str(e), (name, max_near, knn, wide, str(e))
                refused.append((max_near, knn))
                continue
            same(got, want, (name, max_near, knn, wide))
    assert capi.debug_within(None, tris, pts, 0)[0]["count"].max() >= 1
    if name in STACK_CHAINS:
        # the refusal is the stack's, not the tree's: points whose radius reaches nothing leave nothing pending, and those are answered on the same tree
        far = points_of((hi + (hi - lo) * 2 + 1).astype(f32)[None].repeat(4, 0), f32(np.linalg.norm(hi - lo) * 0.5 + 0.25))
        same(capi.debug_within_walk(c.nodes, tris, far, 8, False, wide=False), capi.debug_within(None, tris, far, 8, False), (name, "far"))
    else:
        assert not refused


# ---- 3. cross-checks with the nearest query

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_cross_checks_with_the_nearest_query(wcases, name):
    case = wcases[name]
    nodes, tris, pts = case.scene["nodes"], case.scene["triangles"], case.pts
    nearest = capi.debug_nearest(None, tris, pts)
    walk1 = capi.debug_nearest_walk(nodes, tris, pts)
    out1, near1 = capi.debug_within_walk(nodes, tris, pts, 1, True)
    assert near1[:, 0].tobytes() == walk1.tobytes() == nearest.tobytes()                   # k = 1: rt_scene_nearest's record
    for max_near in MAX_NEARS:
        out, near = case.want(max_near, False)
        assert np.array_equal(out["nearest_primitive"], nearest["primitive_id"])
        assert np.array_equal(out["count"] > 0, nearest["primitive_id"] != INVALID)
        assert np.array_equal(out["stored"], np.minimum(out["count"], max_near))
        if max_near:
            assert near.tobytes() == case.want(8, False)[1][:, :max_near].tobytes()        # a prefix of the longer list
            kout, knear = case.want(max_near, True)
            assert knear.tobytes() == near.tobytes()                                       # the k-nearest list is the counting mode's
            assert np.array_equal(kout["count"], kout["stored"]) and np.array_equal(kout["stored"], out["stored"])
            assert np.array_equal(kout["flags"], out["flags"] | np.where(out["flags"] & SEARCHED, K_NEAREST, 0))
            listed = near["primitive_id"] != INVALID
            assert np.array_equal(listed.sum(1), out["stored"]) and (listed[:, :-1] >= listed[:, 1:]).all()
            d = np.where(listed, near["distance"], np.inf)
            assert (d[:, :-1] <= d[:, 1:]).all()
    cls = np.arange(len(pts)) % CLASSES
    assert not case.want(8, False)[0]["flags"][cls == NOT_SEARCHED].any()


# ---- 4. the k-nearest mode prunes

def test_k_nearest_walk_prunes(wcases):
    """share of point x triangle pairs a k = 8 walk with radius +inf tests on the 40 000-triangle city: below 1 %.  Measured on the host walk: 0.00136
    (child-pair records) and 0.00097 (4-wide records)."""
    case = wcases["city"]
    cls = np.arange(len(case.pts)) % CLASSES
    pts = points_of(case.pts["position"][cls == 0])
    nt = len(case.scene["triangles"])
    for wide in (False, True):
        out, near, tested = capi.debug_within_walk(case.scene["nodes"], case.scene["triangles"], pts, 8, True, wide=wide, counts=True)
        share = tested.sum() / (len(pts) * nt)
        print("share of point x triangle pairs tested, wide =", wide, ":", share)
        assert (out["stored"] == 8).all() and tested.min() >= 8 and share < 0.01, share
    _, _, none = capi.debug_within_walk(case.scene["nodes"], case.scene["triangles"], case.pts[cls == NOT_SEARCHED], 8, True, counts=True)
    assert not none.any()                                                       # a point that is not searched is not walked


# ---- 5. refusals and record sizes

def test_refusals_and_record_sizes(golden_scenes):
    assert T.point_hits.itemsize == 16 and capi.WITHIN_MAX == 8
    lib = capi.load()
    sc = golden_scenes["cornell"]
    tris, nodes = np.ascontiguousarray(sc["triangles"]), np.ascontiguousarray(sc["nodes"])
    pts, out, near = points_of(np.zeros((4, 3), f32)), np.zeros(4, T.point_hits), np.zeros((4, 8), T.nearest)
    p = lambda a: a.ctypes.data

    def refused(rc, text):
        assert rc != 0 and text in lib.rt_last_error(None).decode(), (rc, lib.rt_last_error(None).decode())

    refused(lib.rt_scene_within(None, p(pts), 4, 8, 0, p(out), p(near), None), "ctx is NULL")
    refused(lib.rt_scene_within_buffer(None, None, 4, 8, 0, None, None, None), "ctx is NULL")
    refused(lib.rt_scene_within(None, None, 0, 0, 0, None, None, None), "ctx is NULL")
    for call, tail in ((lambda *a: lib.rt_debug_within(None, p(tris), len(tris), *a), ()),
                       (lambda *a: lib.rt_debug_within_walk(p(nodes), len(nodes), p(tris), len(tris), 1, *a), (None,))):
        refused(call(None, 4, 8, 0, p(out), p(near), *tail), "NULL argument")
        refused(call(p(pts), 4, 8, 0, None, p(near), *tail), "NULL argument")
        refused(call(p(pts), 4, 8, 0, p(out), None, *tail), "NULL argument")
        refused(call(p(pts), 4, 9, 0, p(out), p(near), *tail), "RT_WITHIN_MAX")
        refused(call(p(pts), 4, 0, 1, p(out), None, *tail), "max_near >= 1")
        refused(call(p(pts), 4, 8, 2, p(out), p(near), *tail), "unknown option bits")
        assert call(None, 0, 0, 0, None, None, *tail) == 0                                  # n == 0: RT_OK, nothing done
    refused(lib.rt_debug_within(None, None, len(tris), p(pts), 4, 8, 0, p(out), p(near)), "NULL argument")
    refused(lib.rt_debug_within_walk(None, len(nodes), p(tris), len(tris), 1, p(pts), 4, 8, 0, p(out), p(near), None), "NULL argument")
    refused(lib.rt_debug_within_walk(p(nodes), len(nodes), p(tris), len(tris), 2, p(pts), 4, 8, 0, p(out), p(near), None), "wide must be")
    refused(lib.rt_debug_within_walk(p(nodes), len(nodes), p(tris), len(tris) - 1, 0, p(pts), 4, 8, 0, p(out), p(near), None), "outside the array")
    assert out.tobytes() == bytes(out.nbytes) and near.tobytes() == bytes(near.nbytes)      # nothing was written by any of them
    assert lib.rt_debug_within(None, p(tris), len(tris), p(pts), 4, 0, 0, p(out), None) == 0            # max_near == 0: near may be NULL
    assert (out["flags"] == SEARCHED).all()
