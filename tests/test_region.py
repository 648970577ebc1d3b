"""Overlap queries (rt_scene_overlap / rt_scene_select / rt_frame_pick_rect, raytracing_amd/csrc/region.h) without a GPU.

The contract is a statement about the triangles alone: per region (up to 8 half-spaces, s_k(x) = ((nx x0 + ny x1) + nz x2) + d in binary32, outside when
s_k > 0) a triangle is rejected when one plane has all three corners outside, inside when no plane has any, touching otherwise or when inside; the count of
touching and of inside triangles and the touching ones with the lowest ids.  So (1) the header (rt_debug_overlap's host brute force) is compared with a numpy
restatement with the same operand order, byte for byte; (2) the kernel's walk on the host (rt_debug_overlap_walk, child-pair and 4-wide) equals the brute
force on the scenes and on the tree corpus, with coefficients near FLT_MAX too (the exactness argument's overflow case); (3) rt_debug_select agrees with the
overlap answers region by region; (4) the planes of a pixel rectangle hold the rectangle's pixel centres and none just outside; (5) refusals and sizes."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_nearest import INVALID, city, triangles_of          # noqa: F401 (fixtures)
from tests.test_refit import positions
from tests.test_within import STACK_CHAINS, corpus_triangles

f32 = np.float32
SEARCHED, INSIDE, CROSSING_SHIFT = 1, 1, 8
MAX_LISTS = (0, 1, 3, 8)
CLASSES = 12          # region i of a case is of class i % CLASSES (make_regions)
(BOX, ENCLOSING, FAR, HALF_SPACE, ROTATED, SLAB, FRUSTUM, WEDGE, NO_PLANES, NINE_PLANES, NAN_COEFFICIENT, INF_COEFFICIENT) = range(CLASSES)
NOT_SEARCHED = (NO_PLANES, NINE_PLANES, NAN_COEFFICIENT, INF_COEFFICIENT)


# ---- region.h in numpy

def np_planes(pl, X):
    """s_k(x) for planes float32[k, 4] and points float32[..., 3] -> float32[..., k], region.h's operand order"""
    pl, X = pl.astype(f32), X.astype(f32)[..., None, :]
    with np.errstate(all="ignore"):
        return ((pl[:, 0] * X[..., 0] + pl[:, 1] * X[..., 1]) + pl[:, 2] * X[..., 2]) + pl[:, 3]


def np_overlap(P, regions, max_list):
    """rt_debug_overlap(NULL, ...) in numpy: P float32[nt, 3, 3], regions types.region[n] -> (types.region_hits[n], types.region_member[n, max_list])"""
    n = len(regions)
    out = np.zeros(n, T.region_hits)
    members = np.zeros((n, max_list), T.region_member)
    members["primitive_id"] = INVALID
    for i, g in enumerate(regions):
        k = int(g["num_planes"])
        if not 1 <= k <= 8 or not np.isfinite(g["planes"][:k]).all():
            continue
        with np.errstate(all="ignore"):
            outside = (np_planes(g["planes"][:k], P) > 0).sum(1)              # [nt, k]: corners outside plane k
        touching = ~(outside == 3).any(1)
        inside = (outside == 0).all(1)
        ids = np.flatnonzero(touching)
        out[i] = (len(ids), inside.sum(), min(len(ids), max_list), SEARCHED)
        for j, t in enumerate(ids[:max_list]):
            flags = INSIDE if inside[t] else int(sum(1 << (CROSSING_SHIFT + a) for a in range(k) if outside[t, a]))
            members[i, j] = (t, flags)
    return out, members


def same(got, want, what=""):
    for g, w, names in ((got[0], want[0], T.region_hits.names), (got[1], want[1], T.region_member.names)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, [k for k in names if g[k].tobytes() != w[k].tobytes()],
                                                                    np.argwhere(np.array([a.tobytes() != b.tobytes() for a, b in zip(g.reshape(-1), w.reshape(-1))]))[:8].ravel())


# ---- the regions of a case

def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def look_camera(position, front, up=(0.0, 0.0, 1.0), size=32):
    cam = T.default_camera(size, size).copy()
    f = np.asarray(front, np.float64) / np.linalg.norm(front)
    r = np.cross(f, up); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    for k, a in enumerate("xyz"):
        cam["position"][a], cam["front"][a], cam["up"][a] = position[k], f[k], u[k]
    return cam


def make_regions(tris, n, seed):
    """the mixed batch: region i is of class i % CLASSES -- an axis-aligned box, a box around the whole scene, a box far away, one half-space through the
    middle, a rotated box, a slab whose first plane lies exactly on the scene's lowest x (a Cornell wall), a 5-plane frustum, an 8-plane wedge, and the four
    kinds that are not searched"""
    rng = np.random.default_rng(seed)
    flat = positions(tris).astype(np.float64).reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    ext, mid, diag = hi - lo, (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    out = np.zeros(n, T.region)
    for i in range(n):
        cls = i % CLASSES
        c = lo + rng.uniform(0.2, 0.8, 3) * ext
        h = rng.uniform(0.15, 0.45, 3) * ext
        if cls == BOX:
            g = T.box_region(c - h, c + h)
        elif cls == ENCLOSING:
            g = T.box_region(lo - 0.01 * diag - 1e-3, hi + 0.01 * diag + 1e-3)
        elif cls == FAR:
            g = T.box_region(hi + 2 * diag + 1, hi + 3 * diag + 2)
        elif cls == HALF_SPACE:
            nrm = rng.normal(size=3)
            g = T.planes_region([[*nrm, -nrm @ (mid + rng.uniform(-0.1, 0.1, 3) * ext)]])
        elif cls == ROTATED:
            m = np.concatenate([rotation(rng.normal(size=3), rng.uniform(0.2, 1.2)) * rng.uniform(0.5, 2.0), c[:, None]], 1)
            g = T.oriented_box_region(m, h)
        elif cls == SLAB:
            g = T.planes_region([[-1, 0, 0, f32(lo[0])], [1, 0, 0, -f32(lo[0] + rng.uniform(0.0, 0.6) * ext[0])]])       # lo.x <= x <= lo.x + part of the extent
        elif cls == FRUSTUM:
            cam = look_camera(mid + np.array([0.0, -1.2 * diag, 0.1 * diag]), (0.0, 1.0, -0.08))
            x0, y0 = rng.integers(0, 20, 2)
            g = capi.debug_rect_region(cam, 32, 32, int(x0), int(y0), int(x0 + rng.integers(4, 12)), int(y0 + rng.integers(4, 12)), 0.0, 1.5 * diag)
            assert g["num_planes"] == 5
        elif cls == WEDGE:
            b = T.box_region(c - 1.5 * h, c + 1.5 * h)
            d1, d2 = np.array([1.0, 1.0, 0.0]), np.array([-1.0, 0.5, 1.0])
            g = T.planes_region(np.concatenate([b["planes"][:6], [[*d1, -d1 @ (c + 0.5 * h)], [*d2, -d2 @ (c + 0.5 * h)]]]))
        else:
            g = T.box_region(c - h, c + h)
            if cls == NO_PLANES:
                g["num_planes"] = 0
            elif cls == NINE_PLANES:
                g["num_planes"] = 9
            elif cls == NAN_COEFFICIENT:
                g["planes"][rng.integers(0, 6), rng.integers(0, 4)] = np.nan
            else:
                g["planes"][rng.integers(0, 6), rng.integers(0, 4)] = np.inf if i % 2 else -np.inf
        g["reserved"] = rng.integers(0, 2**32, 3, dtype=np.uint64).astype(np.uint32)          # ignored
        out[i] = g
    return out


def check_classes(out, nt):
    """what the classes promise of a case's brute-force answer: no class is degenerate (asserted on the HOST's brute force)"""
    cls = np.arange(len(out)) % CLASSES
    c, ins = out["count"].astype(np.int64), out["inside"].astype(np.int64)
    assert (ins <= c).all() and (out["flags"][~np.isin(cls, NOT_SEARCHED)] == SEARCHED).all()
    assert ((0 < ins) & (ins < c))[cls == BOX].sum() >= 2, (c[cls == BOX], ins[cls == BOX])
    assert (c[cls == ENCLOSING] == nt).all() and (ins[cls == ENCLOSING] == nt).all()
    assert (c[cls == FAR] == 0).all()
    assert ((0 < c) & (c < nt) & (ins < c))[cls == HALF_SPACE].all()
    assert (c[cls == ROTATED] > 0).sum() >= 2
    assert (ins[cls == SLAB] > 0).sum() >= 2 and (c[cls == SLAB] < nt).any()
    assert ((c[cls == FRUSTUM] > 0) & (c[cls == FRUSTUM] < nt)).sum() >= 2
    assert (c[cls == WEDGE] > 0).sum() >= 2
    bad = np.isin(cls, NOT_SEARCHED)
    assert bad.sum() >= 4 and out[bad].tobytes() == bytes(16 * bad.sum())


class RegionCase:
    """a scene, its regions and their brute-force answers per max_list -- computed once, shared, never changed"""

    def __init__(self, name, scene, n=134):
        self.name, self.scene = name, scene
        self.regions = make_regions(scene["triangles"], n, 4000 + n)
        self.wants = {}

    def want(self, max_list):
        if max_list not in self.wants:
            w = capi.debug_overlap(None, self.scene["triangles"], self.regions, max_list)
            for a in w:
                a.setflags(write=False)
            self.wants[max_list] = w
        return self.wants[max_list]


@pytest.fixture(scope="module")
def rcases(golden_scenes, city):
    return {"cornell": RegionCase("cornell", golden_scenes["cornell"]), "coverage": RegionCase("coverage", golden_scenes["coverage"]),
            "city": RegionCase("city", city)}


# ---- 1. the header against numpy

@pytest.mark.parametrize("name", ["cornell", "coverage"])
def test_header_equals_numpy_restatement_byte_for_byte(rcases, name):
    case = rcases[name]
    P = positions(case.scene["triangles"]).astype(f32)
    for max_list in MAX_LISTS:
        same(case.want(max_list), np_overlap(P, case.regions, max_list), (name, max_list))
    out, members = case.want(8)
    check_classes(out, len(P))
    # a smaller list is a prefix; listed ids ascend; entries beyond `stored` are invalid
    for max_list in (1, 3):
        assert case.want(max_list)[1].tobytes() == members[:, :max_list].tobytes()
    listed = members["primitive_id"] != INVALID
    assert np.array_equal(listed.sum(1), out["stored"]) and np.array_equal(out["stored"], np.minimum(out["count"], 8))
    ids = np.where(listed, members["primitive_id"].astype(np.int64), 2**40)
    assert (np.diff(ids, axis=1) >= 0).all() and not members["flags"][~listed].any()
    assert (members["flags"][listed] & INSIDE).any() and (members["flags"][listed] >> CROSSING_SHIFT).any()


def test_corners_on_a_plane_count_as_inside(golden_scenes):
    """a slab whose first plane lies exactly on a Cornell wall: the wall's corners evaluate to 0 there, which is not outside"""
    tris = golden_scenes["cornell"]["triangles"]
    P = positions(tris).astype(f32)
    x = P[:, :, 0]
    wall = np.flatnonzero((x == x.min()).all(1))
    assert len(wall) >= 2
    g = T.planes_region([[-1, 0, 0, x.min()], [1, 0, 0, -x.min()]])          # the slab x == the wall's x: nothing but the wall is inside
    out, members = capi.debug_overlap(None, tris, [g], 8)
    assert out["inside"][0] == len(wall) and out["count"][0] > len(wall)
    assert set(members["primitive_id"][0][(members["flags"][0] & INSIDE) != 0]) <= set(wall)
    same((out, members), np_overlap(P, np.array([g]), 8), "the wall")


# ---- 2. the walk equals brute force

@pytest.mark.parametrize("name", ["cornell", "coverage", "city"])
def test_walk_equals_brute_force_byte_for_byte(rcases, name):
    case = rcases[name]
    nt = len(case.scene["triangles"])
    check_classes(case.want(0)[0], nt)
    for max_list in MAX_LISTS:
        for wide in (False, True):
            same(capi.debug_overlap_walk(case.scene["nodes"], case.scene["triangles"], case.regions, max_list, wide=wide), case.want(max_list), (name, max_list, wide))
    # the walk prunes: a far box tests nothing, a small box far fewer triangles than there are, a region that is not searched is not walked
    cls = np.arange(len(case.regions)) % CLASSES
    _, _, tested = capi.debug_overlap_walk(case.scene["nodes"], case.scene["triangles"], case.regions, 0, counts=True)
    assert not tested[cls == FAR].any() and not tested[np.isin(cls, NOT_SEARCHED)].any() and (tested[cls == ENCLOSING] == nt).all()
    if name == "city":
        assert tested[cls == FRUSTUM].max() < nt


def corpus_regions(tris, n=48, huge=False):
    P = positions(tris).astype(np.float64).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    rng = np.random.default_rng(len(P) + n)
    out = np.zeros(n, T.region)
    for i in range(n):
        c, h = lo + rng.uniform(-0.1, 1.1, 3) * ext, rng.uniform(0.05, 0.6, 3) * ext
        if i % 4 == 0:
            g = T.box_region(lo - ext - 1, hi + ext + 1)                      # encloses everything: the most entries pending
        elif i % 4 == 1:
            nrm = rng.normal(size=3)
            g = T.planes_region([[*nrm, -nrm @ c]])
        elif i % 4 == 2:
            g = T.oriented_box_region(np.concatenate([rotation(rng.normal(size=3), rng.uniform(0, 3)), c[:, None]], 1), h)
        else:
            g = T.box_region(c - h, c + h)
        if huge:
            # coefficients near FLT_MAX: every product with a coordinate above 1 overflows, sums meet inf - inf
            scale = 3.0e38 / float(np.abs(g["planes"][:int(g["num_planes"])]).max())
            g["planes"] = (g["planes"].astype(np.float64) * scale * rng.uniform(0.5, 1.0)).astype(f32)
        out[i] = g
    return out


@pytest.mark.parametrize("name", _trees.names())
def test_walk_equals_brute_force_on_the_tree_corpus(name):
    c = _trees.case(name)
    tris = corpus_triangles(c)
    regions = corpus_regions(tris)
    refused = []
    for max_list in (0, 3, 8):
        want = capi.debug_overlap(None, tris, regions, max_list)
        for wide in (False, True):
            if wide and not c.folds:
                with pytest.raises(capi.RtError):
                    capi.debug_overlap_walk(c.nodes, tris, regions, max_list, wide=True)
                continue
            try:
                got = capi.debug_overlap_walk(c.nodes, tris, regions, max_list, wide=wide)
            except capi.RtError as e:
                # a chain of 120 interior nodes leaves more children pending than the walk's stack holds: refused, never answered wrongly
                assert name in STACK_CHAINS and not wide and "deeper than the walk's stack" in str(e), (name, max_list, wide, str(e))
                refused.append(max_list)
                continue
            same(got, want, (name, max_list, wide))
    assert capi.debug_overlap(None, tris, regions, 0)[0]["count"].max() == len(tris)
    if name not in STACK_CHAINS:
        assert not refused


def test_a_left_deep_chain_deeper_than_the_stack_is_refused():
    c = _trees.case("random, left 121")
    tris = corpus_triangles(c)
    P = positions(tris).reshape(-1, 3)
    everything = T.box_region(P.min(0) - 1, P.max(0) + 1)
    with pytest.raises(capi.RtError, match="deeper than the walk's stack"):
        capi.debug_overlap_walk(c.nodes, tris, [everything], 8, wide=False)
    # the refusal is the stack's, not the tree's: a region that reaches nothing leaves nothing pending and is answered on the same tree
    far = T.box_region(P.max(0) + 10, P.max(0) + 11)
    same(capi.debug_overlap_walk(c.nodes, tris, [far], 8, wide=False), capi.debug_overlap(None, tris, [far], 8), "far")


@pytest.mark.parametrize("name", ["sah soup 0", "extreme soup 0"])
def test_coefficients_near_flt_max(name):
    """the exactness argument's overflow case: products and sums that overflow on the box's corner overflow on every corner inside the box, so the walk still
    equals the brute force"""
    c = _trees.case(name)
    tris = corpus_triangles(c)
    regions = corpus_regions(tris, 64, huge=True)
    assert np.isfinite(regions["planes"]).all() and np.abs(regions["planes"]).max() > 1e38
    want = capi.debug_overlap(None, tris, regions, 8)
    P = positions(tris).astype(f32)
    same(want, np_overlap(P, regions, 8), (name, "numpy"))
    with np.errstate(all="ignore"):
        s = np.concatenate([np_planes(g["planes"][:int(g["num_planes"])], P).ravel() for g in regions])
    assert np.isinf(s).any()                                                 # (the case does overflow)
    for wide in (False, True):
        if wide and not c.folds:
            continue
        same(capi.debug_overlap_walk(c.nodes, tris, regions, 8, wide=wide), want, (name, wide))
    assert (want[0]["count"] > 0).any() and (want[0]["count"] < len(tris)).any()


# ---- 3. select agrees with overlap

@pytest.mark.parametrize("name", ["cornell", "coverage"])
def test_select_agrees_with_overlap_region_by_region(rcases, name):
    case = rcases[name]
    tris = case.scene["triangles"]
    out, members = case.want(8)
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 7, len(tris)).astype(np.uint32)                    # object 7 has no triangle
    ids[:5] = 5
    for first in range(0, 64, 32):
        regions = case.regions[first:first + 32]
        touching, inside, ot, oi = capi.debug_select(None, tris, regions, ids, 8)
        for r in range(32):
            tb, ib = (touching >> r) & 1, (inside >> r) & 1
            assert tb.sum() == out["count"][first + r] and ib.sum() == out["inside"][first + r] and not (ib & ~tb).any()
            lowest = np.flatnonzero(tb)[:8]
            assert np.array_equal(lowest, members["primitive_id"][first + r][:len(lowest)]) and len(lowest) == out["stored"][first + r]
            assert np.array_equal(ib[lowest] != 0, (members["flags"][first + r][:len(lowest)] & INSIDE) != 0)
        for o in range(8):
            mine = ids == o
            assert ot[o] == np.bitwise_or.reduce(touching[mine], initial=0)
            assert oi[o] == (np.bitwise_and.reduce(inside[mine]) if mine.any() else 0)
        assert oi[7] == 0 and ot[7] == 0 and ot.any() and oi.any() and (oi != ot).any()
    t2, i2 = capi.debug_select(None, tris, case.regions[:1])
    assert np.array_equal(t2, capi.debug_select(None, tris, case.regions[:32])[0] & 1)
    with pytest.raises(capi.RtError, match="RT_SELECT_MAX_REGIONS"):
        capi.debug_select(None, tris, case.regions[:33])
    with pytest.raises(capi.RtError, match="not below num_objects"):
        capi.debug_select(None, tris, case.regions[:1], ids, 5)


# ---- 4. the planes of a pixel rectangle

def np_pixel_dir(cam, size, fx, fy):
    """the guide pass's direction through image position (fx, fy) in pixels (a centre: px + 0.5), float64"""
    th = np.tan(0.5 * float(cam["fov"]))
    x = (fx / size * 2 - 1) * th * float(cam["aspect_ratio"])
    y = (fy / size * 2 - 1) * th
    f = np.array([cam["front"][a] for a in "xyz"], np.float64)
    u = np.array([cam["up"][a] for a in "xyz"], np.float64)
    d = np.cross(f, u) * x + u * y + f
    return d / np.linalg.norm(d)


@pytest.mark.parametrize("rect", [(8, 8, 23, 23), (0, 0, 31, 31), (5, 9, 5, 9), (30, 0, 31, 7)])
def test_rect_region_holds_its_pixel_centres_and_none_just_outside(rect):
    x0, y0, x1, y1 = rect
    for cam in (T.default_camera(32, 32), look_camera((3.0, -2.0, 1.5), (-0.4, 1.0, -0.3))):
        g = capi.debug_rect_region(cam, 32, 32, x0, y0, x1, y1)
        assert g["num_planes"] == 4 and not g["planes"][4:].any()
        pos = np.array([cam["position"][a] for a in "xyz"], np.float64)
        s = lambda fx, fy: np_planes(g["planes"][:4], (pos + np_pixel_dir(cam, 32, fx, fy)).astype(f32))
        for y in range(y0 - 1, y1 + 2):
            for x in range(x0 - 1, x1 + 2):
                inside = x0 <= x <= x1 and y0 <= y <= y1
                v = s(x + 0.5, y + 0.5)
                assert (v <= 0).all() if inside else (v > 0).any(), (rect, x, y, v)
        near_far = capi.debug_rect_region(cam, 32, 32, x0, y0, x1, y1, 0.5, 7.0)
        assert near_far["num_planes"] == 6 and near_far["planes"][:4].tobytes() == g["planes"][:4].tobytes()
        f = np.array([cam["front"][a] for a in "xyz"], np.float64)
        for t, want in ((0.25, (True, False)), (0.75, (False, False)), (6.5, (False, False)), (7.5, (False, True))):
            v = np_planes(near_far["planes"][4:6], (pos + f * t).astype(f32))
            assert (v[0] > 0, v[1] > 0) == want, (t, v)
        assert capi.debug_rect_region(cam, 32, 32, x0, y0, x1, y1, 0.5)["num_planes"] == 5


# ---- 5. refusals and record sizes

def test_refusals_and_record_sizes(golden_scenes):
    assert T.region.itemsize == 144 and T.region_hits.itemsize == 16 and T.region_member.itemsize == 8 and capi.REGION_LIST_MAX == 8
    lib = capi.load()
    sc = golden_scenes["cornell"]
    tris, nodes = np.ascontiguousarray(sc["triangles"]), np.ascontiguousarray(sc["nodes"])
    rg = np.array([T.box_region((-1, -1, -1), (1, 1, 1))] * 4, T.region)
    out, members = np.zeros(4, T.region_hits), np.zeros((4, 8), T.region_member)
    p = lambda a: a.ctypes.data

    def refused(rc, text):
        assert rc != 0 and text in lib.rt_last_error(None).decode(), (rc, lib.rt_last_error(None).decode())

    refused(lib.rt_scene_overlap(None, p(rg), 4, 8, p(out), p(members)), "ctx is NULL")
    refused(lib.rt_scene_overlap_buffer(None, None, 4, 8, None, None), "ctx is NULL")
    refused(lib.rt_scene_select(None, p(rg), 4, None, None, None, None), "ctx is NULL")
    refused(lib.rt_scene_select_buffer(None, None, 4, None, None, None, None), "ctx is NULL")
    refused(lib.rt_frame_pick_rect(None, 0, 0, 1, 1, 0.0, 1.0, None, None, None, None, None), "frame is NULL")
    for call, tail in ((lambda *a: lib.rt_debug_overlap(None, p(tris), len(tris), *a), ()),
                       (lambda *a: lib.rt_debug_overlap_walk(p(nodes), len(nodes), p(tris), len(tris), 1, *a), (None,))):
        refused(call(None, 4, 8, p(out), p(members), *tail), "NULL argument")
        refused(call(p(rg), 4, 8, None, p(members), *tail), "NULL argument")
        refused(call(p(rg), 4, 8, p(out), None, *tail), "NULL argument")
        refused(call(p(rg), 4, 9, p(out), p(members), *tail), "RT_REGION_LIST_MAX")
        assert call(None, 0, 0, None, None, *tail) == 0                                     # n == 0: RT_OK, nothing done
    refused(lib.rt_debug_overlap_walk(None, len(nodes), p(tris), len(tris), 1, p(rg), 4, 8, p(out), p(members), None), "NULL argument")
    refused(lib.rt_debug_overlap_walk(p(nodes), len(nodes), p(tris), len(tris), 2, p(rg), 4, 8, p(out), p(members), None), "wide must be")
    refused(lib.rt_debug_overlap_walk(p(nodes), len(nodes), p(tris), len(tris) - 1, 0, p(rg), 4, 8, p(out), p(members), None), "outside the array")
    cam, g = np.array([T.default_camera(32, 32)]), np.zeros(1, T.region)
    refused(lib.rt_debug_rect_region(None, 32, 32, 0, 0, 1, 1, 0.0, 1.0, p(g)), "NULL argument")
    refused(lib.rt_debug_rect_region(p(cam), 32, 32, 2, 0, 1, 1, 0.0, 1.0, p(g)), "x1 < x0")
    refused(lib.rt_debug_rect_region(p(cam), 32, 32, 0, 3, 1, 2, 0.0, 1.0, p(g)), "y1 < y0")
    refused(lib.rt_debug_rect_region(p(cam), 32, 32, 0, 0, 32, 1, 0.0, 1.0, p(g)), "outside the image")
    assert out.tobytes() == bytes(out.nbytes) and members.tobytes() == bytes(members.nbytes) and g.tobytes() == bytes(144)      # nothing was written
    assert lib.rt_debug_overlap(None, p(tris), len(tris), p(rg), 4, 0, p(out), None) == 0               # max_list == 0: members may be NULL
    assert (out["flags"] == SEARCHED).all()


def test_region_helpers():
    g = T.box_region((0, 1, 2), (3, 4, 5))
    assert g["num_planes"] == 6
    pts = np.array([[0, 1, 2], [3, 4, 5], [1.5, 2, 3], [-0.1, 2, 3], [1, 4.1, 3], [1, 2, 5.5]], f32)
    s = np_planes(g["planes"][:6], pts)
    assert np.array_equal((s > 0).any(1), [False, False, False, True, True, True])
    m = np.concatenate([rotation((0, 0, 1), np.pi / 4) * 2.0, np.array([[10.0], [0.0], [0.0]])], 1)
    o = T.oriented_box_region(m, (1.0, 0.5, 0.25))                           # half extents in the matrix's frame: 2, 1 and 0.5 in the world
    inside = np.array([[10, 0, 0], [10 + 1.3, 1.3, 0], [10, 0, 0.49]], f32)
    outside = np.array([[10 + 1.5, 1.5, 0], [10 - 0.8, 0.8, 0], [10, 0, 0.51]], f32)
    assert not (np_planes(o["planes"][:6], inside) > 0).any() and (np_planes(o["planes"][:6], outside) > 0).any(1).all()
