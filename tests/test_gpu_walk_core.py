"""-m gpu: the pieces k_query_trace, k_bake, k_nearest, k_within and k_region share (raytracing_amd/csrc/walk_kernels.h) where no other test names them: a traversal stack that
runs past its RT_QUERY_STACK_LDS = 12 entries in LDS into the spill area, lanes alone and in partial waves, and the persistent grid's stride.

The scene is a slab stack: N = 16384 unit quads (32768 triangles) at z = 0, 1, ..., N - 1, corners at integer coordinates, normals along -z, built by the
host builder.  Its tree is a perfect binary tree over the quads, 14 interior levels deep, so a walk that descends to one quad leaves one pending child per
level: the Python restatements below (the child-pair ray walk: near child first, the far child pushed when both boxes are hit; the nearest walk: both
children pass while `best` is infinite) measure a pending depth of 14 = RT_QUERY_STACK_LDS + 2 for every ray and every point used here, and the tests
refuse to run on less.  N is the smallest power of two that reaches it (N = 8192 gives 13).

  rays     from (0.3, 0.6, -1) along +z; even rays are exactly axis-parallel with their origins shifted sideways (1/dir is not finite: the child-pair walk
           with the select-form box test), odd rays are tilted by i * 2^-24 in x and y (the 4-wide walk when the scene has 4-wide trees)
  nearest  points beside the stack at x = 3 + i / 256, spread over its height, no distance limit
  within   the nearest walk's points with max_distance = inf: every box passes, so the counting walk (it visits every passing child, pushes the rest and
           never lowers its bound) leaves one pending child per pair level -- the restatement below measures 14; max_near 0 and 8, and k_nearest at 8
  overlap  even regions are one box that encloses the whole stack (every box passes: the same 14), odd regions are slabs that cut the stack at varying
           heights, for verdicts of both kinds; max_list 0 and 8
  bake     even points lie on the first quad with normal (0, 0, -1); the bias is -(N / 2 + 0.5), which puts their origins between two quads in the middle of
           the stack, looking down through N / 2 back faces: a long walk whose every triangle is culled (all unoccluded).  Odd points are this test's own
           addition for verdicts of both kinds: normal (0, 0, +1), placed so that the same bias puts their origins at z = -1 below the first quad.

Everything is compared byte for byte: Context.trace with the oracle as tests/test_gpu_query.py obtains it, Context.nearest with the host's brute force,
Context.within and Context.overlap with the host's brute force, Context.bake with the host's rays, the oracle's verdicts of them and the host's reduction as tests/test_gpu_bake.py does.  After every call rt_finish
succeeds: no walk raised the stack's status word.  One process, each GPU step once, nothing retried; nothing here provokes a fault."""
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests import _oracle
from tests.test_wide_bvh import wide_of
from tests.test_gpu_query import context, expected, check_closest

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 0xFFFFFFFF
N_QUADS = 16384
STACK_LDS = 12                         # RT_QUERY_STACK_LDS (walk_kernels.h)
COUNTS = [1, 63, 64, 65, 130]          # a lone lane, a partial wave, a full wave, a second chunk with one lane, two chunks and a partial third
DISTINCT = 130
WITHIN_CASES = [(0, False), (8, False), (8, True)]          # (max_near, k_nearest)
BAKE_BIAS = -(N_QUADS / 2 + 0.5)
BAKE_RADIUS = float(N_QUADS)


def slab_stack(n_quads):
    quad = S.quad((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), normal=np.array([0, 0, -1], f32))      # wound so that its front faces -z
    P, Nn, U = (np.tile(a, (n_quads, 1, 1)) for a in quad)
    P[:, :, 2] = np.repeat(np.arange(n_quads, dtype=f32), 2)[:, None]
    scene = host.Scene(arrays=dict(triangles=S.to_triangles([(P, Nn, U, 0)]), materials=np.array([S.make_material()])))
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    scene.build_bvh()
    scene.finalize()
    return {k: np.array(v) for k, v in scene.arrays().items() if k != "flags"}


def corners(tris):
    return np.stack([np.stack([tris[v]["position"][k] for k in "xyz"], -1) for v in ("v1", "v2", "v3")], 1).astype(np.float64)


def ray_pending_depth(nodes, tris, o, d, t_max):
    """the deepest the child-pair walk's stack gets for one ray: trace_bvh.cl's loop, near child first by the split axis, the far child pushed when both
    boxes are hit, a pop re-tested against the current t_max (float64: every coordinate of this scene is exact)"""
    lo = np.stack([nodes["bounds_min"][k] for k in "xyz"], -1).astype(np.float64)
    hi = np.stack([nodes["bounds_max"][k] for k in "xyz"], -1).astype(np.float64)
    P = corners(tris)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d

    def box(i):
        with np.errstate(invalid="ignore"):
            t0, t1 = (lo[i] - o) * inv, (hi[i] - o) * inv
        near, far = np.fmax.reduce(np.minimum(t0, t1)), np.fmin.reduce(np.maximum(t0, t1))
        entry = max(near, 0.0)
        return entry <= min(far, t_max), entry

    stack, deepest, node = [], 0, 0
    while node is not None:
        count = int(nodes["num_primitives_axis"][node]) >> 16
        if count:
            for t in range(int(nodes["offset"][node]), int(nodes["offset"][node]) + count):
                e1, e2 = P[t, 1] - P[t, 0], P[t, 2] - P[t, 0]
                pv = np.cross(d, e2)
                det = e1 @ pv
                if det < 1e-8:
                    continue
                tv = o - P[t, 0]
                u, qv = (tv @ pv) / det, np.cross(tv, e1)
                v, dist = (d @ qv) / det, (e2 @ qv) / det
                if u >= 0 and v >= 0 and u + v <= 1 and 0.0 <= dist <= t_max:
                    t_max = dist
            node = None
        else:
            axis = int(nodes["num_primitives_axis"][node]) & 0xFFFF
            c = (node + 1, int(nodes["offset"][node]))
            if d[axis] < 0:
                c = c[::-1]
            (h0, _), (h1, e1_) = box(c[0]), box(c[1])
            if h0 and h1:
                stack.append((c[1], e1_))
                deepest = max(deepest, len(stack))
            node = c[0] if h0 else c[1] if h1 else None
        while node is None and stack:
            cand, entry = stack.pop()
            if t_max >= entry:
                node = cand
    return deepest


def nearest_pending_depth(nodes, tris, p):
    """the same for the nearest walk: a child passes when !(box d2 > best), the nearer is visited, the other pushed; best is infinite until the first leaf"""
    lo = np.stack([nodes["bounds_min"][k] for k in "xyz"], -1).astype(np.float64)
    hi = np.stack([nodes["bounds_max"][k] for k in "xyz"], -1).astype(np.float64)
    d2 = lambda i: float((np.maximum(np.maximum(lo[i] - p, p - hi[i]), 0.0) ** 2).sum())
    best, stack, deepest, node = np.inf, [], 0, 0
    while node is not None:
        count = int(nodes["num_primitives_axis"][node]) >> 16
        if count:
            first = int(nodes["offset"][node])
            found = capi.debug_nearest(None, tris[first:first + count], np.asarray(p, f32)[None])
            best = min(best, float(found["distance"][0]) ** 2)
            node = None
        else:
            c = sorted(((d2(i), i) for i in (node + 1, int(nodes["offset"][node]))))
            c = [(e, i) for e, i in c if not e > best]
            if len(c) == 2:
                stack.append(c[1])
                deepest = max(deepest, len(stack))
            node = c[0][1] if c else None
        while node is None and stack:
            entry, cand = stack.pop()
            if not entry > best:
                node = cand
    return deepest


def node_boxes(nodes):
    return (np.stack([nodes[b][k] for k in "xyz"], -1).astype(np.float64) for b in ("bounds_min", "bounds_max"))


def counting_pending_depth(nodes, passes):
    """the same for a counting walk (k_within without k_nearest, k_region) on the child-pair tree: passes[i] = node i's box passes; every passing child is
    visited, the first next, the other pushed; the bound is never lowered, so a pop always accepts"""
    stack, deepest, node = [], 0, 0 if passes[0] else None
    while node is not None:
        c = []
        if not int(nodes["num_primitives_axis"][node]) >> 16:
            c = [i for i in (node + 1, int(nodes["offset"][node])) if passes[i]]
        if len(c) == 2:
            stack.append(c[1])
            deepest = max(deepest, len(stack))
        node = c[0] if c else stack.pop() if stack else None
    return deepest


class Slab:
    """the scene, the 130 distinct rays and points, the precondition and every expected answer (computed once, shared, never changed)"""

    def __init__(self):
        self.scene = slab_stack(N_QUADS)
        nodes, tris = self.scene["nodes"], self.scene["triangles"]
        i = np.arange(DISTINCT)
        even = i % 2 == 0
        rays = np.zeros(DISTINCT, T.ray)
        shift, tilt = (i / 1024.0).astype(f32), (i * 2.0 ** -24).astype(f32)
        rays["origin"]["x"], rays["origin"]["y"], rays["origin"]["z"] = np.where(even, f32(0.3) + shift, f32(0.3)), np.where(even, f32(0.6) + shift, f32(0.6)), -1.0
        rays["direction"]["x"] = rays["direction"]["y"] = np.where(even, f32(0.0), tilt)
        rays["direction"]["z"], rays["direction"]["w"] = 1.0, 2.0 * N_QUADS
        self.rays = rays
        self.points = np.stack([3.0 + i / 256.0, np.full(DISTINCT, 0.5), (i * 127 % N_QUADS) + 0.25, np.full(DISTINCT, np.inf)], -1).astype(f32)
        bake = np.zeros((DISTINCT, 8), f32)
        bake[:, 0], bake[:, 1] = 0.25 + i / 512.0, 0.5 + i / 1024.0
        bake[:, 2], bake[:, 6] = np.where(even, 0.0, -1.0 - BAKE_BIAS), np.where(even, -1.0, 1.0)
        self.bake_points = bake

        # non-vacuity, before any device call: the stack of every walk below runs past its entries in LDS
        comp = lambda r, part: np.array([r[part][k] for k in "xyz"], np.float64)
        self.ray_depth = min(ray_pending_depth(nodes, tris, comp(r, "origin"), comp(r, "direction"), float(r["direction"]["w"])) for r in rays)
        self.point_depth = min(nearest_pending_depth(nodes, tris, p[:3].astype(np.float64)) for p in self.points)
        assert self.ray_depth >= STACK_LDS + 2, "the rays' pending depth is %d, below %d: the spill area is not reached" % (self.ray_depth, STACK_LDS + 2)
        assert self.point_depth >= STACK_LDS + 2, "the points' pending depth is %d, below %d: the spill area is not reached" % (self.point_depth, STACK_LDS + 2)

        # within and overlap: a counting walk's pending depth depends on which boxes pass alone.  With an infinite radius every box passes for every point,
        # and the enclosing box's planes reject none: one restatement of the walk speaks for all of them
        lo, hi = node_boxes(nodes)
        gap = np.maximum(np.maximum(lo[:, None] - self.points[None, :, :3], self.points[None, :, :3] - hi[:, None]), 0.0)
        point_passes = ~((gap ** 2).sum(-1) > np.float64(self.points[:, 3])[None])                 # [node, point]: !(nearest_box_d2 > r2)
        assert point_passes.all()
        self.within_depth = counting_pending_depth(nodes, point_passes.all(1))
        assert self.within_depth >= STACK_LDS + 2, "the within points' pending depth is %d, below %d" % (self.within_depth, STACK_LDS + 2)
        enclosing = T.box_region((-1.0, -1.0, -1.0), (2.0, 2.0, float(N_QUADS)))
        regions = np.zeros(DISTINCT, T.region)
        regions[0::2] = enclosing
        for k in range(1, DISTINCT, 2):                                            # below a plane between two quads; every other one tilted through a quad
            regions[k] = T.planes_region([(0.25 * (k % 4 == 1), 0.0, 1.0, -(k * 119 % N_QUADS + 0.125))])
        self.regions = regions
        pl = np.float64(enclosing["planes"][:int(enclosing["num_planes"])])
        corner = np.where(pl[None, :, :3] >= 0.0, lo[:, None], hi[:, None])                        # region.h's box test: the corner lowest along the normal
        box_passes = ~((corner * pl[None, :, :3]).sum(-1) + pl[None, :, 3] > 0.0).any(1)
        assert box_passes.all()
        self.region_depth = counting_pending_depth(nodes, box_passes)
        assert self.region_depth >= STACK_LDS + 2, "the enclosing regions' pending depth is %d, below %d" % (self.region_depth, STACK_LDS + 2)
        self.within = {(m, knn): capi.debug_within(None, tris, self.points, m, k_nearest=knn) for m, knn in WITHIN_CASES}
        self.overlap = {m: capi.debug_overlap(None, tris, regions, m) for m in (0, 8)}
        assert all((got[0]["stored"] == m).any() for (m, _), got in self.within.items())           # a full list
        counts = self.overlap[8][0]["count"]
        assert (counts[0::2] == len(tris)).all() and ((counts[1::2] > 0) & (counts[1::2] < len(tris))).all() and len(set(counts[1::2].tolist())) > 1
        assert (self.overlap[8][0]["stored"] == 8).any()

        self.orc = _oracle.Oracle(16, 16, self.scene)
        self.wide, self.entry = wide_of(nodes, 1)
        self.hits, self.occluded, skipped = expected(self.orc, self.wide, self.entry, rays)
        assert not skipped.any() and (self.hits["primitive_id"] != INVALID).all() and self.occluded.all()
        self.nearest = capi.debug_nearest(None, tris, self.points)
        assert (self.nearest["primitive_id"] != INVALID).all()
        self.baked = {samples: self.bake_expected(bake, samples) for samples in (16, 64)}

    def bake_expected(self, points, samples, first_index=0):
        rays = capi.debug_bake_rays(None, points, samples, 5, BAKE_BIAS, BAKE_RADIUS, first_index=first_index)
        occ = (self.orc.wide_trace(self.wide, self.entry, rays.reshape(-1), True) != INVALID).astype(np.uint32)
        return capi.debug_bake_reduce(rays, occ.reshape(rays.shape), samples)


@pytest.fixture(scope="module")
def slab():
    return Slab()


@pytest.fixture(params=[1, 0], ids=["wide_trees", "wide_trees_off"])
def ctx(request, slab):
    c = context(wide=request.param)
    try:
        c.upload_scene(slab.scene)
        yield c
    finally:
        c.close()


def same_bake(got, want, what):
    assert np.array_equal(got["unoccluded"], want["unoccluded"]), (what, got["unoccluded"][:8], want["unoccluded"][:8])
    assert got["bent_normal"].tobytes() == want["bent_normal"].tobytes(), what


def test_rays_spill_and_equal_the_oracle(slab, ctx):
    for n in COUNTS:
        got = ctx.trace(slab.rays[:n])
        ctx.finish()
        check_closest(got, slab.hits[:n], n)
        assert got.tobytes() == slab.hits[:n].tobytes(), n                 # every ray hits: the whole record is specified
        occ = ctx.trace(slab.rays[:n], any_hit=True)
        ctx.finish()
        assert occ.tobytes() == slab.occluded[:n].tobytes(), n


def test_points_spill_and_equal_brute_force(slab, ctx):
    for n in COUNTS:
        got = ctx.nearest(slab.points[:n])
        ctx.finish()
        assert got.tobytes() == slab.nearest[:n].tobytes(), (n, int((got["primitive_id"] != slab.nearest["primitive_id"][:n]).sum()))


def test_within_spills_and_equals_brute_force(slab, ctx):
    for max_near, knn in WITHIN_CASES:
        want, want_near = slab.within[(max_near, knn)]
        for n in COUNTS:
            got = ctx.within(slab.points[:n], max_near, k_nearest=knn)
            ctx.finish()
            got, near = got if max_near else (got, want_near[:n])
            assert got.tobytes() == want[:n].tobytes(), (max_near, knn, n, got["count"][:4], want["count"][:4])
            assert near.tobytes() == want_near[:n].tobytes(), (max_near, knn, n)


def test_overlaps_spill_and_equal_brute_force(slab, ctx):
    for max_list in (0, 8):
        want, want_members = slab.overlap[max_list]
        for n in COUNTS:
            got = ctx.overlap(slab.regions[:n], max_list)
            ctx.finish()
            got, members = got if max_list else (got, want_members[:n])
            assert got.tobytes() == want[:n].tobytes(), (max_list, n, got["count"][:4], want["count"][:4])
            assert members.tobytes() == want_members[:n].tobytes(), (max_list, n)


@pytest.mark.parametrize("samples", [16, 64])
def test_bakes_equal_reduced_oracle_verdicts(slab, ctx, samples):
    want = slab.baked[samples]
    assert (want["unoccluded"][0::2] == samples).all()                         # through back faces only
    assert ((want["unoccluded"][1::2] > 0) & (want["unoccluded"][1::2] < samples)).any()
    for n in COUNTS:
        got = ctx.bake(slab.bake_points[:n], samples, seed=5, bias=BAKE_BIAS, radius=BAKE_RADIUS)
        ctx.finish()
        same_bake(got, want[:n], (samples, n))


def test_the_strided_grid(slab, ctx):
    """more chunks than resident blocks: every block takes a second chunk (rays, points), a second group (bake)"""
    cus = ctx.device_info()[1]
    round_up_8 = lambda v: (v + 7) & ~7
    n = (round_up_8(cus * 24) + 1) * 64 + 1
    tile = lambda a: np.resize(a, n)
    got = ctx.trace(tile(slab.rays))
    ctx.finish()
    assert got.tobytes() == tile(slab.hits).tobytes()
    occ = ctx.trace(tile(slab.rays), any_hit=True)
    ctx.finish()
    assert occ.tobytes() == tile(slab.occluded).tobytes()
    near = ctx.nearest(np.resize(slab.points, (n, 4)))
    ctx.finish()
    assert near.tobytes() == tile(slab.nearest).tobytes()
    # a point's index enters its rays, so tiling does not give the expected bake: one launch against launches of 1024 points instead (anchored by the 130
    # points compared with the oracle above)
    m = round_up_8(cus * 20) + 2
    pts = np.resize(slab.bake_points, (m, 8))
    whole = ctx.bake(pts, 64, seed=5, bias=BAKE_BIAS, radius=BAKE_RADIUS)
    ctx.finish()
    same_bake(whole[:DISTINCT], slab.baked[64], "the first 130 of one launch")
    ctx.set_bake_chunk_points(1024)
    chunked = ctx.bake(pts, 64, seed=5, bias=BAKE_BIAS, radius=BAKE_RADIUS)
    ctx.finish()
    assert chunked.tobytes() == whole.tobytes()
