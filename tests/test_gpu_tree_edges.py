"""-m gpu: the device's tree kernels (fold_kernels.h, ploc_kernels.h, the refit kernels of refit.hip; driven by device_fold.hip) on the corpus of tests/_trees.py --
trees of 2 .. 1025 leaves around the kernels' block sizes (the scan's 1024, k_fold_emit's 64, k_ploc_*'s 256), chains under and over the stack bound, identical
and zero-extent boxes (every cost and every Morton code a tie), clusters 1e7 apart, soups with coincident triangles -- against the host's restatements, which
tests/test_tree_corpus.py and the CPU suite check on the same inputs.  Every comparison is byte for byte; where the host refuses a tree the device must refuse
it, and where the host folds it the device must fold it.  Nothing here provokes a fault: every input is a valid tree."""
import re
import numpy as np
import pytest
from tests import _oracle, _trees
from tests.test_wide_bvh import WIDE, check, wide_of, _rays_for
from tests.test_own_tree import check_own_structure, shadow_and_closest_on, shadow_soup_arrays, wide_metric, light_dir
from tests.test_refit import jitter, moved, positions, same_nodes, same_records
from tests.test_gpu_device_fold import same
from tests.test_gpu_fuzz import random_scene
from raytracing_amd import capi, host, scenes as S, types as T

pytestmark = pytest.mark.gpu
D = light_dir()
ALL = _trees.names()                                             # (names only: a case is made when its test asks for it)
TREES = _trees.names(leaf_roots=False)
BUILT = _trees.names("built")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def attempt(fn):
    """fn()'s result, or None where the library refuses"""
    try:
        return fn()
    except capi.RtError:
        return None


def same_bytes(dev, hst):
    """(records, entry) of the device against the host's"""
    assert dev[1] == hst[1] and len(dev[0]) == len(hst[0]), (dev[1], hst[1], len(dev[0]), len(hst[0]))
    a, b = np.ascontiguousarray(dev[0]).view(np.uint8).reshape(-1, 64), np.ascontiguousarray(hst[0]).view(np.uint8).reshape(-1, 64)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, "first differing record %d of %d: device %r host %r" % (bad[0], len(a), a[bad[0]].view(WIDE), b[bad[0]].view(WIDE))


def both_or_neither(dev, hst, what):
    assert (dev is None) == (hst is None), "%s: the device %s, the host %s" % (what, "refuses" if dev is None else "folds", "refuses" if hst is None else "folds")
    return dev is not None


# ---- the fold -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_the_fold_by_surface_area(ctx, name):
    c = _trees.case(name)
    hst = attempt(lambda: wide_of(c.nodes, 1, with_roots=True))
    assert (hst is not None) == c.folds
    dev = attempt(lambda: capi.device_fold(ctx, c.nodes))
    if both_or_neither(dev, hst, name):
        same(dev[:3], hst)
        check(c.nodes, fold=(dev[0].view(WIDE).reshape(-1), dev[1], dev[2]))


@pytest.mark.parametrize("name", ALL)
def test_the_fold_by_the_own_trees_metric(ctx, name):
    c = _trees.case(name)
    hst = attempt(lambda: wide_metric(c.nodes, 0.5, [D]))
    dev = attempt(lambda: capi.device_fold(ctx, c.nodes, 0.5, [np.abs(D)]))
    if both_or_neither(dev, hst, name):
        same_bytes(dev[:2], hst)


def weights_of(kind, n, rng):
    if kind == "random":
        return rng.integers(0, 50, n).astype(np.float64) + rng.random(n) * 0.01
    if kind == "zero":                                         # every comparison of the dynamic programme a tie
        return np.zeros(n)
    return 10.0 ** rng.uniform(-30, 30, n)


@pytest.mark.parametrize("name", ALL)
def test_the_fold_by_per_node_weights(ctx, name):
    c = _trees.case(name)
    rng = np.random.default_rng(len(c.nodes))
    for kind in ("random", "zero", "span"):
        w = weights_of(kind, len(c.nodes), rng)
        hst = attempt(lambda: capi.wide_bvh_weights(c.nodes, w))
        dev = attempt(lambda: capi.device_fold(ctx, c.nodes, weights=w))
        # (the frame's limits aside, depth under these weights decides: the restated rule says which way)
        assert (hst is not None) == _trees.expected_to_fold(c.nodes, w), (name, kind)
        if both_or_neither(dev, hst, "%s, %s weights" % (name, kind)):
            same(dev[:3], hst)


# ---- the tree builder ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TREES)
def test_the_tree_built_on_the_device(ctx, name):
    c = _trees.case(name)
    own, _, rounds = capi.device_tree(ctx, c.nodes, 0.5, [D])
    check_own_structure(c.nodes, own)
    again, _, _ = capi.device_tree(ctx, c.nodes, 0.5, [D])
    assert own.tobytes() == again.tobytes()                    # no choice depends on which thread arrives first
    n_leaves = int(_trees.is_leaf(c.nodes).sum())
    assert 1 <= rounds <= n_leaves - 1, (rounds, n_leaves)     # every round merges at least the cheapest pair
    hst = attempt(lambda: wide_metric(own, 0.5, [D]))
    dev = attempt(lambda: capi.device_fold(ctx, own, 0.5, [np.abs(D)]))
    folds = both_or_neither(dev, hst, name)
    if folds:
        same_bytes(dev[:2], hst)
    if name.startswith("pow2"):
        # one merge a round: a tree as deep as it has leaves, refused by both sides -- and for its depth, where the leaves are within the frame's reach
        assert not folds and rounds == n_leaves - 1
        levels = _trees.record_levels(own, _trees.metric_weights(own, 0.5, [D]))
        assert levels > _trees.MAX_LEVELS, levels
        assert _trees.frame_ok(own) == (name.startswith("pow2 near"))


@pytest.mark.parametrize("seed", range(6))
def test_shadow_verdicts_on_the_device_built_tree_of_a_soup(ctx, env_map, seed):
    """tests/test_own_tree.py's soups: k_trace_w4's walk (restated on the CPU) over the fold of the tree built on the device gives the reference's verdicts"""
    arrays = shadow_soup_arrays(seed, env_map)
    own, _, _ = capi.device_tree(ctx, arrays["nodes"], 0.5, [D])
    check_own_structure(arrays["nodes"], own)
    shadow_and_closest_on(arrays, {"device": wide_metric(own, 0.5, [D])}, 32, 24, 3)     # asserts equal shadow verdicts at every bounce


# ---- the refit ----------------------------------------------------------------------------------------------------------------------------------------------------
def poses_of(tris, rng):
    P = positions(tris)
    far = P.copy()
    far[0, 0, 0] = np.float32(3e8)                             # beyond 2^28: the records above that vertex no longer qualify
    return {"unmoved": tris, "jitter": jitter(tris, rng), "one point": moved(tris, np.broadcast_to(P[0, 0], P.shape).copy()),
            "shifted by 1e7": moved(tris, (P.astype(np.float64) + 1e7).astype(np.float32)), "a vertex at 3e8": moved(tris, far)}


@pytest.mark.parametrize("name", BUILT)
def test_the_refit_on_the_device_equals_the_host_restatement(ctx, name):
    c = _trees.case(name)
    rng = np.random.default_rng(len(c.tris))
    folds = [f for f in (attempt(lambda: wide_of(c.nodes, 1)), attempt(lambda: wide_of(c.nodes, 2))) if f is not None]
    assert folds
    for pose_name, pose in poses_of(c.tris, rng).items():
        for rec, entry in folds:
            hst = attempt(lambda: capi.debug_refit(None, c.nodes, pose, rec, entry))
            dev = attempt(lambda: capi.debug_refit(ctx, c.nodes, pose, rec, entry))
            assert (dev is None) == (hst is None), (name, pose_name)
            if hst is None:
                continue
            same_nodes(dev[0], hst[0])
            assert dev[2] == hst[2], (name, pose_name, "the disqualified flag", dev[2], hst[2])
            assert (dev[1] is None) == (hst[1] is None)
            if hst[1] is not None:
                same_records(dev[1], hst[1])
                if pose_name == "a vertex at 3e8":
                    assert hst[2] and dev[2]                  # the root record holds that vertex


# ---- the adaptation's crossing counts -----------------------------------------------------------------------------------------------------------------------------
def rays_of(nodes, rng, n=240):
    rays = _rays_for(nodes, rng, n)
    o = np.array([r[0] for r in rays], np.float64)
    d = np.array([r[1] for r in rays], np.float64)
    for i in range(0, n, 5):                                   # along an axis: two direction components zero, 1 / d infinite, 0 * inf in the slab test
        d[i] = np.eye(3)[i % 3] * (1.0 if i % 2 else -1.0)
    o4 = np.concatenate([o, np.full((n, 1), 1e30)], 1).astype(np.float32)
    o4[::7, 3] = np.float32(np.linalg.norm(_trees.extents(nodes)[0]) * 0.5)      # some rays end inside the scene
    return o4, np.concatenate([d, np.zeros((n, 1))], 1).astype(np.float32)


@pytest.mark.parametrize("name", ALL)
def test_crossing_counts_on_the_device_equal_the_hosts(ctx, name):
    c = _trees.case(name)
    o, d = rays_of(c.nodes, np.random.default_rng(len(c.nodes)))
    hst, hst_cut = capi.count_box_passes(None, c.nodes, o, d)
    dev, dev_cut = capi.count_box_passes(ctx, c.nodes, o, d)
    assert hst[0] > 0                                          # rays do pass the root
    assert np.array_equal(dev, hst), np.nonzero(dev != hst)[0][:8]
    assert dev_cut == hst_cut, (dev_cut, hst_cut)
    # the contract (include/rt_hip.h): more than 61 pending nodes cut a walk short.  A left-deep chain leaves one leaf pending per level, a right-deep one none
    if name in ("identical, left 81", "identical, left 121"):         # interior node k is node k, met with k leaves pending: node 62 is counted and not opened
        assert hst_cut == hst[0] and hst[62] == hst[0] and (hst[63:len(c.nodes) // 2] == 0).all()
    if name in ("identical, right 81", "identical, right 121", "identical, left 21"):
        assert hst_cut == 0 and (hst == hst[0]).all()


# ---- through rt_scene_upload --------------------------------------------------------------------------------------------------------------------------------------
def finished(tris, mats, env_map, directional=True):
    s = host.Scene(arrays=dict(triangles=tris, materials=mats))
    if directional:
        s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    s.build_bvh()
    s.set_env_image(env_map)
    s.finalize()
    return s.arrays()


def small_triangles(centres, size):
    """one triangle per centre, `size` (a number, or one per centre) across"""
    n = len(centres)
    corners = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]])
    P = np.asarray(centres, np.float64)[:, None, :] + np.broadcast_to(np.asarray(size, np.float64), (n,))[:, None, None] * corners
    N = np.tile(np.array([0, 0, 1], np.float32), (n, 3, 1))
    return S.to_triangles([(P.astype(np.float32), N, np.zeros((n, 3, 2), np.float32), 0)])


def upload_scene_of(which, env_map):
    if isinstance(which, int):
        return random_scene(np.random.default_rng(1000 + which), env_map)
    mats = np.array([S.make_material(kd=(0.7, 0.6, 0.5), ks=(0.2, 0.2, 0.2), roughness=0.4)], dtype=T.packed_material)
    if which.startswith("triangles at 2^k"):
        # 200 triangles at 2^k * (1, 1, 0.5), each 2^k / 2 across: k = -126 .. 27 is every normal binary32 power of two the records' frame takes (coordinates below
        # 2^28), the uppermost 46 twice.  Every triangle is nearer to all below it than to the next above, so whoever clusters these leaves bottom-up gets a chain
        # (PLOC: one merge a round), 50 or more record levels deep at three nodes a record -- over the 33 the walk's stack holds.  The builder the reference's tree
        # comes from makes the same chain, and no scene with such a tree gets 4-wide records at all; so the reference's tree is a balanced one here (any tree with
        # exact boxes over the triangles in their order is a valid scene, and the oracle walks the same one): it folds, and the shadow rays' own tree is attempted.
        k = np.concatenate([np.arange(-126, 28), np.arange(-18, 28)])
        sc = finished(small_triangles(np.ldexp(1.0, k)[:, None] * [1.0, 1.0, 0.5], np.ldexp(0.5, k)), mats, env_map)
        P = positions(sc["triangles"])
        sc["nodes"] = _trees.synthesise(np.stack([P.min(axis=1), P.max(axis=1)], 1), "balanced")
        return sc
    if which == "coincident triangles":
        return finished(small_triangles(np.tile([[0.0, 1.0, 0.5]], (64, 1)), 0.8), mats, env_map)
    quad = S.to_triangles([S.quad((-1, 0, 0), (1, 0, 0), (1, 2, 0), (-1, 2, 0)) + (0,)])
    assert len(quad) == 2
    return finished(quad, mats, env_map)


def shadow_metric_of(lights):
    """wide_bvh.cpp's shadow_metric(lights, 0.5) as rt_debug_device_tree takes a metric: (iso, directions)"""
    dirs, iso = [], 0.0
    for l in lights:
        v = np.array([l["origin"][c] for c in "xyz"], np.float64)
        if int(l["type"]) == 0 or not np.linalg.norm(v) > 0.0:
            iso += 1.0
        else:
            dirs.append(np.abs(v / np.linalg.norm(v)))
    return (iso + 0.5 * len(dirs), dirs) if dirs else (1.0, None)


UPLOADS = list(range(8)) + ["triangles at 2^k", "triangles at 2^k, either builder", "coincident triangles", "a quad"]


def records_in(fold):
    return 0 if fold is None else len(fold[0])


@pytest.mark.parametrize("which", UPLOADS)
def test_an_uploaded_scene_renders_the_oracles_bits(ctx, env_map, which):
    """device fold on, device builder forced (or, "either builder", both started), own shadow tree forced, adaptive fold 31"""
    w, h, bounces, spp = 32, 24, 3, 2
    sc = upload_scene_of(which, env_map)
    cam = T.default_camera(w, h)
    c = capi.Context(0)
    try:
        for opt, value in ((7, 1), (9, 2 if str(which).endswith("either builder") else 1), (2, 2), (4, 31)):
            assert c.lib.rt_ctx_set_option(c.handle, opt, value) == 0
        c.upload_scene(sc)                                     # must not fail, whatever falls back
        report = c.tree_report()
        fr = capi.Frame(c, w, h)
        fr.set_camera(cam); fr.set_max_bounces(bounces)
        fr.integrate(spp)
        got, st = fr.radiance()[..., :3].copy(), fr.stats()
        fr.close()
    finally:
        c.close()
    orc = _oracle.Oracle(w, h, sc)
    orc.set_camera(cam); orc.set_max_bounces(bounces); orc.integrate(spp)
    assert np.array_equal(got, orc.radiance()[..., :3], equal_nan=True)
    assert (st.closest_rays, st.shadow_rays) == orc.ray_totals()
    # who folded the reference's tree, who built the shadow rays': the report says, and a fall-back to the host is one the debug entries make too
    nodes = sc["nodes"]
    folded = re.search(r"fold of the reference's tree [0-9.]+ \((on the device|on host threads)\)", report)
    assert folded, report
    ref_fold = attempt(lambda: capi.device_fold(ctx, nodes))
    assert (folded.group(1) == "on the device") == (ref_fold is not None), report
    assert "shadow tree: built on" in report, report
    if not any(records_in(f) for f in (ref_fold, attempt(lambda: wide_of(nodes, 1)), attempt(lambda: wide_of(nodes, 2)))):
        return                                                 # a leaf root, or a tree nobody folds: no records, no tree of the backend's own
    iso, dirs = shadow_metric_of(sc["lights"])
    own = attempt(lambda: capi.device_tree(ctx, nodes, iso, dirs)[0])
    own_folds = own is not None and attempt(lambda: capi.device_fold(ctx, own, iso, dirs)) is not None
    assert ("shadow tree: built on the device (PLOC)" in report) == own_folds, report
    assert ("built on the device (PLOC), forced" in report) == own_folds, report
    if str(which).startswith("triangles at 2^k"):
        # the path from refusal to the fall-back: the reference's tree folds on the device, the tree built there over its leaves is too deep -- for its depth alone --
        # and so is the one the host's builder makes where it is started; the shadow rays (there are some) walk the reference's topology, and the bits above held
        assert ref_fold is not None and own is not None and not own_folds
        assert _trees.frame_ok(own) and _trees.record_levels(own, _trees.metric_weights(own, iso, dirs)) > _trees.MAX_LEVELS
        assert "shadow tree: the own tree does not qualify -> reference topology" in report, report
        assert st.shadow_rays > 0
