"""A corpus of small, lopsided and extreme binary trees for the tree code -- the host's restatements (tests/test_wide_bvh.py, test_own_tree.py, test_refit.py) and
the device's kernels (tests/test_gpu_tree_edges.py) are run over the same cases.  A plain module: no fixtures, no pytest settings.

  * synthesised trees: T.bvh_node arrays written directly in the reference's linear layout (first child at i + 1, second at `offset`, a leaf has
    num_primitives_axis >> 16 != 0), interior boxes the exact unions of their children's -- leaf counts around the kernels' block sizes, balanced / random /
    chain topologies, random and degenerate leaf boxes;
  * built trees: triangles through the reference's builder (bvh_of) -- the generators of the CPU suite's soup tests live here, with their seeds.

Whether a tree is MEANT to fold is decided here, by `expected_to_fold`: thirty lines of plain Python that restate the rule (the collapse's dynamic programme with
its first-minimum tie-break, then the depth of the record tree against the 33 levels the walk's stack allows; the root box against the frame's limits) -- not by
asking the code under test."""
import collections
import numpy as np
from raytracing_amd import scenes as S, types as T

Case = collections.namedtuple("Case", "name nodes tris folds kind")     # tris: None for a synthesised tree; folds: meant to qualify for the 4-wide layout
MATS = np.array([S.make_material(kd=(0.7, 0.7, 0.7))], dtype=T.packed_material)
LEAF_COUNTS = (2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
MAX_LEVELS = 33                                                          # record levels k_trace_w4's stack holds (three pending slots per level)


# ---- the soups of the CPU suite (their tests import these: same generators, same seeds) -----------------------------------------------------------------------
def _flat_normals(n):
    return np.tile(np.array([0, 0, 1], np.float32), (n, 3, 1))


def extreme_soup(seed):
    """test_wide_tree_of_random_soups_with_extreme_coordinates: slivers, coincident triangles, huge offsets (coarse fp32 grid) and tiny extents"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    scale = float(10.0 ** rng.integers(-6, 7))
    offset = rng.normal(size=3) * float(10.0 ** rng.integers(-3, 8))
    P = (rng.normal(size=(n, 1, 3)) * scale + rng.normal(size=(n, 3, 3)) * scale * float(10.0 ** rng.integers(-5, 1)) + offset)
    P = P.astype(np.float32)
    if seed % 2:
        P[: n // 3] = P[0]                                   # coincident triangles
    return S.to_triangles([(P, _flat_normals(n), np.zeros((n, 3, 2), np.float32), 0)]), MATS


def sah_soup(seed):
    """test_the_sah_collapse_is_optimal_on_small_trees"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 120))
    P = (rng.normal(size=(n, 1, 3)) * rng.uniform(0.2, 3.0, size=(1, 1, 3)) + rng.normal(size=(n, 3, 3)) * 0.05).astype(np.float32)
    return S.to_triangles([(P, _flat_normals(n), np.zeros((n, 3, 2), np.float32), 0)]), MATS


def refit_soup(seed):
    """test_node_refit_and_folds_on_random_soups: (triangles, materials, the generator -- the test draws its poses from it afterwards)"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(3, 600))
    scale = float(10.0 ** rng.integers(-4, 5))
    offset = rng.normal(size=3) * float(10.0 ** rng.integers(-3, 6))
    P = (rng.normal(size=(n, 1, 3)) * scale + rng.normal(size=(n, 3, 3)) * scale * float(10.0 ** rng.integers(-4, 1)) + offset).astype(np.float32)
    return S.to_triangles([(P, _flat_normals(n), np.zeros((n, 3, 2), np.float32), 0)]), MATS, rng


def shadow_soup(seed):
    """test_shadow_verdicts_on_random_soups: slivers, coincident triangles (ties!), geometry around the lights"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 600))
    P = rng.normal(size=(n, 1, 3)) * 1.2 + rng.normal(size=(n, 3, 3)) * float(10.0 ** rng.uniform(-1.2, 0.0)) + np.array([0.0, 2.5, 1.0])
    P = P.astype(np.float32)
    if seed % 2:
        P[: n // 4] = P[0]
    N = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    N = (N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-20)).astype(np.float32)[:, None, :].repeat(3, 1)
    tris = S.to_triangles([(P, N, np.zeros((n, 3, 2), np.float32), 0)])
    mats = np.array([S.make_material(kd=(0.7, 0.6, 0.5), ks=(0.3, 0.3, 0.3), roughness=0.3)], dtype=T.packed_material)
    return tris, mats


def one_triangle(p):
    P = np.asarray(p, np.float32).reshape(1, 3, 3)
    return S.to_triangles([(P, _flat_normals(1), np.zeros((1, 3, 2), np.float32), 0)])


def leaf_root_scene():
    """test_a_leaf_root_and_a_two_triangle_scene, first half"""
    return one_triangle([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), MATS


def two_triangle_scene():
    """... and its second half"""
    return np.concatenate([one_triangle([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), one_triangle([[5, 5, 5], [6, 5, 5], [5, 6, 7]])]), MATS


# triangle counts of `grid_soup` that put the refit's grids (256 threads a block; the fold's k_fold_emit: 64) one short of, on and one past a block boundary: the
# builder gives these soups one triangle per leaf, so triangles = leaves = 63 .. 65 and 255 .. 257, interior nodes = one less (64 .. 66, 256 .. 258 for the same
# boundaries), and the records of the two-level fold number 63, 64, 65 at 121, 126, 129 triangles and 255, 256, 257 at 515, 495, 516 (the SAH fold: 64, 65 at 127,
# 134).  tests/test_tree_corpus.py asserts that these counts are met.
GRID_TRIANGLES = (63, 64, 65, 66, 121, 126, 127, 129, 134, 255, 256, 257, 258, 495, 515, 516)
GRID_SIZES = (63, 64, 65, 255, 256, 257)


def grid_soup(n):
    rng = np.random.default_rng(11)
    P = (rng.normal(size=(n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 0.05).astype(np.float32)
    return S.to_triangles([(P, _flat_normals(n), np.zeros((n, 3, 2), np.float32), 0)]), MATS


# ---- synthesised trees ------------------------------------------------------------------------------------------------------------------------------------------
def leaf_boxes(kind, n, rng):
    """float32[n, 2, 3]: lo, hi of every leaf"""
    f = np.float32
    if kind == "random":
        c = rng.uniform(-1, 1, (n, 3)) * [3.0, 2.0, 1.0]
        h = rng.uniform(0.01, 0.2, (n, 3))
        return np.stack([c - h, c + h], 1).astype(f)
    if kind == "identical":                                    # every cost a tie, every Morton code the same
        return np.tile(np.array([[0.25, -1.0, 2.0], [1.25, 0.5, 2.5]], f), (n, 1, 1))
    if kind == "point":                                        # zero extent on all three axes, the root's too
        return np.tile(np.array([[1.5, -2.25, 0.75], [1.5, -2.25, 0.75]], f), (n, 1, 1))
    if kind == "points":                                       # zero-extent leaves at distinct points
        c = rng.uniform(-2, 2, (n, 3)).astype(f)
        return np.stack([c, c], 1)
    if kind == "coplanar":                                     # one axis of zero extent
        c = rng.uniform(-1, 1, (n, 3)) * [3.0, 2.0, 0.0] + [0.0, 0.0, 0.5]
        h = rng.uniform(0.01, 0.2, (n, 3)) * [1.0, 1.0, 0.0]
        return np.stack([c - h, c + h], 1).astype(f)
    if kind == "diagonal":                                     # collinear on a space diagonal
        t = rng.permutation(n).astype(np.float64) / max(n, 1) * 4.0 - 2.0
        c = np.stack([t, t, t], 1)
        return np.stack([c - 0.01, c + 0.01], 1).astype(f)
    if kind == "clusters":                                     # two tight clusters 1e7 apart
        c = rng.normal(size=(n, 3)) * 1e-3
        c[n // 2:, 0] += 1e7
        h = rng.uniform(1e-5, 1e-4, (n, 3))
        return np.stack([c - h, c + h], 1).astype(f)
    if kind in ("pow2", "pow2 near"):
        # unit boxes centred at 2^k along x.  "pow2": k = -100 .. 99 (coordinates far beyond what a record's frame takes: no fold of any tree over these leaves
        # qualifies); "pow2 near": k = -172 .. 27, every coordinate within the frame's limits, so that a fold can be refused for its depth alone.
        # In binary32 these are not 200 distinct boxes: 2^k +- 0.5 rounds to +- 0.5 for every k <= -26 (and 2^k itself is 0 below k = -149), so the first 75 ("pow2")
        # or 147 ("pow2 near") leaves coincide exactly, and 0.5 + 2^k has only a few bits left up to k = -1.  PLOC's one merge per round, a tree as deep as it has
        # leaves, therefore comes about in two ways: among the coincident leaves every cost ties and only positions 0 and 1 choose each other (the tie-break by
        # lower position, the stable sort); from k = 0 on it is the geometry -- every box is nearer to everything below it than to its upper neighbour.
        k = np.arange(-100, 100) if kind == "pow2" else np.arange(-172, 28)
        assert n == len(k)
        c = np.stack([np.ldexp(1.0, k), np.zeros(n), np.zeros(n)], 1)
        return np.stack([c - 0.5, c + 0.5], 1).astype(f)
    raise ValueError(kind)


def synthesise(boxes, topology, rng=None):
    """The tree over leaves 0 .. n - 1 (leaf k: box k, first triangle k, one triangle) of the given topology, in the reference's linear layout.
    topology: "balanced", "random" (split sizes drawn from rng), "left" (a chain through the first children), "right" (through the second children)."""
    n = len(boxes)
    nodes = np.zeros(2 * n - 1, T.bvh_node)
    lo, hi = np.zeros((2 * n - 1, 3), np.float32), np.zeros((2 * n - 1, 3), np.float32)
    at = 0
    todo = [(0, n, -1)]                                        # (first leaf, leaf count, the parent waiting for its second child's index)
    pending = []                                               # interior nodes in the order made: their boxes are filled in afterwards, children first
    while todo:
        first, count, parent = todo.pop()
        me = at
        at += 1
        if parent >= 0:
            nodes["offset"][parent] = me
        if count == 1:
            nodes["num_primitives_axis"][me] = 1 << 16
            nodes["offset"][me] = first
            lo[me], hi[me] = boxes[first, 0], boxes[first, 1]
            continue
        give = {"balanced": count - count // 2, "left": count - 1, "right": 1}.get(topology) or int(rng.integers(1, count))
        nodes["num_primitives_axis"][me] = me % 3             # the split axis: any of the three
        pending.append(me)
        todo.append((first + give, count - give, me))         # popped second: follows the first child's subtree
        todo.append((first, give, -1))
    for me in reversed(pending):
        a, b = me + 1, int(nodes["offset"][me])
        lo[me], hi[me] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
    for k, c in enumerate("xyz"):
        nodes["bounds_min"][c], nodes["bounds_max"][c] = lo[:, k], hi[:, k]
    return nodes


def chain_leaves(interior):
    return interior + 1


# ---- what a tree is meant to do: the rule, restated -------------------------------------------------------------------------------------------------------------
def is_leaf(nodes):
    return (nodes["num_primitives_axis"] >> 16) != 0


def extents(nodes):
    return np.stack([nodes["bounds_max"][c].astype(np.float64) - nodes["bounds_min"][c].astype(np.float64) for c in "xyz"], 1)


def area_weights(nodes):
    e = extents(nodes)
    return e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]


def metric_weights(nodes, iso, dirs):
    """own_bvh.h's metric: iso * half the surface area + the projected areas along |dirs| (binary32 directions, as the debug entries take them)"""
    e = extents(nodes)
    m = iso * 0.5 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    for d in np.abs(np.asarray(dirs, np.float32).reshape(-1, 3).astype(np.float64)):
        m = m + d[0] * e[:, 1] * e[:, 2] + d[1] * e[:, 2] * e[:, 0] + d[2] * e[:, 0] * e[:, 1]
    return m


def record_levels(nodes, weights=None):
    """Depth of the record tree of the SAH collapse (root = 1; 0 for a leaf root): T[n] = weight + F[n][4], F[n][k] = min over i of G(first, i) + G(second, k - i),
    the FIRST minimum kept; with k slots to spend a node below a record's root is folded iff F[n][k] < T[n]."""
    leaf = is_leaf(nodes)
    if leaf[0]:
        return 0
    w = area_weights(nodes) if weights is None else np.asarray(weights, np.float64)
    off = nodes["offset"].astype(np.int64)
    nn = len(nodes)
    Tn, F = np.zeros(nn), np.zeros((nn, 5))
    split, opened = np.zeros((nn, 5), np.int64), np.zeros(nn, np.int64)
    G = lambda c, i: 0.0 if leaf[c] else (min(Tn[c], F[c, i]) if i >= 2 else Tn[c])
    for n in range(nn - 1, -1, -1):
        if leaf[n]:
            continue
        l, r = n + 1, int(off[n])
        for k in (2, 3, 4):
            best, at = 0.0, 0
            for i in range(1, k):
                c = G(l, i) + G(r, k - i)
                if at == 0 or c < best:
                    best, at = c, i
            F[n, k], split[n, k] = best, at
        Tn[n] = w[n] + F[n, 4]
        for i in (2, 3, 4):
            if F[n, i] < Tn[n]:
                opened[n] |= 1 << i
    def slots(n, k, out):
        give = (int(split[n, k]), k - int(split[n, k]))
        for c, g in zip((n + 1, int(off[n])), give):
            if not leaf[c] and g >= 2 and (opened[c] >> g) & 1:
                slots(c, g, out)
            else:
                out.append(c)
    deepest, todo = 0, [(0, 1)]
    while todo:
        n, depth = todo.pop()
        deepest = max(deepest, depth)
        out = []
        slots(n, 4, out)
        todo += [(c, depth + 1) for c in out if not leaf[c]]
    return deepest


def frame_ok(nodes):
    """wide_quant.h's limits on the root's box (every other box lies inside it): coordinates below 2^28, 254 cells of at most 2^20 span the extent"""
    lo = np.array([nodes["bounds_min"][c][0] for c in "xyz"], np.float64)
    hi = np.array([nodes["bounds_max"][c][0] for c in "xyz"], np.float64)
    return bool((np.maximum(np.abs(lo), np.abs(hi)) < 2.0 ** 28).all() and ((hi - lo) <= 254.0 * 2.0 ** 20).all())


def expected_to_fold(nodes, weights=None):
    return bool(is_leaf(nodes)[0]) or (frame_ok(nodes) and record_levels(nodes, weights) <= MAX_LEVELS)


def morton_cells(nodes):
    """ploc_kernels.h's k_ploc_keys in the world frame: per leaf the three 21-bit cell coordinates of its box's centre (cells of the root's longest extent; 1.0
    where that is zero)"""
    leaves = nodes[is_leaf(nodes)]
    lo = np.array([nodes["bounds_min"][c][0] for c in "xyz"], np.float64)
    hi = np.array([nodes["bounds_max"][c][0] for c in "xyz"], np.float64)
    longest = float((hi - lo).max())
    e = longest if longest > 0.0 else 1.0
    c = np.stack([0.5 * (leaves["bounds_min"][a].astype(np.float64) + leaves["bounds_max"][a].astype(np.float64)) for a in "xyz"], 1)
    t = np.clip((c - lo) / e, 0.0, 1.0)
    return (t * 2097151.0).astype(np.uint32)


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------------------------------------
LEAF_ROOTS = ("one triangle",)                                           # the cases whose root is a leaf (tests/test_tree_corpus.py checks the list): no tree to build over them
_specs, _cases = None, {}


def _built(name, tris, mats):
    from tests.test_wide_bvh import bvh_of
    nodes, tris = bvh_of(tris, mats)
    return Case(name, nodes, tris, expected_to_fold(nodes), "built")


def _synth(name, kind, n, topology, seed):
    rng = np.random.default_rng(seed)
    nodes = synthesise(leaf_boxes(kind, n, rng), topology, rng)
    return Case(name, nodes, None, expected_to_fold(nodes), "synth")


def specs():
    """name -> (kind, how to make it): the list costs nothing, a case is made when `case` is first asked for it"""
    global _specs
    if _specs is not None:
        return _specs
    out = {}
    def add(kind, name, make, *args):
        assert name not in out
        out[name] = (kind, lambda: make(name, *args))
    def synth(name, kind, n, topology, seed):
        add("synth", name, _synth, kind, n, topology, seed)
    def built(name, soup, *args):
        add("built", name, lambda name, *a: _built(name, *soup(*a)[:2]), *args)
    # every leaf count, balanced and with random split sizes, random boxes: node counts 2 L - 1 around 64, 256, 1024 and 2048
    for i, n in enumerate(LEAF_COUNTS):
        synth("balanced %d" % n, "random", n, "balanced", 1000 + i)
        synth("random %d" % n, "random", n, "random", 2000 + i)
    # every kind of degenerate leaf box under every topology, chains of 20 and 80 interior nodes each way
    shapes = (("balanced", 65), ("random", 129), ("left", chain_leaves(20)), ("right", chain_leaves(20)), ("left", chain_leaves(80)), ("right", chain_leaves(80)))
    for j, kind in enumerate(("random", "identical", "point", "points", "coplanar", "diagonal", "clusters")):
        for i, (topology, n) in enumerate(shapes):
            synth("%s, %s %d" % (kind, topology, n), kind, n, topology, 3000 + 10 * j + i)
    # ties and zero extents across the scan's and the sort's block boundaries
    for i, (kind, n) in enumerate((("identical", 513), ("identical", 1025), ("point", 512), ("points", 1024), ("coplanar", 257), ("clusters", 1023))):
        synth("%s, random %d" % (kind, n), kind, n, "random", 4000 + i)
    # chains of 120 interior nodes: 40 record levels at three folded nodes a record -- refused whatever the boxes
    for i, (kind, topology) in enumerate((("random", "left"), ("random", "right"), ("identical", "left"), ("identical", "right"))):
        synth("%s, %s %d" % (kind, topology, chain_leaves(120)), kind, chain_leaves(120), topology, 5000 + i)
    for i, kind in enumerate(("pow2", "pow2 near")):
        synth("%s, balanced 200" % kind, kind, 200, "balanced", 6000 + i)
    for seed in range(6):
        built("extreme soup %d" % seed, extreme_soup, seed)
    for seed in range(8):
        built("sah soup %d" % seed, sah_soup, seed)
    for seed in range(6):
        built("refit soup %d" % seed, refit_soup, seed)
    for seed in range(6):
        built("shadow soup %d" % seed, shadow_soup, seed)
    built("one triangle", leaf_root_scene)
    built("two triangles", two_triangle_scene)
    for n in GRID_TRIANGLES:
        built("grid soup %d" % n, grid_soup, n)
    _specs = out
    return out


def names(kind=None, leaf_roots=True):
    return [n for n, (k, _) in specs().items() if kind in (None, k) and (leaf_roots or n not in LEAF_ROOTS)]


def case(name):
    """made once per process and never changed (callers copy before they write)"""
    if name not in _cases:
        _cases[name] = specs()[name][1]()
    return _cases[name]


def corpus():
    return [case(n) for n in names()]
