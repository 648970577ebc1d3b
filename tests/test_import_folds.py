"""What rt_scene_import_folds takes and what it refuses (rtw::check_fold in wide_bvh.cpp, reached without a context through rt_debug_check_folds), against a
plain restatement of the rule written here: imported records go straight under k_trace_w4 and every query walk, so they must be a tree from the entry (a cycle
is a walk that never ends), at most 33 record levels deep (the walks' stacks are sized from that), over exactly the scene's leaves, each reached once by its
FIRST triangle (the leaf's exact box and its triangle count travel in that record), with slot counts and frames as build_wide_bvh writes them.

  * nothing valid is refused: every fold the library makes of every tree of tests/_trees.py that folds -- SAH, two levels, the own tree's metric, random
    weights, the pair layout -- is accepted, by the library and by the restatement;
  * every class of defect, by the smallest mutation of a valid fold that shows it: both refuse, and name the same class;
  * the depth boundary from both sides, records by the hundred thousand (the check is iterative), and 2 400 random single-word mutations on which the
    library's answer must be the restatement's.

No GPU: the check is host code.  Nothing here runs a walk on records that should have been refused."""
import collections
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests import _trees
from tests.test_wide_bvh import WIDE, wide_of
from tests.test_own_tree import own_tree, wide_metric, light_dir

LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
MAX_LEVELS = 33                  # wide_bvh.cpp's walk in build_wide_bvh: the entry's record is level 1, `depth > 33` is refused; leaves are no level
# wide_quant.h, wide_frame: cell = 2^e with e from -126 (where it starts) to 20 (`e > 20` is refused), stored biased by 127; a box coordinate is refused unless
# |c| < 2^28, and the origin is floor(min / cell) * cell with cell a power of two <= 2^20, so |origin| <= 2^28
EXP_BYTES = (1, 147)
ORIGIN_MAX = 2.0 ** 28

# the library's words for each class (the text in parentheses of "... do not fit this scene (...)")
WORDS = {
    "entry": "the entry is not a record of the array, or without records not a leaf",
    "range": "a ref outside the records / the triangles",
    "twice": "a record is reached twice",
    "deep": "deeper than the walk's stack",
    "slots": "a record's slot count is not the number of its refs, 2 to 4",
    "frame": "a record's frame is outside what the walk's arithmetic takes",
    "not a start": "a leaf ref is not the first triangle of a leaf of the scene",
    "leaf twice": "a leaf of the scene is reached twice",
    "missing": "a leaf of the scene is missing",
}


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------------------
def restated(nodes, recs, entry):
    """The class of the first defect in the order of WORDS, or None.  Level by level from the entry, with sets and counters; shares nothing with the library."""
    recs = np.ascontiguousarray(recs).view(WIDE).reshape(-1)
    leaves = nodes[(nodes["num_primitives_axis"] >> 16) != 0]
    n_tris = int((leaves["offset"].astype(np.int64) + (leaves["num_primitives_axis"] >> 16)).max())
    scene_has = collections.Counter(int(o) for o in leaves["offset"])
    n = len(recs)
    refs = [[int(x) for x in r] for r in recs["ref"]]
    if n == 0:
        if not entry & LEAF or entry == EMPTY:
            return "entry"
    elif entry >= n:
        return "entry"
    for x in ([entry] if n == 0 else [x for r in refs for x in r if x != EMPTY]):
        if (x & LEAF and (x ^ LEAF) >= n_tris) or (not x & LEAF and x >= n):
            return "range"
    reached, got, levels, level = set(), collections.Counter(), 0, [entry]
    while level:
        here = [x for x in level if not x & LEAF]
        got.update(x ^ LEAF for x in level if x & LEAF)
        if len(set(here)) != len(here) or reached & set(here):
            return "twice"
        reached |= set(here)
        levels += 1 if here else 0
        level = [x for r in here for x in refs[r] if x != EMPTY]
    if levels > MAX_LEVELS:
        return "deep"
    order = sorted(reached)
    for r in order:
        occupied = sum(x != EMPTY for x in refs[r])
        if int(recs["meta"][r]) >> 24 != occupied or not 2 <= occupied <= 4:
            return "slots"
    for r in order:
        meta = int(recs["meta"][r])
        for a in range(3):
            o = float(recs["origin"][r][a])
            if not np.isfinite(o) or abs(o) > ORIGIN_MAX or not EXP_BYTES[0] <= (meta >> (8 * a)) & 0xFF <= EXP_BYTES[1]:
                return "frame"
    if any(t not in scene_has for t in got):
        return "not a start"
    if any(got[t] > scene_has[t] for t in got):
        return "leaf twice"
    if any(got[t] < c for t, c in scene_has.items()):
        return "missing"
    return None


def library(nodes, recs, entry):
    """the same answer from rt_debug_check_folds: the class its message names, or None"""
    try:
        capi.check_folds(nodes, recs, entry)
    except capi.RtError as e:
        said = str(e)
        assert said.startswith("rt_debug_check_folds: the records do not fit this scene ("), said
        cls = [k for k, v in WORDS.items() if said.endswith("(" + v + ")")]
        assert len(cls) == 1, said
        return cls[0]
    return None


def both(nodes, recs, entry):
    a, b = library(nodes, recs, entry), restated(nodes, recs, entry)
    assert a == b, "the library says %r, the restatement %r" % (a, b)
    return a


# ---- folds to work on --------------------------------------------------------------------------------------------------------------------------------
def two_triangle_leaves(n_leaves, topology, seed):
    """a synthesised tree of _trees.py whose leaf k holds triangles 2 k and 2 k + 1 (the folds do not look at triangles)"""
    rng = np.random.default_rng(seed)
    nodes = _trees.synthesise(_trees.leaf_boxes("random", n_leaves, rng), topology, rng)
    leaf = _trees.is_leaf(nodes)
    nodes["offset"][leaf] *= 2
    nodes["num_primitives_axis"][leaf] = 2 << 16
    return nodes


@pytest.fixture(scope="module")
def small():
    """(nodes, records, entry): 65 two-triangle leaves, random splits -- some twenty records"""
    nodes = two_triangle_leaves(65, "random", 77)
    recs, entry = wide_of(nodes)
    assert 10 <= len(recs) <= 64 and both(nodes, recs, entry) is None
    return nodes, recs, entry


def shape(recs, entry):
    """parent[(record)] = (record, slot) it hangs from; level[record]; reached records in depth-first order"""
    parent, level, order, todo = {}, {entry: 1}, [], [entry]
    while todo:
        r = todo.pop()
        order.append(r)
        for k in range(3, -1, -1):
            x = int(recs["ref"][r][k])
            if x != EMPTY and not x & LEAF:
                parent[x], level[x] = (r, k), level[r] + 1
                todo.append(x)
    return parent, level, order


def slots_of(recs, r, leaf):
    return [k for k in range(4) if int(recs["ref"][r][k]) != EMPTY and bool(int(recs["ref"][r][k]) & LEAF) == leaf]


def empty_slot(recs, r, k):
    recs["ref"][r][k] = EMPTY
    for a in range(3):
        recs["lo"][r][a] |= 255 << (8 * k)
        recs["hi"][r][a] &= ~np.uint32(255 << (8 * k))


def fewer_slots(recs, r):
    recs["meta"][r] = (int(recs["meta"][r]) & 0xFFFFFF) | ((int(recs["meta"][r]) >> 24) - 1) << 24


# ---- nothing valid is refused --------------------------------------------------------------------------------------------------------------------------
def folds_of(case):
    """name -> (records, entry) for every fold the library makes of the case's tree; a fold the BUILDER itself turns down (two levels at a time or other
    weights can be deeper than the SAH fold that `expected_to_fold` speaks of) is not there"""
    nodes = case.nodes
    out = {}
    def attempt(name, make):
        try:
            out[name] = make()
        except capi.RtError as e:
            assert "does not qualify" in str(e), (case.name, name, str(e))
    recs, entry, roots = wide_of(nodes, 1, with_roots=True)                 # (meant to fold: this one is not allowed to fail)
    out["sah"] = (recs, entry)
    attempt("two levels", lambda: wide_of(nodes, 2))
    d = light_dir()
    if _trees.is_leaf(nodes)[0]:
        attempt("metric", lambda: wide_metric(nodes, 0.5, [d]))
    else:
        attempt("metric", lambda: wide_metric(own_tree(nodes, 0.5, [d]), 0.5, [d]))       # the shadow rays' own tree: other interior nodes, the SAME leaves
    rng = np.random.default_rng(len(nodes))
    w = rng.integers(0, 50, len(nodes)).astype(np.float64) + rng.random(len(nodes)) * 0.01
    attempt("weights", lambda: capi.wide_bvh_weights(nodes, w)[:2])
    if len(recs):
        paired, proots = recs.copy(), roots.copy()
        assert capi.load().rt_debug_pair_layout(np.ascontiguousarray(nodes).ctypes.data, len(nodes), paired.ctypes.data, proots.ctypes.data, len(paired)) == 0
        out["pairs"] = (paired, int(np.nonzero(proots == 0)[0][0]))
    return out


def test_nothing_the_library_folds_is_refused():
    tried, turned_down = collections.Counter(), collections.defaultdict(set)
    names =[n for n in _trees.names() if _trees.case(n).folds]
    assert set(_trees.LEAF_ROOTS) <= set(names)
    # the deepest chains of the corpus that still fold (80 interior nodes: 27 record levels; the chains of 120 are meant not to)
    assert {"random, left 81", "random, right 81", "identical, left 81", "identical, right 81"} <= set(names)
    for name in names:
        case = _trees.case(name)
        folds = folds_of(case)
        for kind in {"two levels", "metric", "weights"} - set(folds):
            turned_down[kind].add(name)
        for kind, (recs, entry) in folds.items():
            assert both(case.nodes, recs, entry) is None, (name, kind)
            tried[kind] += 1
    assert tried["sah"] == len(names) and tried["pairs"] == len(names) - len(_trees.LEAF_ROOTS)
    # what the builder itself turns down: two levels at a time make 40 record levels of a chain of 80 interior nodes, which three nodes a record fold in 27
    assert turned_down["two levels"] <= {n for n in names if n.endswith((", left 81", ", right 81"))}, turned_down
    assert min(tried["metric"], tried["weights"]) >= len(names) * 9 // 10, tried


# ---- each class of defect, by the smallest mutation that shows it ---------------------------------------------------------------------------------------
def defects(nodes, recs, entry, other=None):
    """(name, records, entry, class or None = any) -- every one a small change of the valid fold `recs` of a tree over the leaves of `nodes`;
    other: (records, entry) of another scene's fold (here: of a tree over 50 two-triangle leaves)"""
    recs = np.ascontiguousarray(recs).view(WIDE).reshape(-1)
    parent, level, order = shape(recs, entry)
    n = len(recs)
    leaves = nodes[_trees.is_leaf(nodes)]
    size_of = dict(zip(leaves["offset"].tolist(), (leaves["num_primitives_axis"] >> 16).tolist()))
    n_tris = max(t + c for t, c in size_of.items())
    out = []
    def case(name, cls, change, new_entry=None):
        bad = recs.copy()
        change(bad)
        out.append((name, bad, entry if new_entry is None else new_entry, cls))
    def set_ref(r, k, to):
        return lambda bad: bad["ref"][r].__setitem__(k, to)
    inner = next(r for r in order if slots_of(recs, r, False) and r != entry)                # a record below the entry with a record below it
    deep = max(order, key=lambda r: level[r])
    assert level[deep] >= 3
    case("a ref at its own record", "twice", set_ref(inner, slots_of(recs, inner, False)[0], inner))
    case("a ref at an ancestor", "twice", set_ref(deep, slots_of(recs, deep, True)[0], parent[parent[deep][0]][0]))
    case("a ref at the entry", "twice", set_ref(inner, slots_of(recs, inner, False)[0], entry))
    two = next(r for r in order if slots_of(recs, r, False) and len(slots_of(recs, r, False) + slots_of(recs, r, True)) >= 2)
    k_in = slots_of(recs, two, False)[0]
    k_other = next(k for k in slots_of(recs, two, False) + slots_of(recs, two, True) if k != k_in)
    case("two slots at the same record", "twice", set_ref(two, k_other, int(recs["ref"][two][k_in])))
    # a record with three or four slots, two of them leaves, the first of these a leaf of two triangles or more
    big = lambda r, k: size_of[int(recs["ref"][r][k]) ^ LEAF] >= 2
    leafy = next(r for r in order if len(slots_of(recs, r, True)) >= 2 and int(recs["meta"][r]) >> 24 >= 3 and any(big(r, k) for k in slots_of(recs, r, True)))
    k0 = next(k for k in slots_of(recs, leafy, True) if big(leafy, k))
    k1 = next(k for k in slots_of(recs, leafy, True) if k != k0)
    case("a leaf ref at n_tris", "range", set_ref(leafy, k0, LEAF | n_tris))
    case("a leaf ref beyond n_tris", "range", set_ref(leafy, k0, LEAF | (n_tris + 1000)))
    case("a leaf ref at a leaf's second triangle", "not a start", set_ref(leafy, k0, int(recs["ref"][leafy][k0]) + 1))
    case("a leaf ref over another leaf's slot", "leaf twice", set_ref(leafy, k0, int(recs["ref"][leafy][k1])))
    case("a leaf slot emptied, the count adjusted", "missing", lambda bad: (empty_slot(bad, leafy, k0), fewer_slots(bad, leafy)))
    case("a leaf slot emptied, the count left", "slots", lambda bad: empty_slot(bad, leafy, k0))
    case("the entry one past the records", "entry", lambda bad: None, n)
    case("a leaf entry with records", "entry", lambda bad: None, LEAF | 0)
    case("an exponent byte of 255", "frame", lambda bad: bad["meta"].__setitem__(inner, int(bad["meta"][inner]) | 0xFF00))
    case("a NaN origin", "frame", lambda bad: bad["origin"][inner].__setitem__(2, np.nan))
    out.append(("the first half of the records", recs[:n // 2].copy(), entry, None))
    out.append(("zero bytes", np.zeros(n, WIDE), entry, "twice"))                              # record 0's four refs are record 0
    # another scene's records, the count padded to match
    if other is None:
        other_nodes = two_triangle_leaves(50, "balanced", 78)                                  # a valid fold, of a scene with fewer leaves
        other = wide_of(other_nodes)
        assert both(other_nodes, other[0], other[1]) is None
        cls = "missing"
    else:
        cls = None
    theirs = np.ascontiguousarray(other[0]).view(WIDE).reshape(-1)
    padded = np.zeros(max(n, len(theirs)), WIDE)
    padded[:len(theirs)] = theirs
    padded[len(theirs):] = theirs[0]                                                           # (unreached copies: tolerated as such)
    out.append(("another scene's records", padded, other[1], cls))
    assert len(out) == 17
    return out


def test_every_class_of_defect_is_refused_and_named(small):
    nodes, recs, entry = small
    cases = defects(nodes, recs, entry)
    for name, bad, bad_entry, cls in cases:
        said = both(nodes, bad, bad_entry)
        assert said is not None, name + ": accepted"
        assert cls is None or said == cls, (name, said, cls)
    assert both(nodes, recs, entry) is None                                                    # ... and nothing above wrote to the fixture


def test_another_scenes_records_with_other_leaves_are_refused(small):
    """the same record count, other leaves: a tree whose leaves hold three triangles each"""
    nodes, recs, entry = small
    rng = np.random.default_rng(77)
    other = _trees.synthesise(_trees.leaf_boxes("random", 65, rng), "random", rng)                # the same topology as `small` ...
    leaf = _trees.is_leaf(other)
    other["offset"][leaf] *= 3                                                                 # ... over leaves of three triangles
    other["num_primitives_axis"][leaf] = 3 << 16
    theirs, their_entry = wide_of(other)
    assert len(theirs) == len(recs) and both(other, theirs, their_entry) is None
    assert both(nodes, theirs, their_entry) in ("range", "not a start")
    assert both(other, recs, entry) in ("not a start", "missing")


def test_a_leaf_root_has_no_records_and_its_entry_is_its_leaf():
    case = _trees.case("one triangle")
    recs, entry = wide_of(case.nodes)
    assert len(recs) == 0 and entry == LEAF | int(case.nodes["offset"][0])
    assert both(case.nodes, recs, entry) is None
    assert both(case.nodes, recs, 0) == "entry"                                                # not a leaf ref
    assert both(case.nodes, recs, EMPTY) == "entry"
    assert both(case.nodes, recs, entry + 1) == "range"                                        # beyond the one triangle
    two = _trees.case("two triangles")
    if not _trees.is_leaf(two.nodes)[0]:
        assert both(two.nodes, recs, LEAF | int(two.nodes["offset"][1])) == "missing"          # one leaf of two as the whole tree


# ---- the depth boundary ---------------------------------------------------------------------------------------------------------------------------------
def chain(interior, topology="left"):
    rng = np.random.default_rng(5)
    return _trees.synthesise(_trees.leaf_boxes("random", _trees.chain_leaves(interior), rng), topology, rng)


def spliced(recs, entry):
    """one record more on the way down: a new record takes one leaf of the entry's record and the record below it, the entry's record refers to the new one"""
    k_chain, k_leaf = slots_of(recs, entry, False)[0], slots_of(recs, entry, True)[0]
    assert int(recs["meta"][entry]) >> 24 >= 3
    out = np.concatenate([recs, recs[entry:entry + 1]])
    new = len(recs)
    for k in range(4):
        if k not in (k_chain, k_leaf):
            empty_slot(out, new, k)
    out["meta"][new] = (int(out["meta"][new]) & 0xFFFFFF) | 2 << 24
    out["ref"][entry][k_leaf] = new
    empty_slot(out, entry, k_chain)
    fewer_slots(out, entry)
    return out


def test_the_depth_boundary_from_both_sides():
    # the chain whose SAH fold has exactly 33 record levels, found by _trees.py's restatement of the collapse (three folded nodes a record: 99)
    interior = next(k for k in range(60, 140) if _trees.record_levels(chain(k)) == MAX_LEVELS and _trees.record_levels(chain(k + 1)) == MAX_LEVELS + 1)
    nodes = chain(interior)
    recs, entry = wide_of(nodes)                                                               # build_wide_bvh accepts it ...
    parent, level, order = shape(recs, entry)
    assert max(level.values()) == MAX_LEVELS
    assert both(nodes, recs, entry) is None                                                    # ... and so does the importer
    with pytest.raises(capi.RtError, match="does not qualify"):                                # one level more: the builder's own refusal
        wide_of(chain(interior + 1))
    # one level more by hand: a record spliced in between the entry's record and the chain below it, holding one of the entry's leaves and the chain
    deeper = spliced(recs, entry)
    assert max(shape(deeper, entry)[1].values()) == MAX_LEVELS + 1
    assert both(nodes, deeper, entry) == "deep"
    # the same splice on a fold with a level to spare is taken: it is the depth that is refused, nothing else about the splice
    shallow_nodes = chain(interior - 3)
    shallow, e = wide_of(shallow_nodes)
    assert max(shape(shallow, e)[1].values()) == MAX_LEVELS - 1
    assert both(shallow_nodes, spliced(shallow, e), e) is None


# ---- long inputs: the check is iterative ------------------------------------------------------------------------------------------------------------------
def long_chain(n, cycle):
    """n records, record i = (leaf i, record i + 1); the last one holds leaves n - 1 and n -- or, `cycle`, leaf n - 1 and record 0.  The tree: a chain
    through the second children over n + 1 one-triangle leaves."""
    leaves = n + 1
    nodes = np.zeros(2 * leaves - 1, T.bvh_node)
    interior = np.arange(0, 2 * leaves - 2, 2)
    nodes["offset"][interior] = interior + 2
    nodes["offset"][interior + 1] = np.arange(leaves - 1)
    nodes["num_primitives_axis"][interior + 1] = 1 << 16
    nodes["offset"][-1], nodes["num_primitives_axis"][-1] = leaves - 1, 1 << 16
    recs = np.zeros(n, WIDE)
    recs["meta"] = 127 | 127 << 8 | 127 << 16 | 2 << 24
    recs["ref"][:, 0] = LEAF | np.arange(n, dtype=np.uint32)
    recs["ref"][:, 1] = np.arange(1, n + 1, dtype=np.uint32)
    recs["ref"][:, 2:] = EMPTY
    recs["ref"][n - 1, 1] = 0 if cycle else LEAF | n
    return nodes, recs


def test_two_hundred_thousand_records_in_a_chain_or_a_cycle_are_refused_not_crashed_on():
    nodes, recs = long_chain(200_000, False)
    assert both(nodes, recs, 0) == "deep"
    nodes, recs = long_chain(200_000, True)
    assert both(nodes, recs, 0) == "twice"
    nodes, recs = long_chain(MAX_LEVELS, False)                                                 # the same assembly at the limit is taken
    assert both(nodes, recs, 0) is None
    nodes, recs = long_chain(MAX_LEVELS + 1, False)
    assert both(nodes, recs, 0) == "deep"


# ---- random single-word mutations --------------------------------------------------------------------------------------------------------------------------
def test_the_library_and_the_restatement_agree_on_random_mutations(small):
    nodes0, recs0, entry0 = small
    # three small folds; the third carries a second, unreached copy of every record, so that a ref can move to "another valid, unused target"
    nodes1 = two_triangle_leaves(24, "balanced", 81)
    recs1, entry1 = wide_of(nodes1)
    nodes2 = two_triangle_leaves(33, "random", 82)
    recs2, entry2 = wide_of(nodes2, 2)
    recs2 = np.concatenate([recs2, recs2])
    half = len(recs2) // 2
    folds = [(nodes0, recs0, entry0, 0), (nodes1, recs1, entry1, 0), (nodes2, recs2, entry2, half)]
    for nodes, recs, entry, _ in folds:
        assert both(nodes, recs, entry) is None
    rng = np.random.default_rng(20240)
    REF0, META = 10, 3                                                                         # words of a record: origin 0..2, meta 3, refs 10..13
    taken = refused = 0
    classes = collections.Counter()
    for i in range(2400):
        nodes, recs, entry, half = folds[i % 3]
        words = recs.copy().view(np.uint32).reshape(len(recs), 16)
        n_tris = 2 * int(_trees.is_leaf(nodes).sum())
        r = int(rng.integers(len(recs)))
        kind = int(rng.integers(10))
        k = REF0 + int(rng.integers(4))
        a = int(rng.integers(3))
        if kind == 0:
            words[r, k] = rng.integers(0, 2 ** 32, dtype=np.uint64)
        elif kind == 1:
            words[r, k] = rng.integers(len(recs))
        elif kind == 2:
            words[r, k] = LEAF | int(rng.integers(n_tris + 2))
        elif kind == 3:
            words[r, k] = EMPTY
        elif kind == 4 and half and int(words[r, k]) < half:                                  # a record ref moves to that record's unreached copy
            words[r, k] += half
        elif kind in (4, 5):
            words[r, META] ^= 1 << int(rng.integers(32))
        elif kind == 6:
            words[r, META] = (int(words[r, META]) & ~(0xFF << (8 * a))) | int(rng.integers(256)) << (8 * a)
        elif kind in (7, 8):
            words[r, a] ^= 1 << int(rng.integers(32))
        else:
            words[r, a] = rng.integers(0, 2 ** 32, dtype=np.uint64)
        bad = words.view(WIDE).reshape(-1)
        want = restated(nodes, bad, entry)
        assert library(nodes, bad, entry) == want, (i, kind, r, k, a, want)
        taken += want is None
        refused += want is not None
        classes[want] += 1
    # neither side passes by always saying the same: the restatement alone takes a tenth and refuses a tenth
    assert taken >= 240 and refused >= 240, classes
    assert len(classes) >= 7, classes


def test_the_same_defects_made_of_a_golden_scenes_folds(golden_scenes):
    """the table above on the "coverage" scene's folds (leaves of several sizes), the closest-hit rays' and the shadow rays' own tree's: what
    tests/test_gpu_import_folds.py hands to a context, checked here without one"""
    nodes = golden_scenes["coverage"]["nodes"]
    d = light_dir()
    other = wide_of(golden_scenes["cornell"]["nodes"])
    for recs, entry in (wide_of(nodes), wide_metric(own_tree(nodes, 0.5, [d]), 0.5, [d])):
        assert both(nodes, recs, entry) is None
        for name, bad, bad_entry, cls in defects(nodes, recs, entry, other):
            said = both(nodes, bad, bad_entry)
            assert said is not None and (cls is None or said == cls), (name, said, cls)
