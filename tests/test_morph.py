"""The scene's triangles morphed from one weight per sparse morph target (raytracing_amd/csrc/morph.h, morph.hip), checked ON THE CPU
through the host restatement of the kernels' rule (rt_debug_morph with ctx = NULL):

  * against np_morph below, the same arithmetic in numpy binary32 with the same operation order, BIT FOR BIT in every lane (numpy rounds every binary32 product,
    sum, quotient and square root once, as the library does with contraction off);
  * all-zero weights return the rest pose byte for byte, a planted -0.0 included; a weight of -0.0 is skipped; position-only targets leave the normals' bytes
    alone; a normal that sums to zero length is left un-normalised; the order of the deltas inside a target does not matter; empty targets and a set with no
    deltas at all are legal;
  * rt_debug_morph_skin(NULL) is rt_debug_skin(NULL) of rt_debug_morph(NULL);
  * what is refused, with a message.

The device half is tests/test_gpu_morph.py."""
import numpy as np
import pytest
from raytracing_amd import capi, types as T
from tests.test_motion_filter import random_triangles
from tests.test_pose import decorated, same_bytes
from tests.test_skin import random_case as random_skin_case

f32 = np.float32
VERTS = ("v1", "v2", "v3")


def _lanes(tris, field):
    """float32[n, 3, 3]: (triangle, corner, coordinate) of `field` = "position" or "normal" """
    return np.stack([np.stack([tris[v][field][a] for a in "xyz"], -1) for v in VERTS], 1).astype(f32)


def same_words(got, want):
    """any two arrays of 32-bit lanes (a field of the triangles, say), word for word"""
    assert (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all()


def np_morph(rest, deltas, offsets, weights):
    """the restatement: targets in ascending order, each delta at its corner, morph.h's order of operations; a corner's normal renormalised once at the end"""
    w = np.asarray(weights, f32)
    P, N = _lanes(rest, "position"), _lanes(rest, "normal")
    touched = np.zeros(P.shape[:2], bool)
    with np.errstate(all="ignore"):
        for t in range(len(offsets) - 1):
            if w[t] == 0:                                           # +0 and -0
                continue
            d = deltas[offsets[t]:offsets[t + 1]]
            tri, c = d["corner"] // 3, d["corner"] % 3              # no corner twice in a target: the fancy assignment below is one write per corner
            P[tri, c] = P[tri, c] + w[t] * d["position"]
            normal = (np.ascontiguousarray(d["normal"]).view(np.uint32) != 0).any(1)
            tri, c, dn = tri[normal], c[normal], d["normal"][normal]
            N[tri, c] = N[tri, c] + w[t] * dn
            touched[tri, c] = True
        l = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        ok = touched & (l > 0) & np.isfinite(l)
        unit = N / np.sqrt(l)[..., None]
        assert P.dtype == f32 and unit.dtype == f32
        N = np.where(ok[..., None], unit, N)
    out = rest.copy()
    # (lanes of untouched corners are the input's bytes anyway: P and N started as copies)
    for k, v in enumerate(VERTS):
        for j, a in enumerate("xyz"):
            out[v]["position"][a] = P[:, k, j]
            out[v]["normal"][a] = N[:, k, j]
    return out


def random_targets(rng, n, n_targets, share=0.3, position_only=0.3, ordered=False):
    """n_targets sparse targets over n triangles, each moving about `share` of the 3 n corners (at least one where share > 0), a `position_only` part of them
    without normal deltas; inside a target the corners come in random order unless `ordered`"""
    targets = []
    for t in range(n_targets):
        k = min(3 * n, max(1, int(round(share * 3 * n)))) if share > 0 else 0
        corners = rng.permutation(3 * n)[:k]
        if ordered:
            corners = np.sort(corners)
        dp = rng.normal(0, 0.2, (k, 3)).astype(f32)
        dn = None if rng.uniform() < position_only else rng.normal(0, 0.5, (k, 3)).astype(f32)
        targets.append((corners, dp, dn))
    return targets


def random_case(rng, n, n_targets, **kw):
    """(triangles with every copied lane filled, deltas, offsets, weights); some weights are +0, some negative, none normalised"""
    tris = decorated(random_triangles(rng, n), rng)
    deltas, offsets = T.morph_targets(random_targets(rng, n, n_targets, **kw))
    w = rng.normal(0, 1, n_targets).astype(f32)
    w[rng.uniform(size=n_targets) < 0.2] = 0.0
    return tris, deltas, offsets, w


@pytest.mark.parametrize("n_targets", [1, 2, 7, 300])
@pytest.mark.parametrize("n", [1, 2, 63, 257])
def test_host_restatement_equals_numpy_bit_for_bit(n, n_targets):
    rng = np.random.default_rng(1000 * n + n_targets)
    tris, deltas, offsets, w = random_case(rng, n, n_targets, share=0.3 if n_targets < 300 else 0.02)
    w[0] = 0.75                                                   # something moves
    got = capi.debug_morph(None, tris, deltas, offsets, w)
    same_bytes(got, np_morph(tris, deltas, offsets, w))
    assert (_lanes(got, "position") != _lanes(tris, "position")).any()
    for v in VERTS:                                               # the copied lanes
        same_words(got[v]["texcoord"], tris[v]["texcoord"])
        same_words(got[v]["position"]["w"], tris[v]["position"]["w"])
        same_words(got[v]["normal"]["w"], tris[v]["normal"]["w"])


def test_zero_weights_return_the_rest_pose_byte_for_byte():
    rng = np.random.default_rng(5)
    tris, deltas, offsets, w = random_case(rng, 100, 5, share=1.0, position_only=0.0)
    tris["v2"]["position"]["y"][3] = -0.0                          # x + 0 * d would turn this into +0.0
    tris["v1"]["normal"]["z"][7] = -0.0
    tris["v3"]["normal"]["x"][9] = 2.5                             # and a renormalisation would shorten this one
    same_bytes(capi.debug_morph(None, tris, deltas, offsets, np.zeros(5, f32)), tris)
    same_bytes(capi.debug_morph(None, tris, deltas, offsets, np.array([0.0, -0.0, 0.0, -0.0, -0.0], f32)), tris)


def test_a_weight_of_negative_zero_is_skipped():
    rng = np.random.default_rng(6)
    tris, deltas, offsets, w = random_case(rng, 50, 4, share=1.0)
    w[:] = (0.5, -0.0, -1.25, 0.0)
    got = capi.debug_morph(None, tris, deltas, offsets, w)
    same_bytes(got, np_morph(tris, deltas, offsets, w))
    keep = np.concatenate([deltas[offsets[0]:offsets[1]], deltas[offsets[2]:offsets[3]]])       # the same morph without targets 1 and 3
    keep_offsets = np.array([0, offsets[1], offsets[1] + offsets[3] - offsets[2]], np.uint32)
    same_bytes(got, capi.debug_morph(None, tris, keep, keep_offsets, w[[0, 2]]))


def test_position_only_targets_leave_the_normals_bytes_alone():
    rng = np.random.default_rng(7)
    tris, deltas, offsets, w = random_case(rng, 80, 6, share=0.7, position_only=1.0)
    w[:] = rng.uniform(0.5, 2.0, 6)
    for a in "xyz":
        tris["v1"]["normal"][a][:] *= f32(3.0)                      # not unit: a renormalisation would show
    got = capi.debug_morph(None, tris, deltas, offsets, w)
    same_bytes(got, np_morph(tris, deltas, offsets, w))
    for v in VERTS:
        same_words(got[v]["normal"], tris[v]["normal"])
    assert (_lanes(got, "position") != _lanes(tris, "position")).any()


def test_a_normal_that_sums_to_zero_length_is_left_as_summed():
    rng = np.random.default_rng(8)
    tris = decorated(random_triangles(rng, 3), rng)
    for a, val in zip("xyz", (0.25, -0.5, 1.0)):
        tris["v2"]["normal"][a][1] = val
    deltas, offsets = T.morph_targets([([3 * 1 + 1], [[0.0, 0.0, 0.0]], [[-0.25, 0.5, -1.0]])])
    got = capi.debug_morph(None, tris, deltas, offsets, np.ones(1, f32))
    same_bytes(got, np_morph(tris, deltas, offsets, np.ones(1, f32)))
    assert all(got["v2"]["normal"][a][1] == 0 for a in "xyz")
    same_bytes(got[[0, 2]], tris[[0, 2]])


def test_the_order_inside_a_target_does_not_matter():
    rng = np.random.default_rng(9)
    tris = decorated(random_triangles(rng, 120), rng)
    targets = random_targets(rng, 120, 9, share=0.5, ordered=True)
    shuffled = []
    for corners, dp, dn in targets:
        p = rng.permutation(len(corners))
        shuffled.append((corners[p], dp[p], None if dn is None else dn[p]))
    w = rng.normal(0, 1, 9).astype(f32)
    a = capi.debug_morph(None, tris, *T.morph_targets(targets), w)
    b = capi.debug_morph(None, tris, *T.morph_targets(shuffled), w)
    same_bytes(a, b)
    same_bytes(a, np_morph(tris, *T.morph_targets(targets), w))


def test_an_empty_target_and_a_set_with_no_deltas():
    rng = np.random.default_rng(10)
    tris = decorated(random_triangles(rng, 40), rng)
    targets = random_targets(rng, 40, 3, share=0.4)
    w = np.array([0.5, 2.0, -1.0], f32)
    base = capi.debug_morph(None, tris, *T.morph_targets(targets), w)
    empty = (np.zeros(0, np.int64), np.zeros((0, 3), f32), None)
    with_empty = [targets[0], empty, targets[1], targets[2], empty]
    deltas, offsets = T.morph_targets(with_empty)
    assert list(np.diff(offsets.astype(np.int64)) == 0) == [False, True, False, False, True]
    same_bytes(capi.debug_morph(None, tris, deltas, offsets, np.array([0.5, 9.0, 2.0, -1.0, 9.0], f32)), base)
    deltas, offsets = T.morph_targets([empty, empty])
    assert len(deltas) == 0 and list(offsets) == [0, 0, 0]
    same_bytes(capi.debug_morph(None, tris, deltas, offsets, np.array([3.0, -4.0], f32)), tris)


def test_morph_then_skin_is_the_composition_of_the_two_restatements():
    rng = np.random.default_rng(11)
    tris, infl, mats = random_skin_case(rng, 130, 9)
    deltas, offsets = T.morph_targets(random_targets(rng, 130, 5, share=0.4))
    w = rng.normal(0, 1, 5).astype(f32)
    got = capi.debug_morph_skin(None, tris, deltas, offsets, w, infl, mats)
    same_bytes(got, capi.debug_skin(None, capi.debug_morph(None, tris, deltas, offsets, w), infl, mats))
    assert (_lanes(got, "position") != _lanes(capi.debug_skin(None, tris, infl, mats), "position")).any()


def _raw(tris, deltas, offsets, num_targets, num_triangles, weights, no_out=False):
    """rt_debug_morph itself, for the cases capi's wrapper would not let through; the message of a refusal, None when accepted"""
    lib = capi.load()
    out = None if no_out else np.zeros_like(tris)
    p = lambda x: None if x is None else x.ctypes.data
    rc = lib.rt_debug_morph(None, p(tris), p(deltas), p(offsets), num_targets, num_triangles, p(weights), p(out))
    return None if rc == 0 else lib.rt_last_error(None).decode()


def test_what_is_refused():
    rng = np.random.default_rng(12)
    tris, deltas, offsets, w = random_case(rng, 10, 3, share=0.5)
    n, k = len(tris), len(offsets) - 1
    assert _raw(tris, deltas, offsets, k, n, w) is None
    for missing in range(4):
        args = [tris, deltas, offsets, w]
        args[missing] = None
        assert _raw(args[0], args[1], args[2], k, n, args[3]) == "rt_debug_morph: NULL argument"
    assert _raw(tris, deltas, offsets, k, n, w, no_out=True) == "rt_debug_morph: NULL argument"
    assert _raw(tris, deltas, offsets, k, 0, w) == "rt_debug_morph: no triangles"
    assert _raw(tris, deltas, offsets, k, 2**31, w) == "rt_debug_morph: more than 1431655765 triangles (a corner index is 32 bits)"
    assert _raw(tris, deltas, offsets, 0, n, w) == "rt_debug_morph: no targets"
    assert _raw(tris, deltas, offsets, 65537, n, w) == "rt_debug_morph: more than 65536 targets"

    def with_(field, at, value, offs=None):
        d = deltas.copy()
        if field is not None:
            d[field][at] = value
        return _raw(tris, d, offsets if offs is None else np.asarray(offs, np.uint32), k, n, w)

    o = offsets.astype(np.int64)
    assert with_(None, 0, 0, [1, o[1], o[2], o[3]]) == "rt_debug_morph: target_offsets[0] is not 0"
    assert with_(None, 0, 0, [0, o[2], o[1], o[3]]) == "rt_debug_morph: target_offsets decrease"
    assert with_("corner", 2, 3 * n) == "rt_debug_morph: a corner is not below 3 * num_triangles"
    for field in ("position", "normal"):
        for bad in (np.inf, -np.inf, np.nan):
            assert with_(field, (4, 1), bad) == "rt_debug_morph: a delta is not finite"
    assert with_("pad", 1, 7) == "rt_debug_morph: a delta's pad is not 0"
    assert with_("corner", 1, deltas["corner"][0]) == "rt_debug_morph: a target moves the same corner twice"
    # the same corner in two different targets is what targets are for
    d = deltas.copy()
    d["corner"][o[1]] = d["corner"][0]
    clash = (d["corner"][o[1] + 1:o[2]] == d["corner"][0]).any()
    assert clash or _raw(tris, d, offsets, k, n, w) is None
    # the first offence in array order decides: a bad pad at delta 1 before a bad corner at delta 3, and the other way round
    d = deltas.copy()
    d["pad"][1], d["corner"][3] = 1, 3 * n
    assert _raw(tris, d, offsets, k, n, w) == "rt_debug_morph: a delta's pad is not 0"
    d = deltas.copy()
    d["corner"][1], d["pad"][3] = 3 * n, 1
    assert _raw(tris, d, offsets, k, n, w) == "rt_debug_morph: a corner is not below 3 * num_triangles"
    for bad in (np.inf, np.nan):
        bad_w = w.copy()
        bad_w[1] = bad
        assert _raw(tris, deltas, offsets, k, n, bad_w) == "rt_debug_morph: a weight is not finite"
    # the wrapper's own refusals
    with pytest.raises(capi.RtError, match="types.morph_delta"):
        capi.debug_morph(None, tris, np.zeros(4, np.float32), offsets, w)
    with pytest.raises(capi.RtError, match="one weight per target"):
        capi.debug_morph(None, tris, deltas, offsets, w[:2])
    with pytest.raises(capi.RtError, match="past the deltas"):
        capi.debug_morph(None, tris, deltas[:3], offsets, w)
    with pytest.raises(capi.RtError, match="past the deltas"):                     # ... also with no deltas at all
        capi.debug_morph(None, tris, deltas[:0], np.array([0, 5, 5, 5], np.uint32), w)
