"""The UV atlas's rule (raytracing_amd/csrc/atlas.h) without a GPU: rt_debug_atlas(NULL, ...) -- the host restatement -- byte for byte
against a restatement in Python integers written from the rule's text.  Python's int is exact; np.float32(np.float64(w) / np.float64(A)) is the one binary64
divide and the one rounding to binary32 of bc.  tests/test_gpu_atlas.py runs the same cases through the kernels."""
import ctypes as C
import numpy as np
import pytest
from raytracing_amd import capi, scenes as S, types as T

f32 = np.float32
INVALID = 0xFFFFFFFF
NEIGHBOURS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]


# ---- the rule, in Python integers

def snap(uv, width, height):
    """the six snapped coordinates of a triangle as ints, or None when it is skipped"""
    out = []
    for k in range(6):
        c = f32(uv[k])
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.rint(c * f32(256 * (width if k % 2 == 0 else height)))
        if not np.isfinite(c) or not np.isfinite(r) or abs(float(r)) > 2.0 ** 24:
            return None
        out.append(int(r))
    return out


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def owns(dx, dy):
    return dy > 0 or (dy == 0 and dx < 0)


def py_cover(uv, width, height, gutter=0, object=None, ids=None):
    """(texels, stats dict) by the text of atlas.h"""
    uv = np.asarray(uv, f32).reshape(-1, 6)
    n = width * height
    owner, count = [INVALID] * n, [0] * n
    bc = {}
    st = dict(covered=0, overlapped=0, gutter=0, triangles_skipped=0, triangles_without_texel=0, triangles_filtered=0)
    for i, q in enumerate(uv):
        if object is not None and ids[i] != object:
            st["triangles_filtered"] += 1
            continue
        c = snap(q, width, height)
        if c is None:
            st["triangles_skipped"] += 1
            continue
        xs, ys = c[0::2], c[1::2]
        A = edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2])
        if A == 0:
            st["triangles_skipped"] += 1
            continue
        s = 1 if A > 0 else -1
        # the centres 256 x + 128 within the corners' box, clamped to the atlas
        x0, x1 = max(-((-(min(xs) - 128)) // 256), 0), min((max(xs) - 128) // 256, width - 1)
        y0, y1 = max(-((-(min(ys) - 128)) // 256), 0), min((max(ys) - 128) // 256, height - 1)
        covered = 0
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                px, py = 256 * x + 128, 256 * y + 128
                w = [s * edge(xs[(k + 1) % 3], ys[(k + 1) % 3], xs[(k + 2) % 3], ys[(k + 2) % 3], px, py) for k in range(3)]
                ok = True
                for k in range(3):
                    a, b = (k + 1) % 3, (k + 2) % 3
                    if w[k] < 0 or (w[k] == 0 and not owns(s * (xs[b] - xs[a]), s * (ys[b] - ys[a]))):
                        ok = False
                if not ok:
                    continue
                assert sum(w) == abs(A)
                idx = y * width + x
                covered += 1
                count[idx] += 1
                if i < owner[idx]:
                    owner[idx] = i
                    bc[idx] = (f32(np.float64(w[1]) / np.float64(abs(A))), f32(np.float64(w[2]) / np.float64(abs(A))))
        if covered == 0:
            st["triangles_without_texel"] += 1
    tx = np.zeros(n, T.texel)
    tx["primitive_id"] = INVALID
    for idx in range(n):
        if count[idx]:
            tx[idx] = (bc[idx], owner[idx], min(count[idx], 65535), capi.TEXEL_COVERED)
            st["covered"] += 1
            st["overlapped"] += count[idx] > 1
    for _ in range(gutter):
        nxt = tx.copy()
        for idx in range(n):
            if tx[idx]["flags"] != 0:
                continue
            x, y = idx % width, idx // width
            for dx, dy in NEIGHBOURS:
                if 0 <= x + dx < width and 0 <= y + dy < height and tx[(y + dy) * width + x + dx]["flags"] != 0:
                    nxt[idx] = tx[(y + dy) * width + x + dx]
                    nxt[idx]["flags"], nxt[idx]["count"] = capi.TEXEL_GUTTER, 0
                    st["gutter"] += 1
                    break
        tx = nxt
    return tx, st


# ---- the cases (tests/test_gpu_atlas.py runs them too)

def triangles_of(uv, seed=0):
    """T.triangle records whose texcoord.xy are uv[n, 6], with positions and normals of their own"""
    uv = np.asarray(uv, f32).reshape(-1, 3, 2)
    rng = np.random.default_rng(seed)
    t = np.zeros(len(uv), T.triangle)
    for k, v in enumerate(("v1", "v2", "v3")):
        t[v]["texcoord"]["x"], t[v]["texcoord"]["y"] = uv[:, k, 0], uv[:, k, 1]
        for c in "xyz":
            t[v]["position"][c] = rng.uniform(-1, 1, len(uv)).astype(f32)
            t[v]["normal"][c] = rng.uniform(0.1, 1, len(uv)).astype(f32)
    return t


def flipped(tri):
    return [tri[0], tri[1], tri[4], tri[5], tri[2], tri[3]]


SQUARE_A, SQUARE_B = [0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]           # the unit square about the diagonal through every texel centre (x, x)
BELOW, ABOVE = [0, 0.4375, 1, 0.4375, 0.5, 0], [0, 0.4375, 1, 0.4375, 0.5, 1]     # a shared horizontal edge on the centres of row 3 of 8
HOLDS, MISSES = [0.05, 0.05, 0.07, 0.05, 0.06, 0.07], [0.2, 0.2, 0.21, 0.2, 0.2, 0.21]   # sub-texel at 8 x 8: about the centre of texel (0, 0), beside every centre
BEYOND = float(2 ** 25) / (256 * 8)                                    # snaps to 2^25 at 8 x 8


def random_triangles(n, seed, small=0.0):
    """n random UV triangles in [-0.1, 1.1]^2; a fraction `small` of them within two texel centres each way of a 64-texel atlas"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.1, 1.1, (n, 1, 2))
    size = np.where(rng.uniform(size=(n, 1, 1)) < small, 0.012, rng.uniform(0.05, 0.6, (n, 1, 1)))
    return (c + rng.uniform(-1, 1, (n, 3, 2)) * size).astype(f32).reshape(n, 6)


CASES = {
    "diagonal": ([SQUARE_A, SQUARE_B], 8, 8, {}),
    "diagonal_first_flipped": ([flipped(SQUARE_A), SQUARE_B], 8, 8, {}),
    "diagonal_second_flipped": ([SQUARE_A, flipped(SQUARE_B)], 8, 8, {}),
    "horizontal": ([BELOW, ABOVE], 8, 8, {}),
    "horizontal_first_flipped": ([flipped(BELOW), ABOVE], 8, 8, {}),
    "horizontal_second_flipped": ([BELOW, flipped(ABOVE)], 8, 8, {}),
    "sub_texel": ([HOLDS, MISSES], 8, 8, {}),
    "overlap": ([[0.1, 0.1, 0.9, 0.1, 0.5, 0.9], [0.1, 0.2, 0.9, 0.2, 0.5, 0.95], HOLDS], 8, 8, {}),
    "skipped": ([[0.1, 0.1, 0.5, 0.5, 0.9, 0.9], [np.nan, 0.1, 0.9, 0.1, 0.5, 0.9], [0.1, 0.1, BEYOND, 0.1, 0.5, 0.9], [0.1, np.inf, 0.9, 0.1, 0.5, 0.9], SQUARE_A], 8, 8, {}),
    "clamp": ([[-3, -2, 5, -2, 0.5, 6]], 130, 67, {}),
    "gutter0": ([HOLDS, [0.5, 0.5, 0.8, 0.5, 0.5, 0.8]], 8, 8, dict(gutter=0)),
    "gutter1": ([HOLDS, [0.5, 0.5, 0.8, 0.5, 0.5, 0.8]], 8, 8, dict(gutter=1)),
    "gutter4": ([HOLDS, [0.5, 0.5, 0.8, 0.5, 0.5, 0.8]], 13, 9, dict(gutter=4)),
    "object": ([SQUARE_A, SQUARE_B, [0.1, 0.1, 0.9, 0.1, 0.5, 0.9], MISSES], 8, 8, dict(object=1, ids=[0, 1, 1, 0])),
    "one_texel": ([SQUARE_A, SQUARE_B], 1, 1, {}),
    "random": (random_triangles(40, 3, 0.5), 16, 12, dict(gutter=2)),
}


def run(ctx, uv, width, height, gutter=0, object=None, ids=None, own=True):
    """debug_atlas on `uv`: as the triangles' own texcoords, or (own=False) as the override over triangles with other texcoords"""
    uv = np.asarray(uv, f32).reshape(-1, 6)
    if own:
        return capi.debug_atlas(ctx, triangles_of(uv), width, height, gutter, object, ids)
    return capi.debug_atlas(ctx, triangles_of(random_triangles(len(uv), 99)), width, height, gutter, object, ids, uv=uv)


def same_cover(got, want, what=""):
    tx, st = got
    wtx, wst = want
    wst = wst if isinstance(wst, dict) else {k: int(wst[k]) for k in wst.dtype.names if k != "reserved"}
    assert {k: int(st[k]) for k in wst} == wst, what
    assert tx.tobytes() == np.ascontiguousarray(wtx).tobytes(), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_restatement_equals_the_python_integers(name):
    uv, w, h, kw = CASES[name]
    want = py_cover(uv, w, h, **kw)
    same_cover(run(None, uv, w, h, **kw), want, name)
    same_cover(run(None, uv, w, h, own=False, **kw), want, name + " (uv override)")
    assert (run(None, uv, w, h, **kw)[1]["reserved"] == 0).all()


@pytest.mark.parametrize("name", ["diagonal", "diagonal_first_flipped", "diagonal_second_flipped", "horizontal", "horizontal_first_flipped", "horizontal_second_flipped"])
def test_a_shared_edge_through_centres_gives_each_centre_to_one_triangle(name):
    uv, w, h, _ = CASES[name]
    tx, st = run(None, uv, w, h)
    covered = tx["flags"] == capi.TEXEL_COVERED
    assert (tx["count"][covered] == 1).all() and st["overlapped"] == 0
    if name.startswith("diagonal"):
        assert covered.all() and st["covered"] == 64                       # the square is the atlas: no centre lost on the diagonal or at the rim's owning edges
        assert set(tx["primitive_id"]) == {0, 1}
    else:
        row = tx.reshape(8, 8)[3]                                          # the centres the shared edge passes through (its end points' own centres aside)
        assert (row["count"][1:7] == 1).all() and len(set(row["primitive_id"][1:7])) == 1


def test_sub_texel_overlap_skip_and_clamp_counts():
    tx, st = run(None, *CASES["sub_texel"][:3])
    assert st["covered"] == 1 and st["triangles_without_texel"] == 1 and tx[0]["primitive_id"] == 0
    tx, st = run(None, *CASES["overlap"][:3])
    both = tx["count"] == 2
    assert both.any() and (tx["primitive_id"][both] == 0).all() and st["overlapped"] == int((tx["count"] > 1).sum())
    assert tx[0]["count"] == 1 and tx[0]["primitive_id"] == 2
    tx, st = run(None, *CASES["skipped"][:3])
    assert st["triangles_skipped"] == 4 and set(tx["primitive_id"]) <= {4, INVALID}
    tx, st = run(None, *CASES["clamp"][:3])
    assert st["covered"] > 0 and tx.reshape(67, 130)[0, 64]["count"] == 1 and st["triangles_without_texel"] == 0


def test_gutter_grows_by_one_ring_a_pass_and_never_rewrites_a_record():
    uv, w, h, _ = CASES["gutter4"]
    base, _ = run(None, uv, w, h)
    before = base
    for passes in (1, 2, 3, 4):
        tx, st = run(None, uv, w, h, gutter=passes)
        kept = before["flags"] != 0
        assert tx[kept].tobytes() == before[kept].tobytes()
        new = (tx["flags"] != 0) & ~kept
        assert new.any() and (tx["flags"][new] == capi.TEXEL_GUTTER).all() and (tx["count"][new] == 0).all()
        assert st["gutter"] == int((tx["flags"] == capi.TEXEL_GUTTER).sum()) and st["covered"] == int((base["flags"] == 1).sum())
        before = tx


def test_object_filter_counts_the_others_and_nothing_else():
    uv, w, h, kw = CASES["object"]
    tx, st = run(None, uv, w, h, **kw)
    assert st["triangles_filtered"] == 2 and st["triangles_without_texel"] == 0 and set(tx["primitive_id"]) <= {1, 2, INVALID}


def test_surfaces_are_query_surface_of_the_texels_with_zero_direction():
    uv = np.asarray(CASES["overlap"][0], f32)
    tris = triangles_of(uv, seed=4)
    ids = np.array([5, 6, 7], np.uint32)
    tx, _ = capi.debug_atlas(None, tris, 8, 8, gutter=1)
    sf = capi.atlas_surfaces_host(tris, tx, ids)
    miss = tx["primitive_id"] == INVALID
    assert miss.any() and (~miss).any()
    assert (sf["primitive_id"][miss] == INVALID).all() and (sf["flags"][miss] == 0).all() and not sf["position"][miss].any()
    assert (sf["flags"][~miss] == 1).all() and (sf["t"][~miss] == 0).all() and (sf["object"][~miss] == ids[tx["primitive_id"][~miss]]).all()
    for i in np.flatnonzero(~miss):                                        # query.h: p1 w0 + p2 bu + p3 bv, w0 = 1 - bu - bv, binary32, left to right
        t, (bu, bv) = tris[tx[i]["primitive_id"]], tx[i]["bc"]
        w0 = f32(f32(1) - bu) - bv
        for k, c in enumerate("xyz"):
            assert sf[i]["position"][k] == f32(f32(t["v1"]["position"][c] * w0) + f32(t["v2"]["position"][c] * bu)) + f32(t["v3"]["position"][c] * bv)
        assert np.array_equal(sf[i]["texcoord"], [f32(f32(t["v1"]["texcoord"][c] * w0) + f32(t["v2"]["texcoord"][c] * bu)) + f32(t["v3"]["texcoord"][c] * bv) for c in "xy"])


def test_synthetic_atlas_of_the_golden_cornell_scene(golden_scenes):
    tris = golden_scenes["cornell"]["triangles"]
    columns, rows = S.synthetic_atlas_grid(len(tris), 1, 1)
    assert columns * rows * 2 >= len(tris)
    for w, h in ((2 * columns, 2 * rows), (6 * columns, 6 * rows)):         # two texels a cell each way: the least at which each half holds a centre
        assert S.synthetic_atlas_grid(len(tris), w, h) == (columns, rows)   # (the grid follows the atlas's aspect: these sizes keep it)
        uv = S.synthetic_atlas(tris, w, h)
        assert uv.shape == (len(tris), 6) and uv.dtype == f32 and uv.min() >= 0 and uv.max() <= 1
        tx, st = capi.debug_atlas(None, tris, w, h, uv=uv)
        assert st["overlapped"] == 0 and st["triangles_skipped"] == 0 and st["triangles_without_texel"] == 0
        assert st["covered"] == (len(tris) // 2) * (w // columns) * (h // rows) + (len(tris) % 2) * int((tx["primitive_id"] == len(tris) - 1).sum())
        assert (np.bincount(tx["primitive_id"][tx["flags"] == 1], minlength=len(tris)) > 0).all()
    # at one texel per cell the diagonal passes through the only centre: one half of every cell goes without
    _, st = capi.debug_atlas(None, tris, columns, rows, uv=S.synthetic_atlas(tris, columns, rows))
    assert st["overlapped"] == 0 and st["triangles_without_texel"] == len(tris) // 2


# ---- refusals

def refused(match, fn, *a, **k):
    with pytest.raises(capi.RtError, match=match):
        fn(*a, **k)


def test_the_debug_form_refuses_with_the_familys_messages():
    tris = triangles_of([SQUARE_A])
    for w, h in ((0, 8), (8, 0), (16385, 1), (1, 16385), (16384, 8192)):
        refused("rt_debug_atlas: width and height must be 1 .. 16384 with width \\* height <= 2\\^26", capi.debug_atlas, None, tris, w, h)
    refused("rt_debug_atlas: gutter must be 0 .. 4", capi.debug_atlas, None, tris, 8, 8, gutter=5)
    refused("rt_debug_atlas: desc.object needs object_of_triangle", capi.debug_atlas, None, tris, 8, 8, object=0)
    refused("six floats per triangle", capi.debug_atlas, None, tris, 8, 8, uv=np.zeros(5, f32))
    lib = capi.load()
    d, tx = capi.atlas_desc(8, 8), np.zeros(64, T.texel)
    assert lib.rt_debug_atlas(None, tris.ctypes.data, 1, None, None, None, tx.ctypes.data, None) != 0
    assert lib.rt_last_error(None).decode() == "rt_debug_atlas: NULL argument"
    assert lib.rt_debug_atlas(None, tris.ctypes.data, 1, None, None, C.byref(d), None, None) != 0
    assert lib.rt_debug_atlas(None, None, 1, None, None, C.byref(d), tx.ctypes.data, None) != 0
    assert lib.rt_debug_atlas(None, tris.ctypes.data, 1, None, None, C.byref(d), tx.ctypes.data, None) == 0          # stats may be NULL
    assert capi.debug_atlas(None, tris[:0], 4, 4)[1]["covered"] == 0                                                 # no triangles: an empty atlas


def test_the_scene_forms_refuse_a_null_context():
    lib = capi.load()
    d, bd = capi.atlas_desc(8, 8), capi.bake_desc(16)
    calls = {
        "rt_scene_atlas": lambda: lib.rt_scene_atlas(None, C.byref(d), None, None, None),
        "rt_scene_atlas_buffer": lambda: lib.rt_scene_atlas_buffer(None, C.byref(d), None, None, None),
        "rt_scene_atlas_surfaces": lambda: lib.rt_scene_atlas_surfaces(None, None, 1, None),
        "rt_scene_atlas_surfaces_buffer": lambda: lib.rt_scene_atlas_surfaces_buffer(None, None, 1, None),
        "rt_scene_atlas_bake": lambda: lib.rt_scene_atlas_bake(None, C.byref(d), None, C.byref(bd), None, None, None),
    }
    for name, call in calls.items():
        assert call() != 0 and lib.rt_last_error(None).decode() == name + ": ctx is NULL"
