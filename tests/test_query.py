"""Ray queries without a device: the surface record's arithmetic -- rt_debug_query_surface(NULL, ...), the host restatement that
k_query_surface shares (raytracing_amd/csrc/query.h) -- against numpy in binary32, bit for bit; the record's layout; the refusals that need no GPU.
tests/test_gpu_query.py compares the kernels with this restatement and the walk with the oracle's."""
import ctypes as C
import numpy as np
import pytest
from raytracing_amd import capi, types as T

f32 = np.float32
INVALID = 0xFFFFFFFF


def pos(tris, k):
    return np.stack([tris[k]["position"][c] for c in "xyz"], -1).astype(f32)


def nrm(tris, k):
    return np.stack([tris[k]["normal"][c] for c in "xyz"], -1).astype(f32)


def uv(tris, k):
    return np.stack([tris[k]["texcoord"][c] for c in "xy"], -1).astype(f32)


def np_surface(tris, rays, hits, ids=None):
    """section 7h's arithmetic in numpy, every operation a binary32 one in the stated order"""
    out = np.zeros(len(hits), T.surface)
    out["primitive_id"] = INVALID
    prim = hits["primitive_id"]
    hit = prim < len(tris)
    t = tris[np.where(hit, prim, 0)] if len(tris) else np.zeros(len(hits), T.triangle)
    bu, bv = hits["bc"]["x"].astype(f32)[:, None], hits["bc"]["y"].astype(f32)[:, None]
    w0 = (f32(1.0) - bu) - bv
    blend = lambda a, b, c: (a * w0 + b * bu) + c * bv
    position = blend(pos(t, "v1"), pos(t, "v2"), pos(t, "v3"))
    texcoord = blend(uv(t, "v1"), uv(t, "v2"), uv(t, "v3"))
    n = blend(nrm(t, "v1"), nrm(t, "v2"), nrm(t, "v3"))
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        shading = n / ln[:, None]
        a, b = pos(t, "v2") - pos(t, "v1"), pos(t, "v3") - pos(t, "v1")
        g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
        l2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ok = (l2 > 0) & np.isfinite(l2)
        geo = np.where(ok[:, None], g / np.sqrt(l2)[:, None], f32(0.0)).astype(f32)
        d = np.stack([rays["direction"][c] for c in "xyz"], -1).astype(f32)
        facing = (d[:, 0] * geo[:, 0] + d[:, 1] * geo[:, 1]) + d[:, 2] * geo[:, 2]
    for name, v in (("position", position), ("geometric_normal", geo), ("shading_normal", shading), ("texcoord", texcoord)):
        out[name][hit] = v[hit]
    out["primitive_id"][hit] = prim[hit]
    out["mtl_index"][hit] = t["mtl_index"][hit]
    out["object"][hit] = ids[prim[hit]] if ids is not None else INVALID
    out["t"][hit] = hits["t"][hit]
    out["flags"][hit] = 1 | np.where(facing[hit] > 0, 2, 0)
    return out


def random_case(rng, n, n_tris=37):
    tris = np.zeros(n_tris, T.triangle)
    for v in ("v1", "v2", "v3"):
        for c in "xyz":
            tris[v]["position"][c] = rng.normal(size=n_tris).astype(f32) * f32(3.0)
            tris[v]["normal"][c] = rng.normal(size=n_tris).astype(f32)
        for c in "xy":
            tris[v]["texcoord"][c] = rng.uniform(-2, 2, n_tris).astype(f32)
    tris["mtl_index"] = rng.integers(0, 9, n_tris)
    tris[1]["v3"] = tris[1]["v2"]                                   # a degenerate (zero-area) triangle: the geometric normal is zeros
    for c in "xyz":
        tris[2]["v2"]["normal"][c] = tris[2]["v1"]["normal"][c]     # a blend that cancels to zero at bu = 0, bv = 0.5 (below): a NaN shading normal,
        tris[2]["v3"]["normal"][c] = -tris[2]["v1"]["normal"][c]    # as the guide pass's is
    rays = np.zeros(n, T.ray)
    for c in "xyz":
        rays["origin"][c] = rng.normal(size=n).astype(f32)
        rays["direction"][c] = rng.normal(size=n).astype(f32)
    hits = np.zeros(n, T.hit)
    hits["primitive_id"] = rng.integers(0, n_tris, n)
    u = rng.uniform(0, 1, n)
    hits["bc"]["x"] = (u * rng.uniform(0, 1, n)).astype(f32)
    hits["bc"]["y"] = ((1 - u) * rng.uniform(0, 1, n)).astype(f32)
    hits["t"] = rng.uniform(0.1, 50, n).astype(f32)
    special = [(1, 0.25, 0.25), (2, 0.0, 0.5), (INVALID, 0.3, 0.3), (n_tris, 0.1, 0.1)]      # degenerate, zero blend, a miss, an index past the array (a miss)
    for k, (p, bu, bv) in enumerate(special[:n] if n < len(special) else special):
        i = (k * 7) % n if n >= len(special) else k
        hits[i] = ((bu, bv), p, hits[i]["t"])
    ids = rng.integers(0, 5, n_tris).astype(np.uint32)
    return tris, rays, hits, ids


@pytest.mark.parametrize("with_objects", [False, True], ids=["no_objects", "objects"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_host_restatement_equals_numpy_bit_for_bit(n, with_objects):
    rng = np.random.default_rng(700 + n)
    rounds = 4 if n == 1 else 1                                    # n = 1 holds one special case per round
    for k in range(rounds):
        tris, rays, hits, ids = random_case(rng, n)
        if n == 1:
            hits[0] = [((0.25, 0.25), 1, 2.0), ((0.0, 0.5), 2, 2.0), ((0.3, 0.3), INVALID, 2.0), ((0.2, 0.3), 5, 2.0)][k]
        got = capi.debug_query_surface(None, tris, rays, hits, ids if with_objects else None)
        want = np_surface(tris, rays, hits, ids if with_objects else None)
        assert got.tobytes() == want.tobytes(), [name for name in T.surface.names if got[name].tobytes() != want[name].tobytes()]
        miss = hits["primitive_id"] >= len(tris)
        assert (got["flags"][~miss] & 1).all() and not got["flags"][miss].any()
        assert got[miss].tobytes() == np_surface(tris, rays[miss], hits[miss]).tobytes()       # a miss: the id and zeros, objects or not
        deg = hits["primitive_id"] == 1
        assert not got["geometric_normal"][deg].any()
        zero = (hits["primitive_id"] == 2) & (hits["bc"]["x"] == 0) & (hits["bc"]["y"] == 0.5)
        assert np.isnan(got["shading_normal"][zero]).all()


def test_rays_as_float_rows_equal_ray_records():
    rng = np.random.default_rng(3)
    tris, rays, hits, ids = random_case(rng, 65)
    rows = rays.view(f32).reshape(-1, 8)
    assert capi.debug_query_surface(None, tris, rows, hits, ids).tobytes() == capi.debug_query_surface(None, tris, rays, hits, ids).tobytes()
    with pytest.raises(capi.RtError, match="float32\\[n, 8\\]"):
        capi.ray_records(np.zeros((4, 6), f32))


def test_surface_record_layout():
    assert T.surface.itemsize == 64
    want = dict(position=0, primitive_id=12, geometric_normal=16, mtl_index=28, shading_normal=32, object=44, texcoord=48, t=56, flags=60)
    assert {k: T.surface.fields[k][1] for k in T.surface.names} == want
    header = open(capi._HERE + "/../include/rt_hip.h").read()
    assert "RT_STATIC_ASSERT(sizeof(rt_surface) == 64" in header
    for name in ("rt_scene_trace", "rt_scene_trace_buffer", "rt_frame_pick", "rt_debug_query_surface"):
        assert name in capi.EXPORTS and hasattr(capi.load(), name)


def test_refusals_without_a_device():
    lib = capi.load()
    rays, hits, occ, surf = np.zeros(4, T.ray), np.zeros(4, T.hit), np.zeros(4, np.uint32), np.zeros(4, T.surface)
    err = lambda: lib.rt_last_error(None).decode()
    assert lib.rt_scene_trace(None, rays.ctypes.data, 4, capi.QUERY_CLOSEST, hits.ctypes.data, None, None) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_trace(None, None, 0, capi.QUERY_CLOSEST, None, None, None) != 0 and "ctx is NULL" in err()
    assert lib.rt_scene_trace_buffer(None, None, 4, capi.QUERY_ANY_HIT, None, None, None) != 0 and "ctx is NULL" in err()
    assert lib.rt_frame_pick(None, 0, 0, rays.ctypes.data, hits.ctypes.data, surf.ctypes.data) != 0 and "frame is NULL" in err()
    tris = np.zeros(3, T.triangle)
    assert lib.rt_debug_query_surface(None, tris.ctypes.data, 3, None, None, hits.ctypes.data, 4, surf.ctypes.data) != 0 and "NULL argument" in err()
    assert lib.rt_debug_query_surface(None, tris.ctypes.data, 3, None, rays.ctypes.data, hits.ctypes.data, 4, None) != 0 and "NULL argument" in err()
    assert lib.rt_debug_query_surface(None, None, 0, None, None, None, 0, None) == 0          # n == 0 does nothing
    assert hits.tobytes() == bytes(hits.nbytes) and occ.tobytes() == bytes(occ.nbytes) and surf.tobytes() == bytes(surf.nbytes)   # nothing was written
    with pytest.raises(capi.RtError, match="one hit per ray"):
        capi.debug_query_surface(None, tris, rays, hits[:3])
    # the context-taking calls: without a device there is no context to take, and that is said loudly; with one, a context without a scene refuses the query
    try:
        ctx = capi.Context(0)
    except capi.RtError as e:
        assert "no HIP device" in str(e)
        return
    try:
        with pytest.raises(capi.RtError, match="no scene uploaded"):
            ctx.trace(rays)
    finally:
        ctx.close()
