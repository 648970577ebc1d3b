"""The layers above rt_scene_set_morph / rt_scene_morph / rt_scene_morph_skin as far as they go without a GPU: types.morph_targets packs
sparse targets, scenes.synthetic_morph makes crack-free bounded ones deterministically, the bindings exist with the right arities, and without a device a Render
-- and with it set_morph -- fails loudly instead of falling back."""
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_refit import positions
from tests.test_skin_layers import arrays_of, built

f32 = np.float32


def test_morph_targets_packs_sparse_targets():
    dp = np.arange(12, dtype=np.float64).reshape(4, 3)
    deltas, offsets = T.morph_targets([([5, 2, 7, 0], dp, None), (np.zeros(0, np.int64), np.zeros((0, 3)), None), ([1], [[1, 2, 3]], [[0, 0, -1]])])
    assert deltas.dtype == T.morph_delta and deltas.itemsize == 32 and offsets.dtype == np.uint32
    assert offsets.tolist() == [0, 4, 4, 5]
    assert deltas["corner"].tolist() == [5, 2, 7, 0, 1] and (deltas["pad"] == 0).all()
    assert deltas["position"][:4].tolist() == dp.tolist() and (deltas["normal"][:4].view(np.uint32) == 0).all()
    assert deltas["normal"][4].tolist() == [0, 0, -1]
    raw = deltas.view(np.uint32).reshape(-1, 8)                   # the C layout: corner, position, normal, pad
    assert raw[4, 0] == 1 and raw[4, 1:4].view(f32).tolist() == [1, 2, 3] and raw[4, 4:7].view(f32).tolist() == [0, 0, -1] and raw[4, 7] == 0
    deltas, offsets = T.morph_targets([])
    assert len(deltas) == 0 and offsets.tolist() == [0]
    with pytest.raises(ValueError, match="one position delta"):
        T.morph_targets([([1, 2], [[0, 0, 0]], None)])
    with pytest.raises(ValueError, match="one position delta"):
        T.morph_targets([([1], [[0, 0, 0]], [[0, 0, 1], [0, 0, 1]])])
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        T.morph_targets([([-1], [[0, 0, 0]], None)])
    with pytest.raises(ValueError, match="corners, dpos, dnormal"):
        T.morph_targets([([1], [[0, 0, 0]])])


def test_synthetic_morph_is_deterministic_bounded_and_crack_free(golden_scenes):
    tris = golden_scenes["cornell"]["triangles"]
    n = len(tris)
    targets = S.synthetic_morph(tris, 5, radius=0.2)
    again = S.synthetic_morph(tris, 5, radius=0.2)
    assert len(targets) == 5
    P = positions(tris).reshape(-1, 3)
    diagonal = np.linalg.norm(P.max(0).astype(np.float64) - P.min(0))
    for (c, dp, dn), (c2, dp2, dn2) in zip(targets, again):
        assert c.tobytes() == c2.tobytes() and dp.tobytes() == dp2.tobytes() and dn.tobytes() == dn2.tobytes()
        assert dp.dtype == f32 and dn.dtype == f32 and dp.shape == dn.shape == (len(c), 3)
        assert len(c) > 0 and c.min() >= 0 and c.max() < 3 * n and (np.diff(c) > 0).all()           # in range, none twice
        assert len(c) < 3 * n                                                                     # a bounded region, not the whole mesh
        assert np.ptp(P[c].astype(np.float64), axis=0).max() <= 2 * 0.2 * diagonal * (1 + 1e-6)
        # corners that share a position share a delta, and every corner at a touched position is in the target
        key = {}
        for corner, d, m in zip(c.tolist(), dp, dn):
            k = P[corner].tobytes()
            assert key.setdefault(k, (d.tobytes(), m.tobytes())) == (d.tobytes(), m.tobytes())
        touched = set(key)
        assert all((P[corner].tobytes() in touched) == (corner in set(c.tolist())) for corner in range(3 * n))
    assert any(len(set(P[c].tobytes() for c in t[0].tolist())) < len(t[0]) for t in targets)     # shared positions do occur
    assert S.synthetic_morph(tris, 5, radius=0.2, normals=False)[0][2] is None
    other = S.synthetic_morph(tris, 5, radius=0.2, seed=1)
    assert other[0][0].tobytes() == targets[0][0].tobytes() and other[0][1].tobytes() != targets[0][1].tobytes()
    deltas, offsets = T.morph_targets(targets)
    w = np.linspace(-1, 1, 5).astype(f32)
    got = capi.debug_morph(None, tris, deltas, offsets, w)          # the library takes them, and shared corners stay together
    G = positions(got).reshape(-1, 3)
    where = {}
    for corner in range(3 * n):
        assert where.setdefault(P[corner].tobytes(), G[corner].tobytes()) == G[corner].tobytes()
    assert (G != P).any()
    with pytest.raises(ValueError, match="1 to 65536 targets"):
        S.synthetic_morph(tris, 0)
    with pytest.raises(ValueError, match="no triangles"):
        S.synthetic_morph(tris[:0], 3)


def test_bindings_exist_with_the_right_arities():
    lib = capi.load()
    for name, n in (("rt_scene_set_morph", 5), ("rt_scene_morph", 3), ("rt_scene_morph_skin", 5), ("rt_debug_morph", 8), ("rt_debug_morph_skin", 11)):
        fn = getattr(lib, name)
        assert name in capi.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == n, name
    assert callable(capi.Context.set_morph) and callable(capi.Context.morph_scene) and callable(capi.Context.morph_skin_scene)
    assert callable(capi.debug_morph) and callable(capi.debug_morph_skin)
    assert capi.MORPH_LDS_TARGETS == 1024 and capi.MORPH_MAX_TARGETS == 65536
    hl = host.load()
    for name, n in (("rth_render_set_morph", 5), ("rth_render_morph", 3), ("rth_render_morph_skin", 5)):
        assert name in host.EXPORTS and len(getattr(hl, name).argtypes) == n, name
    assert callable(host.Render.set_morph) and callable(host.Render.morph) and callable(host.Render.morph_skin)


def test_without_a_device_set_morph_fails_loudly(golden_scenes):
    """no GPU: there is no Render to morph, and that is an RtError that says so; with one: set_morph on a scene that was not uploaded refittable is the
    library's refusal.  Either way nothing falls back to the host."""
    arrays = arrays_of(golden_scenes["cornell"])
    s, _ = built(arrays)
    deltas, offsets = T.morph_targets(S.synthetic_morph(s.arrays()["triangles"], 3))
    try:
        r = host.Render(32, 32, s)
    except host.RtError as e:
        assert "HIP" in str(e)
        return
    try:
        with pytest.raises(host.RtError, match="rt_scene_set_morph: RT_CTX_OPT_REFITTABLE was off"):
            r.set_morph(deltas, offsets)
    finally:
        r.close()
