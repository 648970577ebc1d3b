"""The layers above rt_scene_set_skin / rt_scene_skin as far as they go without a GPU: host.Scene(arrays=, skin=) carries the influences
through the BVH build into the built order and leaves the triangles' bytes alone; the bindings exist with the right arities; and without a device a Render --
and with it set_skin -- fails loudly instead of falling back."""
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T
from tests.test_refit import positions


def arrays_of(sc):
    return {k: sc[k] for k in ("triangles", "materials", "textures", "texture_data")}


def built(arrays, **kw):
    s = host.Scene(arrays=arrays, **kw)
    s.set_env_image(np.zeros((2, 2, 4), np.float32))
    before = s.arrays()["triangles"].copy()
    s.build_bvh()
    s.finalize()
    return s, before


def test_scene_carries_the_influences_into_bvh_order(golden_scenes):
    arrays = arrays_of(golden_scenes["cornell"])
    n = len(arrays["triangles"])
    arrays["triangles"] = tris = arrays["triangles"][np.random.default_rng(4).permutation(n)]     # the golden scene is in built order already: out of it
    bones, weights = S.synthetic_skin(tris, 5)
    # make every corner's record its own: slot 3 (weight 0) names the triangle, slot 2 the corner
    bones = bones.copy()
    bones[..., 3] = np.arange(n)[:, None]
    bones[..., 2] = np.arange(3)[None, :]
    s, before = built(arrays, skin=(bones, weights))
    assert s.num_bones() == int(bones.max()) + 1
    after = s.arrays()["triangles"]
    got = s.triangle_skin()
    assert got.shape == (n, 3) and got.dtype == T.skin_influence
    src = got["bone"][:, 0, 3].astype(np.int64)                # the source triangle of every built triangle
    assert sorted(src.tolist()) == list(range(n)) and (src != np.arange(n)).any()          # a permutation, and the build did reorder
    assert after.tobytes() == tris[src].tobytes()              # ... the one the triangles themselves went through
    assert got.tobytes() == T.influences(bones, weights)[src].tobytes()
    # against the positions: the weights are synthetic_skin's of the BUILT triangles' own corners
    again = T.influences(*S.synthetic_skin(after, 5))
    assert got["weight"].tobytes() == again["weight"].tobytes() and (got["bone"][..., :2] == again["bone"][..., :2]).all()
    assert positions(after).tobytes() == positions(tris)[src].tobytes()
    # the triangles' bytes are those of the same scene built without a skin: before the build up to the index that rides in padding[1], after Finalize() entirely
    plain, plain_before = built(arrays)
    assert len(plain.triangle_skin()) == 0 and plain.num_bones() == 0
    assert plain.arrays()["triangles"].tobytes() == after.tobytes()
    raw_on, raw_off = before.view(np.uint32).reshape(-1, 40).copy(), plain_before.view(np.uint32).reshape(-1, 40)
    assert raw_on[:, 38].tolist() == list(range(n)) and (raw_off[:, 38] == 0).all()
    raw_on[:, 38] = 0
    assert raw_on.tobytes() == raw_off.tobytes()
    assert (after.view(np.uint32).reshape(-1, 40)[:, 37:] == 0).all()
    # objects and a skin ride together
    both, _ = built(arrays, objects=np.arange(n, dtype=np.uint32), skin=(bones, weights))
    assert both.triangle_objects().tolist() == src.tolist() and both.triangle_skin().tobytes() == got.tobytes()
    assert both.arrays()["triangles"].tobytes() == after.tobytes()


def test_scene_refuses_a_skin_it_cannot_take(golden_scenes):
    arrays = arrays_of(golden_scenes["cornell"])
    bones, weights = S.synthetic_skin(arrays["triangles"], 3)
    with pytest.raises(host.RtError, match="one row of three corners per triangle"):
        host.Scene(arrays=arrays, skin=(bones[:-1], weights[:-1]))
    with pytest.raises(host.RtError, match=r"\[n, 3, 4\]"):
        host.Scene(arrays=arrays, skin=(bones[:, :2], weights[:, :2]))
    with pytest.raises(host.RtError, match="skin= needs arrays="):
        host.Scene("assets/CornellBox.obj", skin=(bones, weights))
    lib = host.load()
    s = host.Scene(arrays=arrays)
    f = np.ascontiguousarray(T.influences(bones, weights))
    assert lib.rth_scene_set_triangle_skin(s.handle, f.ctypes.data, len(f) - 1) != 0
    assert b"three influences per triangle" in lib.rth_last_error()


def test_bindings_exist_with_the_right_arities():
    lib = capi.load()
    for name, n in (("rt_scene_set_skin", 4), ("rt_scene_skin", 3), ("rt_debug_skin", 7)):
        fn = getattr(lib, name)
        assert name in capi.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == n, name
    assert callable(capi.Context.set_skin) and callable(capi.Context.skin_scene) and callable(capi.debug_skin)
    hl = host.load()
    for name, n in (("rth_render_set_skin", 4), ("rth_render_skin", 3), ("rth_scene_set_triangle_skin", 3), ("rth_scene_num_triangle_skin", 1),
                    ("rth_scene_triangle_skin", 1)):
        assert name in host.EXPORTS and len(getattr(hl, name).argtypes) == n, name
    assert callable(host.Render.set_skin) and callable(host.Render.skin) and callable(host.Scene.triangle_skin)


def test_without_a_device_set_skin_fails_loudly(golden_scenes):
    """no GPU: there is no Render to skin, and that is an RtError that says so; with one: set_skin on a scene that was not uploaded refittable is the
    library's refusal.  Either way nothing falls back to the host."""
    arrays = arrays_of(golden_scenes["cornell"])
    s, _ = built(arrays, skin=S.synthetic_skin(arrays["triangles"], 4))
    try:
        r = host.Render(32, 32, s)
    except host.RtError as e:
        assert "HIP" in str(e)
        return
    try:
        with pytest.raises(host.RtError, match="rt_scene_set_skin: RT_CTX_OPT_REFITTABLE was off"):
            r.set_skin()
    finally:
        r.close()
