"""The scene's objects posed from one 3x4 matrix per object (raytracing_amd/csrc/pose.h, pose.hip), checked ON THE CPU through the host
restatement of the kernel's rule (rt_debug_pose with ctx = NULL):

  * against np_pose below, the same arithmetic in numpy binary32 with the same operation order, BIT FOR BIT in every lane (numpy rounds every binary32 product,
    sum, quotient and square root once, as the library does with contraction off; no lane needed a looser comparison);
  * identity matrices return the input bytes;
  * what is refused, with a message.

The device half is tests/test_gpu_pose.py."""
import os
import numpy as np
import pytest
from raytracing_amd import capi
from tests.test_refit import positions
from tests.test_motion_filter import random_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)


def translation(dx, dy, dz):
    m = IDENTITY.copy()
    m[:, 3] = (dx, dy, dz)
    return m


def rotation(axis, angle, pivot=(0.0, 0.0, 0.0)):
    a = np.array(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    p = np.array(pivot, np.float64)
    return np.concatenate([R, (p - R @ p)[:, None]], 1).astype(f32)


def scale(sx, sy, sz):
    m = np.zeros((3, 4), f32)
    m[0, 0], m[1, 1], m[2, 2] = sx, sy, sz
    return m


MIRROR = scale(-1.0, 1.0, 1.0)                                                      # det < 0
RANK2 = np.array([[1, 2, 3, 0.5], [2, 4, 6, -1], [0.5, -1, 0.25, 2]], f32)          # row y = 2 row x: det = 0
MATRICES = {"identity": IDENTITY, "translation": translation(0.3, -1.25, 7.0), "rotation": rotation((1, 2, -0.5), 0.7, (0.2, 0.1, -0.4)),
            "scale": scale(0.5, 3.0, 1.75), "mirror": MIRROR, "rank2": RANK2}


def np_object(m):
    """pose.h's make_object: cofactors a b - c d in its order, det along the first row, all in binary32"""
    m = np.asarray(m, f32).reshape(12)
    c = np.array([m[5] * m[10] - m[6] * m[9], m[6] * m[8] - m[4] * m[10], m[4] * m[9] - m[5] * m[8],
                  m[2] * m[9] - m[1] * m[10], m[0] * m[10] - m[2] * m[8], m[1] * m[8] - m[0] * m[9],
                  m[1] * m[6] - m[2] * m[5], m[2] * m[4] - m[0] * m[6], m[0] * m[5] - m[1] * m[4]], f32)
    det = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]
    assert det.dtype == f32 and c.dtype == f32
    return m, c, f32(-1.0) if det < 0 else f32(1.0), m.tobytes() == IDENTITY.tobytes()


def np_pose(rest, ids, matrices):
    """the restatement: every triangle of `rest` posed by its object's matrix"""
    out = rest.copy()
    ids = np.asarray(ids)
    with np.errstate(all="ignore"):
        for k, mat in enumerate(matrices):
            m, c, s, ident = np_object(mat)
            sel = ids == k
            if ident or not sel.any():
                continue
            for v in ("v1", "v2", "v3"):
                x, y, z = (rest[v]["position"][a][sel] for a in "xyz")
                for r, a in enumerate("xyz"):
                    out[v]["position"][a][sel] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]
                x, y, z = (rest[v]["normal"][a][sel] for a in "xyz")
                n = [((c[3 * r] * x + c[3 * r + 1] * y) + c[3 * r + 2] * z) * s for r in range(3)]
                l = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                ok = (l > 0) & np.isfinite(l)
                d = np.sqrt(l)
                for r, a in enumerate("xyz"):
                    assert n[r].dtype == f32 and d.dtype == f32
                    out[v]["normal"][a][sel] = np.where(ok, n[r] / d, n[r])
    return out


def decorated(tris, rng):
    """every lane a pose copies, filled: .w lanes, texture coordinates, material indices, padding"""
    t = tris.copy()
    raw = t.view(np.uint32).reshape(len(t), 40)
    junk = rng.integers(1, 2**31, raw.shape).astype(np.uint32)
    for v in range(3):
        raw[:, 12 * v + 3] = junk[:, 12 * v + 3]            # position.w
        raw[:, 12 * v + 4:12 * v + 8] = junk[:, 12 * v + 4:12 * v + 8]      # texcoord
        raw[:, 12 * v + 11] = junk[:, 12 * v + 11]          # normal.w
    raw[:, 36:40] = junk[:, 36:40]
    return t


def same_bytes(got, want):
    g, w = got.view(np.uint32).reshape(len(got), 40), want.view(np.uint32).reshape(len(want), 40)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


def random_case(rng, n, n_objects, matrices=None):
    tris = decorated(random_triangles(rng, n), rng)
    ids = rng.integers(0, n_objects, n).astype(np.uint32)
    if matrices is None:
        pool = list(MATRICES.values())
        matrices = np.stack([pool[k % len(pool)] if k < len(pool) else rotation(rng.normal(size=3), rng.uniform(0, 6), rng.normal(size=3)) for k in range(n_objects)])
    return tris, ids, matrices


def test_host_restatement_equals_numpy_bit_for_bit(golden_scenes):
    rng = np.random.default_rng(7)
    tris, ids, mats = random_case(rng, 3000, 9)
    zero = 5                                                  # a triangle with a zero normal, in every object in turn
    for k in range(9):
        ids[zero + k] = k
        for a in "xyz":
            tris["v2"]["normal"][a][zero + k] = 0.0
    assert set(ids.tolist()) == set(range(9))
    got = capi.debug_pose(None, tris, ids, mats)
    same_bytes(got, np_pose(tris, ids, mats))
    assert all((got["v2"]["normal"][a][zero:zero + 9] == 0).all() for a in "xyz")
    moved_rows = ids != 0                                     # object 0 is the identity
    assert (positions(got)[moved_rows] != positions(tris)[moved_rows]).any(-1).any(-1).all()
    # a mirror keeps unit normals and flips x only; det = 0 still gives normalised or untouched normals, never NaN
    for a in "xyz":
        assert np.isfinite(got["v1"]["normal"][a]).all()
    # the Cornell scene, one object per 5 triangles
    c = golden_scenes["cornell"]["triangles"]
    cid = (np.arange(len(c)) // 5 % 6).astype(np.uint32)
    cm = np.stack(list(MATRICES.values()))
    same_bytes(capi.debug_pose(None, c, cid, cm), np_pose(c, cid, cm))


def test_identity_returns_the_input_bytes(golden_scenes):
    rng = np.random.default_rng(8)
    tris, ids, _ = random_case(rng, 500, 4)
    same_bytes(capi.debug_pose(None, tris, ids, np.stack([IDENTITY] * 4)), tris)
    c = golden_scenes["cornell"]["triangles"]
    same_bytes(capi.debug_pose(None, c, np.zeros(len(c), np.uint32), IDENTITY[None]), c)
    # ... by the bits of the matrix: a matrix that only EQUALS the identity (a negative zero) is applied like any other
    m = IDENTITY.copy()
    m[0, 1] = -0.0
    same_bytes(capi.debug_pose(None, tris, ids, np.stack([m] * 4)), np_pose(tris, ids, [m] * 4))


def test_refusals():
    rng = np.random.default_rng(9)
    tris, ids, mats = random_case(rng, 20, 3)
    for bad in (np.nan, np.inf, -np.inf):
        m = mats.copy()
        m[1, 2, 3] = bad
        with pytest.raises(capi.RtError, match="not finite"):
            capi.debug_pose(None, tris, ids, m)
    wrong = ids.copy()
    wrong[7] = 3
    with pytest.raises(capi.RtError, match="not below num_objects"):
        capi.debug_pose(None, tris, wrong, mats)
    with pytest.raises(capi.RtError, match="no objects"):
        capi.debug_pose(None, tris, ids, mats, num_objects=0)
    lib = capi.load()
    out = np.zeros_like(tris)
    args = [tris.ctypes.data, ids.ctypes.data, len(tris), mats.ctypes.data, 3, out.ctypes.data]
    for k in (0, 1, 3, 5):
        a = list(args)
        a[k] = None
        assert lib.rt_debug_pose(None, *a) != 0
        assert b"NULL argument" in lib.rt_last_error(None)
    assert lib.rt_scene_set_objects(None, ids.ctypes.data, len(ids), 3) != 0 and b"NULL argument" in lib.rt_last_error(None)
    assert lib.rt_scene_pose(None, mats.ctypes.data, 3) != 0 and b"NULL argument" in lib.rt_last_error(None)


# ---- the host layer without a GPU: which triangles are which object

OBJ = os.path.join(ROOT, "assets", "CornellBox.obj")
NAMES = ["ceiling", "backWall", "rightWall", "leftWall", "tallBox", "light", "floor", "shortBox"]


def obj_faces_by_object(path):
    """{object name: [set of the face's vertex positions]} read from the OBJ's v / o / f lines (positive indices)"""
    v, out, name = [], {}, ""
    for line in open(path, errors="ignore"):
        w = line.split()
        if not w:
            continue
        if w[0] == "v":
            v.append(tuple(np.float32(x) for x in w[1:4]))
        elif w[0] in ("o", "g"):
            name = w[1]
        elif w[0] == "f":
            out.setdefault(name, []).append({v[int(x.split("/")[0]) - 1] for x in w[1:]})
    return out


def loaded(objects):
    from raytracing_amd import host
    s = host.Scene(OBJ, objects=objects)
    s.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    s.set_env_path(os.path.join(ROOT, "assets", "ibl", "CGSkies_0036_free.hdr"))
    before = s.arrays()["triangles"].copy()
    s.build_bvh()
    s.finalize()
    return s, before


def test_the_loader_numbers_the_objs_shapes_and_the_reorder_keeps_them():
    s, before = loaded(True)
    assert s.object_names() == NAMES
    tris, ids = s.arrays()["triangles"], s.triangle_objects()
    assert ids.shape == (len(tris),) and ids.dtype == np.uint32 and set(ids.tolist()) == set(range(8))
    assert tris.tobytes() != before.tobytes()                       # the BVH build did reorder them
    faces = obj_faces_by_object(OBJ)
    assert sorted(faces) == sorted(NAMES)
    P = positions(tris)
    for i in range(len(tris)):
        mine = {tuple(P[i, k]) for k in range(3)}
        assert any(mine <= f for f in faces[NAMES[ids[i]]]), (i, NAMES[ids[i]])
    counts = np.bincount(ids, minlength=8)
    assert [int(c) for c in counts] == [sum(len(f) - 2 for f in faces[n]) for n in NAMES]
    # off (the default): no objects, and the triangles' bytes are the same with and without the opt-in -- before the reorder up to the index that rides
    # in padding[0], after Finalize() entirely
    off, off_before = loaded(False)
    assert off.object_names() == [] and len(off.triangle_objects()) == 0
    assert off.arrays()["triangles"].tobytes() == tris.tobytes()
    raw_on, raw_off = before.view(np.uint32).reshape(-1, 40).copy(), off_before.view(np.uint32).reshape(-1, 40)
    assert (raw_off[:, 37] == 0).all() and set(raw_on[:, 37].tolist()) == set(range(8))
    raw_on[:, 37] = 0
    assert raw_on.tobytes() == raw_off.tobytes()
    assert (tris.view(np.uint32).reshape(-1, 40)[:, 36 + 1:] == 0).all()


def test_caller_built_arrays_take_an_objects_array(golden_scenes):
    from raytracing_amd import host
    sc = golden_scenes["cornell"]
    arrays = {k: sc[k] for k in ("triangles", "materials", "textures", "texture_data")}
    order = np.arange(len(sc["triangles"]), dtype=np.uint32)        # one object per triangle: the reorder itself comes back
    s = host.Scene(arrays=arrays, objects=order)
    s.set_env_image(np.zeros((2, 2, 4), np.float32))
    s.build_bvh()
    s.finalize()
    perm = s.triangle_objects()
    assert sorted(perm.tolist()) == order.tolist()
    assert s.arrays()["triangles"].tobytes() == sc["triangles"][perm].tobytes()
    with pytest.raises(host.RtError, match="one object index per triangle"):
        host.Scene(arrays=arrays, objects=order[:-1])
