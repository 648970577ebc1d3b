"""-m gpu: the layers above the C ABI of the crossing queries give capi's answers through a 64 x 64 frame:
HIPPathTraceIntegrator::TrianglesCross / SelfCross through Render::Cross / SelfCross and the flat C API, host.Render.cross() / .self_cross() /
.interpenetrations(), and rt_render --cross / --self_cross; names appear when the scene was loaded with objects.  One process per step, each step once."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T
from tests.test_refit import positions
from tests.test_cross import make_probes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 64


@pytest.fixture(scope="module")
def cornell():
    """the Cornell box loaded with objects behind a refittable Render, its arrays and a batch of probes"""
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"), objects=True)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    render = host.Render(W, H, scene)
    render.set_camera(host.default_camera(W, H)); render.set_max_bounces(4)
    render.set_refittable(True)
    tris = render.scene_arrays()["triangles"]
    return scene, render, tris, make_probes(tris, 40, 77)


def test_render_cross_equals_capi_and_names_the_objects(cornell):
    scene, render, tris, probes = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    assert len(names) > 1 and len(owner) == len(tris)
    render.render_samples(1)                                                  # a frame exists and is left alone
    for k in (8, 3, 0):
        want = capi.debug_cross(None, tris, probes, k) if k else (capi.debug_cross(None, tris, probes, 0), None)
        got = render.cross(probes, k=k)                                       # Render::Cross through rth_render_cross
        assert [g["count"] for g in got] == list(want[0]["count"]) and [g["first_primitive"] for g in got] == list(want[0]["first_primitive"])
        assert [g["searched"] for g in got] == [bool(f & 1) for f in want[0]["flags"]]
        for i, g in enumerate(got):
            assert len(g["members"]) == (want[0]["stored"][i] if k else 0)
            for m, w in zip(g["members"], want[1][i] if k else ()):
                assert m["primitive_id"] == w["primitive_id"] and m["flags"] == w["flags"] and m["object_name"] == names[owner[w["primitive_id"]]]
                assert m["c0"].tobytes() == w["c0"].tobytes() and m["c1"].tobytes() == w["c1"].tobytes()
    want = capi.debug_cross(None, tris, probes, 8)[0]
    assert (want["count"] > 0).sum() >= 5 and (want["count"] == 0).any() and (want["flags"] == 0).any()
    got = render.cross(probes, any=True)
    assert [g["count"] for g in got] == list(np.minimum(want["count"], 1)) and not any(g["members"] for g in got)
    with pytest.raises(host.RtError, match="RT_CROSS_LIST_MAX"):
        render.cross(probes, k=9)
    # the self form equals the host's brute force; nothing cuts itself in the Cornell box at rest beyond what the brute force says
    rec, mem = capi.debug_cross_self(None, tris, 0, len(tris), 8)
    got = render.self_cross()
    assert [g["count"] for g in got] == list(rec["count"]) and [[m["primitive_id"] for m in g["members"]] for g in got] == [list(r[:s]) for r, s in zip(mem["primitive_id"], rec["stored"])]


def test_interpenetrations_of_two_posed_boxes(cornell):
    scene, render, tris, _ = cornell
    names, owner = scene.object_names(), np.asarray(scene.triangle_objects(), np.uint32)
    n = len(names)
    P = positions(tris).astype(np.float64)
    a, b = names.index("shortBox"), names.index("tallBox")
    ca, cb = P[owner == a].reshape(-1, 3).mean(0), P[owner == b].reshape(-1, 3).mean(0)
    render.set_objects(owner, n)
    mats = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))
    rest = render.interpenetrations()
    assert tuple(sorted((names[a], names[b]))) not in rest["pairs"]           # apart at rest
    mats[a, :, 3] = (cb - ca) + np.array([0.03, 0.02, 0.01]) * np.linalg.norm(cb - ca)       # pushed into each other: the centres nearly coincide
    render.pose(mats)
    posed = capi.debug_pose(None, tris, owner, mats)
    rec, mem = capi.debug_cross_self(None, posed, 0, len(posed), 8, capi.CROSS_OTHER_OBJECTS, owner)
    want = {tuple(sorted((names[owner[i]], names[owner[t]]))) for i in range(len(posed)) for t in mem["primitive_id"][i][:rec["stored"][i]]}
    got = render.interpenetrations()
    assert got["pairs"] == want and tuple(sorted((names[a], names[b]))) in got["pairs"]
    assert got["complete"] == bool((rec["count"] <= 8).all())
    assert all(x != y for x, y in got["pairs"])                               # pairs of one object are skipped
    render.pose(np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1)))           # back to rest for the tests after this one
    assert render.interpenetrations()["pairs"] == rest["pairs"]


def test_rt_render_prints_the_same(cornell):
    scene, render, tris, probes = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    want = capi.debug_cross(None, tris, probes, 8)
    i = int(np.argmax(np.where(want[0]["count"] <= 8, want[0]["count"], 0)))
    q = probes[i]
    arg = ",".join("%.9g" % x for x in list(q["p1"][:3]) + list(q["p2"][:3]) + list(q["p3"][:3]))
    lo = positions(tris).reshape(-1, 3).max(0) + 5
    far = ",".join("%.9g" % x for x in list(lo) + list(lo + [1, 0, 0]) + list(lo + [0, 1, 0]))
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", str(W), "-h", str(H), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--cross", arg, "--cross", arg + ",1", "--cross", far, "--self_cross", "1"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("cross ")]
    stored = int(want[0]["stored"][i])
    assert stored >= 1 and r.returncode == 0 and len(lines) == 1 + stored + 1 + 1 + 1, (r.returncode, r.stdout[-800:], r.stderr[-400:])
    assert ("count %d listed %d" % (want[0]["count"][i], stored)) in lines[0]
    for m in range(stored):
        w = want[1][i, m]
        assert ("primitive %d tests %d " % (w["primitive_id"], w["flags"])) in lines[1 + m] and lines[1 + m].rstrip().endswith(names[owner[w["primitive_id"]]]), lines[1 + m]
    assert "listed 1" in lines[1 + stored] and lines[-1].rstrip().endswith(": none")
    rec = capi.debug_cross_self(None, tris, 0, len(tris), 8)[0]
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("self_cross: ")]
    assert len(head) == 1 and ("triangles %d crossing %d listed %d above the list %d" % (len(tris), (rec["count"] != 0).sum(), rec["stored"].sum(), (rec["count"] > 8).sum())) in head[0]
