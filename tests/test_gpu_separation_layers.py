"""-m gpu: the layers above the C ABI of the separation queries give capi's answers through a 64 x 64 frame:
HIPPathTraceIntegrator::TrianglesSeparation / SelfSeparation through Render::Separation / Clearance and the flat C API, host.Render.separation() and
.clearances(), and rt_render --separation / --clearance; names appear when the scene was loaded with objects.  One process, each step once."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T
from tests.test_refit import positions
from tests.test_separation import make_probes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 64
INF = float("inf")


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


def test_render_separation_equals_capi_and_names_the_objects(cornell):
    scene, render, tris, probes = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    assert len(names) > 1 and len(owner) == len(tris)
    render.render_samples(1)                                                  # a frame exists and is left alone
    inf = capi.debug_separation(None, tris, probes)
    tight = float(np.median(inf["distance"][(inf["flags"] & 2 != 0) & (inf["distance"] > 0) & np.isfinite(inf["distance"])]))
    for r in (INF, tight, 0.0):
        want = capi.debug_separation(None, tris, probes, r)
        got = render.separation(probes, r)                                    # Render::Separation through rth_render_separation
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["searched"] == bool(w["flags"] & 1) and g["found"] == bool(w["flags"] & 2) and g["crossing"] == bool(w["flags"] & 4)
            assert g["primitive_id"] == w["primitive_id"] and g["feature"] == w["feature"] and np.float32(g["distance"]).tobytes() == w["distance"].tobytes()
            assert g["on_probe"].tobytes() == w["on_probe"].tobytes() and g["on_scene"].tobytes() == w["on_scene"].tobytes()
            assert g.get("object_name") == (names[owner[w["primitive_id"]]] if g["found"] else None)
    want = capi.debug_separation(None, tris, probes, tight)
    assert (want["flags"] == 1).any() and (want["flags"] & 4).any() and (want["flags"] == 0).any() and ((want["flags"] & 2 != 0) & (want["distance"] > 0)).any()


def test_clearances_of_two_posed_boxes(cornell):
    scene, render, tris, _ = cornell
    names, owner = scene.object_names(), np.asarray(scene.triangle_objects(), np.uint32)
    n = len(names)
    P = positions(tris).astype(np.float64)
    a, b = names.index("shortBox"), names.index("tallBox")
    keep = np.isin(owner, (a, b))
    render.set_objects(owner, n)
    lo_a, hi_a = P[owner == a].reshape(-1, 3).min(0), P[owner == a].reshape(-1, 3).max(0)
    lo_b, hi_b = P[owner == b].reshape(-1, 3).min(0), P[owner == b].reshape(-1, 3).max(0)
    # the two boxes alone, as two objects of a scene of their own, are what the pair's distance is measured on
    mats = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))

    def brute(posed):
        rec = capi.debug_separation_self(None, posed, 0, len(posed), INF, capi.SEPARATION_OTHER_OBJECTS, owner)
        return host.reduce_clearances(rec, owner, names), rec

    # a known gap: the tall box lifted off the floor by four gaps, the short box lifted clear above the tall box's top by one: nothing else is as near to either
    up = int(np.argmax(hi_b - lo_b))                                           # the tall box's long axis
    gap = float(np.float32((hi_b[up] - lo_b[up]) / 64))
    mats[b, up, 3] = 4 * gap
    mats[a, :, 3] = (lo_b + hi_b) / 2 - (lo_a + hi_a) / 2
    mats[a, up, 3] = hi_b[up] + 5 * gap - lo_a[up]
    render.pose(mats)
    posed = capi.debug_pose(None, tris, owner, mats)
    want, rec = brute(posed)

    def same_entries(got, want):
        assert list(got) == names
        for name in names:
            if want[name] is None:
                assert got[name] is None
                continue
            for key in ("other", "distance", "crossing", "triangle", "other_triangle"):
                assert got[name][key] == want[name][key], (name, key)
            assert got[name]["on_self"].tobytes() == want[name]["on_self"].tobytes() and got[name]["on_other"].tobytes() == want[name]["on_other"].tobytes()

    got = render.clearances()
    same_entries(got, want)
    both = np.flatnonzero(keep)
    pair = capi.debug_separation_self(None, posed[both], 0, len(both), INF, capi.SEPARATION_OTHER_OBJECTS, owner[both])
    assert got["shortBox"]["other"] == "tallBox" and got["tallBox"]["other"] == "shortBox" and not got["shortBox"]["crossing"]
    assert got["shortBox"]["distance"] == got["tallBox"]["distance"] == float(pair["distance"].min())
    assert abs(got["shortBox"]["distance"] - gap) <= 1e-5 * float(np.abs(P).max())       # the two faces are level: the gap, to the pose's rounding
    # pushed into each other: distance 0 and the crossing flag
    mats[a, :, 3] = (lo_b + hi_b) / 2 - (lo_a + hi_a) / 2 + np.array([0.03, 0.02, 0.01]) * np.linalg.norm(hi_b - lo_b)
    mats[a, up, 3] += 4 * gap
    render.pose(mats)
    got = render.clearances()
    same_entries(got, brute(capi.debug_pose(None, tris, owner, mats))[0])
    for name, other in (("shortBox", "tallBox"), ("tallBox", "shortBox")):
        assert got[name]["distance"] == 0.0 and got[name]["crossing"] and got[name]["other"] == other
    render.pose(np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1)))           # back to rest


def test_rt_render_prints_the_same(cornell):
    scene, render, tris, probes = cornell
    names, owner = scene.object_names(), np.asarray(scene.triangle_objects(), np.uint32)
    want = capi.debug_separation(None, tris, probes)
    apart = (want["flags"] & 2 != 0) & (want["distance"] > 0) & np.isfinite(want["distance"])
    i, j = int(np.flatnonzero(apart)[0]), int(np.flatnonzero(want["flags"] & 4)[0])
    arg = lambda q: ",".join("%.9g" % x for x in list(q["p1"][:3]) + list(q["p2"][:3]) + list(q["p3"][:3]))
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", str(W), "-h", str(H), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--separation", arg(probes[i]), "--separation", arg(probes[j]), "--separation", arg(probes[i]) + ",%.9g" % (want["distance"][i] / 2),
                        "--clearance", "1"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("separation ")]
    assert r.returncode == 0 and len(lines) == 3, (r.returncode, r.stdout[-800:], r.stderr[-400:])
    for ln, k in ((lines[0], i), (lines[1], j)):
        w = want[k]
        assert (" primitive %d feature %d " % (w["primitive_id"], w["feature"])) in ln and ln.rstrip().endswith(names[owner[w["primitive_id"]]]), ln
        assert abs(float(ln.split("distance ")[1].split()[0]) - w["distance"]) <= 1e-5 * max(float(w["distance"]), 1e-30)      # (printed with six digits)
    assert " crossing " not in lines[0] and "distance 0 crossing " in lines[1] and lines[2].rstrip().endswith(": none")
    # the per-object table equals the reduction of the host's brute force at rest
    rec = capi.debug_separation_self(None, tris, 0, len(tris), INF, capi.SEPARATION_OTHER_OBJECTS, owner)
    table = host.reduce_clearances(rec, owner, names)
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("clearance: ")]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("clearance   ")]
    assert len(head) == 1 and ("objects %d triangles %d" % (len(names), len(tris))) in head[0] and len(rows) == len(names)
    for name, ln in zip(names, rows):
        e = table[name]
        assert ln.startswith("clearance   %d %s | " % (names.index(name), name)), ln             # (rt_render prints an object as its index and its name)
        if e is None:
            assert ln.rstrip().endswith("| none")
        else:
            assert ("| %d %s distance " % (names.index(e["other"]), e["other"])) in ln and (" triangles %d %d from " % (e["triangle"], e["other_triangle"])) in ln and (" crossing " in ln) == e["crossing"], (ln, e)
