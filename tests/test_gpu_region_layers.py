"""-m gpu: the layers above the C ABI of the overlap queries give capi's answers: HIPPathTraceIntegrator::RegionsOverlap /
SelectRegions / PickRect(Through) through Render::Overlap / Select / PickRect and the flat C API, host.Render.overlap() / .select() / .pick_rect(), and
rt_render --overlap / --pick_rect; names appear when the scene was loaded with objects.  One process per step, each step once."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T
from tests.test_refit import positions

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 32, 24


@pytest.fixture(scope="module")
def cornell():
    """the Cornell box loaded with objects behind a Render, its arrays, and regions of several kinds with their host brute-force answers"""
    scene = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"), objects=True)
    scene.add_directional_light((-0.6, -1.5, 3.5), (15.0, 10.0, 5.0))
    render = host.Render(W, H, scene)
    render.set_camera(host.default_camera(W, H)); render.set_max_bounces(4)
    tris = render.scene_arrays()["triangles"]
    flat = positions(tris).reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    rng = np.random.default_rng(23)
    regions = []
    for i in range(12):
        c, h = lo + rng.uniform(0.2, 0.8, 3) * (hi - lo), rng.uniform(0.1, 0.45, 3) * (hi - lo)
        regions.append(T.box_region(c - h, c + h))
    regions.append(T.box_region(lo - 1, hi + 1))                              # everything
    regions.append(T.box_region(hi + 5, hi + 6))                              # nothing
    bad = T.box_region(lo, hi); bad["num_planes"] = 0
    regions.append(bad)                                                       # not searched
    regions = np.array(regions, T.region)
    return scene, render, tris, regions, (lo, hi)


def test_render_overlap_and_select_equal_capi_and_name_the_objects(cornell):
    scene, render, tris, regions, _ = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    assert len(names) > 1 and len(owner) == len(tris)
    for k in (8, 3, 0):
        want = capi.debug_overlap(None, tris, regions, k)
        got = render.overlap(regions, k=k)                                    # Render::Overlap through rth_render_overlap
        assert [g["count"] for g in got] == list(want[0]["count"]) and [g["inside"] for g in got] == list(want[0]["inside"])
        assert [g["searched"] for g in got] == [bool(f) for f in want[0]["flags"]]
        for g, o, row in zip(got, want[0], want[1]):
            assert len(g["members"]) == o["stored"]
            for m, w in zip(g["members"], row):
                assert m["primitive_id"] == w["primitive_id"] and m["inside"] == bool(w["flags"] & 1) and m["object_name"] == names[owner[w["primitive_id"]]]
                assert m["crossing_planes"] == [p for p in range(8) if (int(w["flags"]) >> (8 + p)) & 1]
    want = capi.debug_overlap(None, tris, regions, 8)
    assert (want[0]["count"] > 8).any() and (want[0]["count"] == 0).any() and ((0 < want[0]["inside"]) & (want[0]["inside"] < want[0]["count"])).any()
    touching, inside, ot, oi = capi.debug_select(None, tris, regions, owner, len(names))
    got = render.select(regions)                                              # Render::Select through rth_render_select
    crossing_differs = False
    for r, g in enumerate(got):
        assert np.array_equal(g["touching"], np.flatnonzero((touching >> r) & 1)) and np.array_equal(g["inside"], np.flatnonzero((inside >> r) & 1))
        assert g["objects_touching"] == sorted({names[o] for o in range(len(names)) if (ot[o] >> r) & 1})
        assert g["objects_inside"] == sorted({names[o] for o in range(len(names)) if (oi[o] >> r) & 1})
        crossing_differs |= g["objects_touching"] != g["objects_inside"]
    assert crossing_differs and got[12]["objects_inside"] == sorted(set(names[o] for o in np.unique(owner))) and got[13]["objects_touching"] == []
    with pytest.raises(host.RtError, match="RT_SELECT_MAX_REGIONS"):
        render.select(np.tile(regions, 3)[:33])
    with pytest.raises(host.RtError, match="RT_REGION_LIST_MAX"):
        render.overlap(regions, k=9)
    c = capi.Context(0)
    try:
        c.upload_scene(render.scene_arrays())
        assert c.overlap(regions, 8)[0].tobytes() == want[0].tobytes() and c.overlap(regions, 8)[1].tobytes() == want[1].tobytes()
        assert c.select(regions)[0].tobytes() == touching.tobytes()
    finally:
        c.close()


def test_pick_rect_equals_capi_and_holds_what_the_pixels_pick(cornell):
    scene, render, tris, regions, _ = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    for rect in ((8, 6, 23, 17), (0, 0, W - 1, H - 1), (3, 4, 3, 4)):
        got = render.pick_rect(*rect)                                         # Render::PickRect -> HIPPathTraceIntegrator::PickRectThrough
        win = render.pick_rect(*rect, window=True)
        g = got["region"]
        assert g["num_planes"] == 4 and win["region"].tobytes() == g.tobytes()
        touching, inside, ot, oi = capi.debug_select(None, tris, [g], owner, len(names))
        assert np.array_equal(got["primitives"], np.flatnonzero(touching & 1)) and np.array_equal(win["primitives"], np.flatnonzero(inside & 1))
        assert got["objects"] == sorted({names[o] for o in range(len(names)) if ot[o] & 1}) and win["objects"] == sorted({names[o] for o in range(len(names)) if oi[o] & 1})
        picked = {render.pick(x, y)["primitive_id"] for y in range(rect[1], rect[3] + 1, 3) for x in range(rect[0], rect[2] + 1, 3)} - {0xFFFFFFFF}
        assert picked and picked <= set(got["primitives"].tolist()), rect
        assert set(win["primitives"].tolist()) <= set(got["primitives"].tolist())
    full = render.pick_rect(0, 0, W - 1, H - 1)
    assert len(full["objects"]) > 1 and len(full["primitives"]) > len(render.pick_rect(3, 4, 3, 4)["primitives"])
    with pytest.raises(host.RtError, match="outside the image"):
        render.pick_rect(0, 0, W, H - 1)
    with pytest.raises(host.RtError, match="x1 < x0"):
        render.pick_rect(5, 0, 4, 3)
    # the Integrator's own PickRect reads the FRAME's camera: after a frame it is the Render's, and the answers agree
    render.render_samples(1)
    nt = len(tris)
    g, t2, i2 = np.zeros(1, T.region), np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
    assert render.lib.rth_render_integrator_pick_rect(render.handle, 8, 6, 23, 17, 0.0, float("inf"), g.ctypes.data, t2.ctypes.data, i2.ctypes.data) == 0
    got = render.pick_rect(8, 6, 23, 17)
    assert g[0].tobytes() == got["region"].tobytes() and np.array_equal(np.flatnonzero(t2 & 1), got["primitives"])


def test_rt_render_prints_the_same(cornell):
    scene, render, tris, regions, (lo, hi) = cornell
    names, owner = scene.object_names(), scene.triangle_objects()
    want = capi.debug_overlap(None, tris, regions, 8)
    i = int(np.argmax(want[0]["count"][:12]))
    box = regions[i]["planes"]
    blo, bhi = (box[0, 3], box[1, 3], box[2, 3]), (-box[3, 3], -box[4, 3], -box[5, 3])
    arg = "%.9g,%.9g,%.9g,%.9g,%.9g,%.9g" % (blo + bhi)
    far = "%.9g,%.9g,%.9g,%.9g,%.9g,%.9g" % (tuple(hi + 5) + tuple(hi + 6))
    r = subprocess.run([os.path.join(ROOT, "raytracing_amd", "rt_render"), "-w", str(W), "-h", str(H), "--spp", "1", "--scene", "assets/CornellBox.obj",
                        "--overlap", arg, "--overlap", arg + ",2", "--overlap", far, "--pick_rect", "8,6,23,17", "--pick_rect", "0,0,%d,%d,window" % (W - 1, H - 1)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("overlap ")]
    stored = int(want[0]["stored"][i])
    assert r.returncode == 0 and len(lines) == 1 + stored + 1 + 2 + 1, (r.returncode, r.stdout[-800:], r.stderr[-400:])
    assert ("count %d inside %d listed %d" % (want[0]["count"][i], want[0]["inside"][i], stored)) in lines[0]
    for m in range(stored):
        w = want[1][i, m]
        assert ("primitive %d " % w["primitive_id"]) in lines[1 + m] and (" inside " if w["flags"] & 1 else " crossing ") in lines[1 + m]
        assert lines[1 + m].rstrip().endswith(names[owner[w["primitive_id"]]]), lines[1 + m]
    assert "listed 2" in lines[1 + stored] and ("primitive %d " % want[1][i, 1]["primitive_id"]) in lines[3 + stored]
    assert lines[-1].rstrip().endswith(": none")
    rects = [ln for ln in r.stdout.splitlines() if ln.startswith("pick_rect ")]
    got, win = render.pick_rect(8, 6, 23, 17), render.pick_rect(0, 0, W - 1, H - 1, window=True)
    heads = [k for k, ln in enumerate(rects) if ": primitives " in ln]
    assert len(heads) == 2 and rects[heads[0]].rstrip().endswith("primitives %d" % len(got["primitives"])) and "window" in rects[heads[1]]
    assert rects[heads[1]].rstrip().endswith("primitives %d" % len(win["primitives"]))
    assert sorted(ln.split("object ", 1)[1].split(" ", 1)[1].rstrip() for ln in rects[heads[0] + 1:heads[1]]) == got["objects"]
    assert sorted(ln.split("object ", 1)[1].split(" ", 1)[1].rstrip() for ln in rects[heads[1] + 1:]) == win["objects"]
