"""The layers of the separation queries without a GPU: the bindings' signatures, every refusal the entry points make before a device is
needed, and host.reduce_clearances -- the reduction of the self form's records to one entry per object -- on a hand-made table."""
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T

INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def test_rt_render_help_names_the_flags():
    r = subprocess.run([RT_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--separation x1,y1,z1,x2,y2,z2,x3,y3,z3[,r]" in r.stdout + r.stderr and "--clearance 1" in r.stdout + r.stderr


@pytest.mark.parametrize("value", ["0,0,0,1,1,1,2,2", "0,0,0,1,0,0,0,1,0,-1", "0,0,0,1,0,0,0,1,0,nan", "nine"])
def test_rt_render_refuses_a_probe_it_cannot_read(value):
    r = subprocess.run([RT_RENDER, "--scene", "assets/CornellBox.obj", "--separation", value], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--separation wants" in r.stderr, (r.returncode, r.stderr[-300:])


def test_signatures_and_record_sizes():
    assert T.separation.itemsize == 48 and T.separation.fields["on_scene"][1] == 16 and T.separation.fields["flags"][1] == 32
    assert (capi.SEPARATION_OTHER_OBJECTS, capi.SEPARATION_SEARCHED, capi.SEPARATION_FOUND, capi.SEPARATION_CROSSING, capi.SEPARATION_FEATURE_CROSSING) == (2, 1, 2, 4, 15)
    lib = capi.load()
    want = {"rt_scene_separation": 6, "rt_scene_separation_buffer": 6, "rt_scene_separation_self": 6, "rt_scene_separation_self_buffer": 6, "rt_debug_separation": 7,
            "rt_debug_separation_walk": 10, "rt_debug_separation_self": 9}
    for name, n in want.items():
        fn = getattr(lib, name)
        assert name in capi.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == n, name
    for name in ("separation", "separation_buffer", "separation_self", "separation_self_buffer"):
        assert callable(getattr(capi.Context, name))
    hl = host.load()
    for name, n in (("rth_render_separation", 5), ("rth_render_clearance", 5)):
        assert name in host.EXPORTS and len(getattr(hl, name).argtypes) == n
    assert callable(host.Render.separation) and callable(host.Render.clearances)


def test_refusals_without_a_device(golden_scenes):
    lib = capi.load()
    sc = golden_scenes["cornell"]
    tris, nodes = np.ascontiguousarray(sc["triangles"]), np.ascontiguousarray(sc["nodes"])
    nt = len(tris)
    pr = T.probes_from_corners(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1]], np.float32), (4, 1, 1)))
    ids = np.zeros(nt, np.uint32)
    out = np.zeros(4, T.separation)
    p = lambda a: a.ctypes.data

    def refused(rc, text):
        assert rc != 0 and text in lib.rt_last_error(None).decode(), (rc, lib.rt_last_error(None).decode())

    refused(lib.rt_scene_separation(None, p(pr), 4, INF, 0, p(out)), "rt_scene_separation: ctx is NULL")
    refused(lib.rt_scene_separation_buffer(None, None, 4, INF, 0, None), "rt_scene_separation_buffer: ctx is NULL")
    refused(lib.rt_scene_separation_self(None, 0, 4, INF, 0, p(out)), "rt_scene_separation_self: ctx is NULL")
    refused(lib.rt_scene_separation_self_buffer(None, 0, 4, INF, 0, None), "rt_scene_separation_self_buffer: ctx is NULL")
    refused(lib.rt_debug_separation(None, p(tris), nt, None, 4, INF, p(out)), "rt_debug_separation: NULL argument")
    refused(lib.rt_debug_separation(None, p(tris), nt, p(pr), 4, INF, None), "rt_debug_separation: NULL argument")
    refused(lib.rt_debug_separation(None, None, nt, p(pr), 4, INF, p(out)), "rt_debug_separation: NULL argument")
    assert lib.rt_debug_separation(None, None, 0, None, 0, INF, None) == 0                         # n == 0: RT_OK, nothing done
    walk = lambda *a: lib.rt_debug_separation_walk(*a)
    refused(walk(None, len(nodes), p(tris), nt, 1, p(pr), 4, INF, p(out), None), "rt_debug_separation_walk: NULL argument")
    refused(walk(p(nodes), len(nodes), p(tris), nt, 1, None, 4, INF, p(out), None), "rt_debug_separation_walk: NULL argument")
    refused(walk(p(nodes), len(nodes), p(tris), nt, 1, p(pr), 4, INF, None, None), "rt_debug_separation_walk: NULL argument")
    refused(walk(p(nodes), len(nodes), p(tris), nt, 2, p(pr), 4, INF, p(out), None), "rt_debug_separation_walk: wide must be")
    refused(walk(p(nodes), len(nodes), p(tris), nt - 1, 0, p(pr), 4, INF, p(out), None), "outside the array")
    assert walk(None, 0, None, 0, 1, None, 0, INF, None, None) == 0
    self_ = lambda *a: lib.rt_debug_separation_self(None, *a)
    refused(self_(None, nt, None, 0, 4, INF, 0, p(out)), "rt_debug_separation_self: NULL argument")
    refused(self_(p(tris), nt, None, 0, 4, INF, 0, None), "rt_debug_separation_self: NULL argument")
    refused(self_(p(tris), nt, None, nt - 3, 4, INF, 0, p(out)), "rt_debug_separation_self: first + n is beyond the triangles")
    refused(self_(p(tris), nt, None, 0xFFFFFFFF, 4, INF, 0, p(out)), "first + n is beyond the triangles")
    refused(self_(p(tris), nt, None, 0, 4, INF, capi.SEPARATION_OTHER_OBJECTS, p(out)), "RT_SEPARATION_OTHER_OBJECTS needs object_of_triangle")
    refused(self_(p(tris), nt, None, 0, 4, INF, 1, p(out)), "rt_debug_separation_self: unknown option bits")
    refused(self_(p(tris), nt, None, 0, 4, INF, 8, p(out)), "rt_debug_separation_self: unknown option bits")
    assert out.tobytes() == bytes(out.nbytes)                                                      # nothing was written
    assert self_(p(tris), nt, p(ids), 0, 4, INF, capi.SEPARATION_OTHER_OBJECTS, p(out)) == 0       # one object: searched, nothing to find
    assert (out["flags"] == capi.SEPARATION_SEARCHED).all() and (out["primitive_id"] == 0xFFFFFFFF).all()
    assert lib.rt_debug_separation(None, p(tris), nt, p(pr), 4, INF, p(out)) == 0 and (out["flags"] & capi.SEPARATION_FOUND).all()


def test_clearances_reduction_on_a_hand_made_table():
    F = capi.SEPARATION_SEARCHED | capi.SEPARATION_FOUND
    names = ["floor", "a", "b", "far", "empty"]
    objects = np.array([0, 0, 1, 1, 2, 2, 3], np.uint32)                # "empty" owns no triangle
    rec = np.zeros(7, T.separation)
    rec["primitive_id"] = 0xFFFFFFFF
    rec["flags"] = capi.SEPARATION_SEARCHED

    def put(i, t, d, flags=F):
        rec[i] = ((i, 0, 0), d, (t, 1, 0), t, flags, 3, (0, 0))

    put(0, 2, 0.5)            # floor: triangle 0 -> a at 0.5, triangle 1 -> b at 0.5: a tie in distance, the lowest (triangle, other triangle) wins
    put(1, 4, 0.5)
    put(2, 5, 0.25)           # a: triangle 2 -> b at 0.25, triangle 3 -> b at 0.2500001: the smaller
    put(3, 4, np.float32(0.25) + np.float32(2.0 ** -24))
    put(4, 3, 0.125)          # b: triangle 4 -> a at 0.125 (the other direction of the pair a - b, smaller: both report it), triangle 5 crosses nothing nearer
    put(5, 2, 0.25)
    # far (triangle 6): nothing within max_distance
    got = host.reduce_clearances(rec, objects, names)
    assert list(got) == names and got["far"] is None and got["empty"] is None
    assert got["floor"]["other"] == "a" and got["floor"]["distance"] == 0.5 and (got["floor"]["triangle"], got["floor"]["other_triangle"]) == (0, 2)
    assert got["b"]["other"] == "a" and got["b"]["distance"] == 0.125 and (got["b"]["triangle"], got["b"]["other_triangle"]) == (4, 3)
    # a's own best was 0.25 by triangle 2; b's direction of the same pair of objects is smaller, so a reports that one, seen from its side
    assert got["a"]["other"] == "b" and got["a"]["distance"] == 0.125 and (got["a"]["triangle"], got["a"]["other_triangle"]) == (3, 4)
    assert got["a"]["on_self"].tolist() == [3.0, 1.0, 0.0] and got["a"]["on_other"].tolist() == [4.0, 0.0, 0.0] and not got["a"]["crossing"]
    # a crossing: distance 0 and the flag
    put(6, 0, 0.0, F | capi.SEPARATION_CROSSING)
    got = host.reduce_clearances(rec, objects, names)
    assert got["far"]["other"] == "floor" and got["far"]["distance"] == 0.0 and got["far"]["crossing"]
    assert got["floor"]["other"] == "a"                                    # floor's own records do not name far: only far's direction is present


def test_clearances_reduction_consults_every_direction_of_a_pair():
    """b's nearest is a third object, yet another of b's triangles names a at a last-bit smaller distance than a's own record of b: a reports that one"""
    F = capi.SEPARATION_SEARCHED | capi.SEPARATION_FOUND
    names = ["a", "b", "c"]
    objects = np.array([0, 1, 1, 2], np.uint32)
    rec = np.zeros(4, T.separation)
    near = np.float32(0.25)
    rec[0] = ((0, 0, 0), near, (1, 0, 0), 1, F, 6, (0, 0))                           # a: triangle 0 -> b's triangle 1
    rec[1] = ((1, 0, 0), np.nextafter(near, np.float32(0)), (0, 0, 0), 0, F, 6, (0, 0))   # b: triangle 1 -> a, a last bit smaller
    rec[2] = ((2, 0, 0), 0.125, (3, 0, 0), 3, F, 0, (0, 0))                          # b: triangle 2 -> c, nearer: b's entry
    rec[3] = ((3, 0, 0), 0.125, (2, 0, 0), 2, F, 3, (0, 0))
    got = host.reduce_clearances(rec, objects, names)
    assert got["b"]["other"] == "c" and got["b"]["distance"] == 0.125
    assert got["a"]["other"] == "b" and np.float32(got["a"]["distance"]) == np.nextafter(near, np.float32(0)) and (got["a"]["triangle"], got["a"]["other_triangle"]) == (0, 1)
    assert got["a"]["on_self"].tolist() == [0.0, 0.0, 0.0] and got["a"]["on_other"].tolist() == [1.0, 0.0, 0.0]
