"""The crossing query's layers without a GPU (rt_scene_cross / rt_scene_cross_self / rt_debug_cross*): the ctypes signatures and record
sizes, every refusal that needs no device, with its message, the flat C API's and host.py's forms, and what rt_render says of --cross and --self_cross
before it touches a device."""
import inspect
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def test_host_layer_signatures():
    lib = host.load()
    for name, n in (("rth_render_cross", 7), ("rth_render_self_cross", 7)):
        fn = getattr(lib, name)
        assert name in host.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == n and fn.restype is not None, name
    assert list(inspect.signature(host.Render.cross).parameters) == ["self", "probes", "k", "any"]
    assert inspect.signature(host.Render.cross).parameters["k"].default == 0 and inspect.signature(host.Render.cross).parameters["any"].default is False
    assert list(inspect.signature(host.Render.interpenetrations).parameters) == ["self"]
    assert list(inspect.signature(host.Render.self_cross).parameters) == ["self", "first", "n", "k", "other_objects"]


def test_rt_render_help_names_the_flags():
    r = subprocess.run([RT_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cross x1,y1,z1,x2,y2,z2,x3,y3,z3[,k]" in r.stdout + r.stderr and "--self_cross 1" in r.stdout + r.stderr


@pytest.mark.parametrize("value", ["0,0,0,1,1,1,2,2", "0,0,0,1,0,0,0,1,0,9", "nine"])
def test_rt_render_refuses_a_probe_it_cannot_read(value):
    r = subprocess.run([RT_RENDER, "--scene", "assets/CornellBox.obj", "--cross", value], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--cross wants" in r.stderr, (r.returncode, r.stderr[-300:])


def test_signatures_and_record_sizes():
    assert T.probe.itemsize == 48 and T.probe_hits.itemsize == 16 and T.cross_member.itemsize == 32
    assert capi.CROSS_LIST_MAX == 8 and capi.CROSS_ANY == 1 and capi.CROSS_OTHER_OBJECTS == 2
    lib = capi.load()
    want = {"rt_scene_cross": 7, "rt_scene_cross_buffer": 7, "rt_scene_cross_self": 7, "rt_scene_cross_self_buffer": 7, "rt_debug_cross": 9,
            "rt_debug_cross_walk": 12, "rt_debug_cross_self": 10}
    for name, n in want.items():
        fn = getattr(lib, name)
        assert name in capi.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == n, name
    for name in ("cross", "cross_buffer", "cross_self", "cross_self_buffer"):
        assert callable(getattr(capi.Context, name))
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    pr = T.probes_from_triangles(v, [[0, 1, 2], [1, 2, 3]])
    assert pr.dtype == T.probe and len(pr) == 2 and pr["p2"][1, :3].tolist() == [0, 1, 0] and not pr["p1"][:, 3].any()
    assert capi.probe_records(v[[[0, 1, 2]]]).tobytes() == pr[:1].tobytes()


def test_refusals_without_a_device(golden_scenes):
    lib = capi.load()
    sc = golden_scenes["cornell"]
    tris, nodes = np.ascontiguousarray(sc["triangles"]), np.ascontiguousarray(sc["nodes"])
    nt = len(tris)
    pr = T.probes_from_corners(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1]], np.float32), (4, 1, 1)))
    ids = np.zeros(nt, np.uint32)
    out, members = np.zeros(4, T.probe_hits), np.zeros((4, 8), T.cross_member)
    p = lambda a: a.ctypes.data

    def refused(rc, text):
        assert rc != 0 and text in lib.rt_last_error(None).decode(), (rc, lib.rt_last_error(None).decode())

    refused(lib.rt_scene_cross(None, p(pr), 4, 8, 0, p(out), p(members)), "rt_scene_cross: ctx is NULL")
    refused(lib.rt_scene_cross_buffer(None, None, 4, 8, 0, None, None), "rt_scene_cross_buffer: ctx is NULL")
    refused(lib.rt_scene_cross_self(None, 0, 4, 8, 0, p(out), p(members)), "rt_scene_cross_self: ctx is NULL")
    refused(lib.rt_scene_cross_self_buffer(None, 0, 4, 8, 0, None, None), "rt_scene_cross_self_buffer: ctx is NULL")
    for who, call, tail in (("rt_debug_cross", lambda *a: lib.rt_debug_cross(None, p(tris), nt, *a), ()),
                            ("rt_debug_cross_walk", lambda *a: lib.rt_debug_cross_walk(p(nodes), len(nodes), p(tris), nt, 1, *a), (None,))):
        refused(call(None, 4, 8, 0, p(out), p(members), *tail), who + ": NULL argument")
        refused(call(p(pr), 4, 8, 0, None, p(members), *tail), who + ": NULL argument")
        refused(call(p(pr), 4, 8, 0, p(out), None, *tail), who + ": NULL argument")
        refused(call(p(pr), 4, 9, 0, p(out), p(members), *tail), who + ": max_list is above RT_CROSS_LIST_MAX")
        refused(call(p(pr), 4, 8, 4, p(out), p(members), *tail), who + ": unknown option bits")
        refused(call(p(pr), 4, 8, capi.CROSS_OTHER_OBJECTS, p(out), p(members), *tail), who + ": RT_CROSS_OTHER_OBJECTS is the self forms'")
        refused(call(p(pr), 4, 8, capi.CROSS_ANY, p(out), p(members), *tail), who + ": RT_CROSS_ANY lists no members")
        refused(call(p(pr), 4, 0, 0, p(out), p(members), *tail), who + ": members given with max_list == 0")
        assert call(None, 0, 0, 0, None, None, *tail) == 0                                   # n == 0: RT_OK, nothing done
    refused(lib.rt_debug_cross_walk(None, len(nodes), p(tris), nt, 1, p(pr), 4, 8, 0, p(out), p(members), None), "rt_debug_cross_walk: NULL argument")
    refused(lib.rt_debug_cross_walk(p(nodes), len(nodes), p(tris), nt, 2, p(pr), 4, 8, 0, p(out), p(members), None), "rt_debug_cross_walk: wide must be")
    refused(lib.rt_debug_cross_walk(p(nodes), len(nodes), p(tris), nt - 1, 0, p(pr), 4, 8, 0, p(out), p(members), None), "outside the array")
    refused(lib.rt_debug_cross_self(None, None, nt, None, 0, 4, 8, 0, p(out), p(members)), "rt_debug_cross_self: NULL argument")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, 0, 4, 8, 0, None, p(members)), "rt_debug_cross_self: NULL argument")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, nt - 3, 4, 8, 0, p(out), p(members)), "rt_debug_cross_self: first + n is beyond the triangles")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, 0xFFFFFFFF, 4, 8, 0, p(out), p(members)), "first + n is beyond the triangles")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, 0, 4, 8, capi.CROSS_OTHER_OBJECTS, p(out), p(members)), "RT_CROSS_OTHER_OBJECTS needs object_of_triangle")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, 0, 4, 9, 0, p(out), p(members)), "rt_debug_cross_self: max_list is above RT_CROSS_LIST_MAX")
    refused(lib.rt_debug_cross_self(None, p(tris), nt, None, 0, 4, 8, 8, p(out), p(members)), "rt_debug_cross_self: unknown option bits")
    assert out.tobytes() == bytes(out.nbytes) and members.tobytes() == bytes(members.nbytes)      # nothing was written
    assert lib.rt_debug_cross(None, p(tris), nt, p(pr), 4, 0, 0, p(out), None) == 0               # max_list == 0: members may be NULL
    assert (out["flags"] == 1).all()
    assert lib.rt_debug_cross(None, p(tris), nt, p(pr), 4, 8, capi.CROSS_ANY, p(out), None) == 0  # any-mode lists nothing whatever max_list says
    assert (out["flags"] == 3).all() and not out["stored"].any()
    assert lib.rt_debug_cross_self(None, p(tris), nt, p(ids), 0, 4, 8, capi.CROSS_OTHER_OBJECTS, p(out), p(members)) == 0 and not out["count"].any()
