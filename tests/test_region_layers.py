"""The layers above the C ABI of the overlap queries as far as they go without a GPU: the flat C API exports Render::Overlap / Select /
PickRect, and rt_render knows --overlap and --pick_rect and refuses what they cannot read before it touches a device."""
import os
import subprocess
import pytest
from raytracing_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def test_flat_c_api_exports_the_render_entries():
    lib = host.load()
    for name in ("rth_render_overlap", "rth_render_select", "rth_render_pick_rect", "rth_render_integrator_pick_rect"):
        assert name in host.EXPORTS and getattr(lib, name).argtypes is not None
    for method in ("overlap", "select", "pick_rect"):
        assert callable(getattr(host.Render, method))


def test_rt_render_help_names_the_flags():
    r = subprocess.run([RT_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--overlap lx,ly,lz,hx,hy,hz[,k]" in r.stdout + r.stderr and "--pick_rect x0,y0,x1,y1[,window]" in r.stdout + r.stderr


@pytest.mark.parametrize("flag, value, text", [("--overlap", "0,0,0,1,1", "--overlap wants"), ("--overlap", "0,0,0,1,1,1,9", "--overlap wants"),
                                               ("--pick_rect", "1,2,3", "--pick_rect wants"), ("--pick_rect", "1,2,3,4,door", "--pick_rect wants")])
def test_rt_render_refuses_what_it_cannot_read(flag, value, text):
    r = subprocess.run([RT_RENDER, "--scene", "assets/CornellBox.obj", flag, value], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr[-300:])
