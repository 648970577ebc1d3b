"""The C-ABI libraries load without a GPU and export every symbol the headers
declare; compute entry points fail loudly (no CPU fallback)."""
import ctypes
import os
import re
import pytest
from raytracing_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_librt_hip_exports_every_declared_symbol():
    lib = ctypes.CDLL(capi.LIB_PATH)
    names = _declared("rt_hip.h")
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(capi.EXPORTS) == names          # the Python binding covers the whole ABI


def test_the_crossing_counts_debug_entry_is_declared_bound_and_refuses_bad_input():
    """rt_debug_count_box_passes: ctx-or-NULL like rt_debug_refit; the host half runs without a GPU"""
    import numpy as np
    from raytracing_amd import types as T
    assert "rt_debug_count_box_passes" in _declared("rt_hip.h") and "rt_debug_count_box_passes" in capi.EXPORTS
    fn = capi.load().rt_debug_count_box_passes
    assert fn.argtypes is not None and len(fn.argtypes) == 8
    leaf = np.zeros(1, T.bvh_node)
    leaf["num_primitives_axis"] = 1 << 16
    for c in "xyz":
        leaf["bounds_min"][c], leaf["bounds_max"][c] = -1.0, 1.0
    o = np.array([[0, 0, -5, 1e30], [0, 0, -5, 1.0], [3, 0, -5, 1e30]], np.float32)
    d = np.array([[0, 0, 1, 0]] * 3, np.float32)
    counts, cut = capi.count_box_passes(None, leaf, o, d)
    assert counts.tolist() == [1] and cut == 0                      # one ray reaches the box; one ends before it, one passes beside it
    bad = np.zeros(3, T.bvh_node)                                   # an interior node whose second child lies outside the array
    bad["offset"][0] = 7
    with pytest.raises(capi.RtError, match="not a tree"):
        capi.count_box_passes(None, bad, o, d)


def test_librt_host_exports():
    lib = ctypes.CDLL(host.LIB_PATH)
    for n in host.EXPORTS:
        assert hasattr(lib, n), n


def test_no_gpu_means_loud_failure_not_fallback():
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.RtError, match="no HIP device"):
        capi.Context(0)
    s = host.Scene(os.path.join(ROOT, "assets", "CornellBox.obj"))
    with pytest.raises(host.RtError, match="HIP"):
        host.Render(32, 32, s)


def test_product_never_touches_the_oracle():
    """Nothing under raytracing_amd/ may import, link or call oracle/."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "raytracing_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".h", ".hip")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"liboracle|libref\.so|orc_[a-z_]+\(|from tests|import tests|#include\s+\"[^\"]*oracle", text) and f != "_build.py":
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad
