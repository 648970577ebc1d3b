"""The UV atlas's layers without a device: the host library exports its entries and refuses a NULL description, the binding's one rule
for a second UV set, the synthetic atlas's grid, and rt_render's flags (parsed before any device is touched)."""
import ctypes
import os
import subprocess
import numpy as np
import pytest
from raytracing_amd import capi, host, scenes as S, types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def test_host_library_exports_and_refuses_null_descriptions():
    assert {"rth_render_atlas", "rth_render_occlusion_atlas"} <= set(host.EXPORTS)
    lib = host.load()
    tx, st, out = np.zeros(4, T.texel), np.zeros(1, T.atlas_stats), np.zeros(4, np.float32)
    assert lib.rth_render_atlas(None, None, None, tx.ctypes.data, st.ctypes.data) != 0
    assert "rth_render_atlas: desc is NULL" in lib.rth_last_error().decode()
    d = capi.atlas_desc(2, 2)
    assert lib.rth_render_occlusion_atlas(None, ctypes.addressof(d), None, None, out.ctypes.data, st.ctypes.data) != 0
    assert "rth_render_occlusion_atlas: desc is NULL" in lib.rth_last_error().decode()


def test_the_bindings_rules():
    assert capi.atlas_uv(None, 5) is None
    assert capi.atlas_uv(np.zeros((5, 3, 2)), 5).shape == (30,) and capi.atlas_uv(np.zeros((5, 6)), 5).dtype == np.float32
    with pytest.raises(capi.RtError, match="six floats per triangle"):
        capi.atlas_uv(np.zeros(29), 5)
    d = capi.atlas_desc(7, 3, 2)
    assert (d.width, d.height, d.gutter, d.object) == (7, 3, 2, 0xFFFFFFFF) and capi.atlas_desc(1, 1, 0, 4).object == 4
    assert ctypes.sizeof(capi.rt_atlas_desc) == 16 and T.texel.itemsize == 16 and T.atlas_stats.itemsize == 32


@pytest.mark.parametrize("n,w,h", [(1, 8, 8), (2, 8, 8), (3, 8, 8), (32, 1, 1), (33, 64, 16), (1000, 16, 64)])
def test_synthetic_atlas_shares_its_corners_exactly(n, w, h):
    columns, rows = S.synthetic_atlas_grid(n, w, h)
    assert columns * rows >= (n + 1) // 2 > columns * (rows - 1)
    uv = S.synthetic_atlas(np.zeros(n, T.triangle), w, h).reshape(n, 3, 2)
    us, vs = np.unique(uv[:, :, 0]), np.unique(uv[:, :, 1])
    assert len(us) <= columns + 1 and len(vs) <= rows + 1 and uv.min() == 0 and uv.max() <= 1        # one value per grid line: neighbours share corners bit for bit
    for t in range(0, n - 1, 2):                                                                          # the two halves of a cell share its diagonal
        assert uv[t, 0].tolist() == uv[t + 1, 0].tolist() and uv[t, 2].tolist() == uv[t + 1, 1].tolist()
    tx, st = capi.debug_atlas(None, np.zeros(n, T.triangle), 2 * columns, 2 * rows, uv=uv)
    assert st["overlapped"] == 0 and st["triangles_skipped"] == 0
    if S.synthetic_atlas_grid(n, 2 * columns, 2 * rows) == (columns, rows):
        assert st["triangles_without_texel"] == 0


def test_rt_render_knows_the_atlas_flags():
    r = subprocess.run([RT_RENDER, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert "--ao_atlas out.pfm --atlas_size w,h [--atlas_gutter n]" in r.stdout + r.stderr
    r = subprocess.run([RT_RENDER, "--ao_atlas", "x.pfm", "--atlas_size", "64"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--atlas_size w,h" in r.stderr
