"""The spatial filter's edges without a GPU: a pixel whose demodulation overflows passes through as h_p, and rt_render refuses --filter where
the image is tiled over GPUs or the sigmas are malformed (before any device is touched)."""
import os
import subprocess

import numpy as np

from raytracing_amd import capi
from tests.test_spatial_filter import random_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def test_overflowing_demodulation_passes_through_as_h():
    rng = np.random.default_rng(3)
    hdr, alb, nrm, dep = random_inputs(rng, 12, 12, invalid=0.0)
    hdr[6, 6, :3] = 3.0e38                        # finite, but / 0.0011 overflows
    alb[6, 6, :3] = 0.0011
    for it in (1, 2, 5):
        out = capi.debug_filter(None, hdr, alb, nrm, dep, dict(iterations=it, flags=capi.FILTER_DEMODULATE, sigma_color=1.0, sigma_normal=0.2,
                                                               sigma_depth=0.2))
        assert np.array_equal(out[6, 6].view(np.uint32), hdr[6, 6].view(np.uint32)), it
        others = np.ones((12, 12), bool)
        others[6, 6] = False
        assert np.isfinite(out[others]).all()


def run_cli(*args):
    return subprocess.run([RT_RENDER] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=60)


def test_rt_render_refuses_filter_over_several_gpus():
    r = run_cli("--gpus", "2", "--filter", "2", "-w", "64", "-h", "64")
    assert r.returncode == 2 and "--filter" in r.stderr and "--gpus" in r.stderr


def test_rt_render_refuses_malformed_filter_sigmas():
    r = run_cli("--filter", "2", "--filter_sigmas", "1,2")
    assert r.returncode == 2 and "--filter_sigmas" in r.stderr


def test_rt_render_help_names_the_filter():
    r = run_cli("--help")
    assert r.returncode == 0 and "--filter n" in r.stdout
