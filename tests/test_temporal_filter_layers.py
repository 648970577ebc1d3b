"""The temporal filter's command line without a GPU: rt_render refuses --temporal_filter where the image is tiled over GPUs or beside
--filter, malformed --temporal_alphas / --temporal_sigmas / --camera_step, and --camera_step without --frames (before any device is touched)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_RENDER = os.path.join(ROOT, "raytracing_amd", "rt_render")


def run_cli(*args):
    return subprocess.run([RT_RENDER] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=60)


def test_rt_render_refuses_temporal_filter_over_several_gpus():
    r = run_cli("--gpus", "2", "--temporal_filter", "2", "-w", "64", "-h", "64")
    assert r.returncode == 2 and "--temporal_filter" in r.stderr and "--gpus" in r.stderr


def test_rt_render_refuses_both_filters():
    r = run_cli("--filter", "2", "--temporal_filter", "2")
    assert r.returncode == 2 and "--filter" in r.stderr and "--temporal_filter" in r.stderr


@pytest.mark.parametrize("flag,value", [("--temporal_alphas", "0.2"), ("--temporal_sigmas", "1,2"), ("--camera_step", "0.1,0.2")])
def test_rt_render_refuses_malformed_values(flag, value):
    r = run_cli("--temporal_filter", "2", flag, value)
    assert r.returncode == 2 and flag in r.stderr


def test_rt_render_camera_step_needs_frames():
    r = run_cli("--camera_step", "0.1,0,0")
    assert r.returncode == 2 and "--frames" in r.stderr


def test_rt_render_help_names_the_temporal_filter():
    r = run_cli("--help")
    assert r.returncode == 0 and "--temporal_filter n" in r.stdout and "--camera_step" in r.stdout
