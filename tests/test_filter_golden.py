"""The spatial and temporal filters' outputs pinned bit for bit.  tests/golden/filters.npz holds random inputs (NaN, invalid and
demodulation-overflow pixels among them) and what rt_debug_filter / rt_debug_filter_temporal computed for them; tests/golden/filters_frame.npz
holds one frame's guides, rt_frame_filter and three rt_frame_filter_temporal calls on a moving camera.  Both were recorded by
tests/golden/make_filter_golden.py.  The numpy restatements (test_spatial_filter.py, test_temporal_filter.py) agree with the filters only within
a tolerance, and the -m gpu tests compare the kernels with a host restatement compiled from the same header: these pins are what notices a
changed order of operations.  The host restatement needs no GPU; the kernels and the frame are -m gpu."""
import os
import re

import numpy as np
import pytest

from raytracing_amd import capi
from tests.golden import make_filter_golden as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "filters.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, NaN for NaN (a NaN's payload may differ between the host and the device)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a)), bits(np.where(nb, 0, b)))


def replay(ctx, z):
    """every recorded case through rt_debug_filter* on ctx (None: the host restatement); returns how many arrays were compared"""
    n = 0
    for key in z.files:
        m = re.fullmatch(r"(\d+x\d+)/spatial_it(\d+)_d(\d)", key)
        if m:
            tag, it, demod = m.group(1), int(m.group(2)), int(m.group(3))
            assert same(G.run_spatial(ctx, z, tag, it, demod), z[key]), key
            n += 1
        m = re.fullmatch(r"(\d+x\d+)/temporal_it(\d+)_d(\d)_m(\d)/image", key)
        if m:
            tag, it, demod, moving = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
            for name, got in zip(("image", "hist", "moments"), G.run_temporal(ctx, z, tag, it, demod, moving)):
                assert same(got, z[key[:-len("image")] + name]), key[:-len("image")] + name
                n += 1
    return n


def test_host_restatement_reproduces_pins(pins):
    assert replay(None, pins) == 2 * (5 * 2 + 3 * 2 * 2 * 3)     # two sizes: 10 spatial outputs, 12 temporal cases of 3 arrays


@pytest.mark.gpu
def test_kernels_reproduce_pins(pins):
    ctx = capi.Context(0)
    try:
        assert replay(ctx, pins) == 2 * (5 * 2 + 3 * 2 * 2 * 3)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_frame_reproduces_pins(golden_scenes):
    z = np.load(os.path.join(GOLDEN, "filters_frame.npz"))
    ctx = capi.Context(0)
    try:
        got = G.run_frame(ctx, golden_scenes["cornell"], z["camera"])
    finally:
        ctx.close()
    assert sorted(got) == sorted(k for k in z.files if k != "camera")
    for k, v in got.items():
        assert same(v, z[k]), k
