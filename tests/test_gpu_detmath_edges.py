"""-m gpu: rt_detmath.h and the IEEE leaves under it on the device (k_debug_eval) against the same source on the host
(oracle.c's orc_debug_eval), bit for bit, on the edge sets of tests/_detmath_cases.py.  No tolerance and no case left out:
this is the contract as rt_detmath.h states it.  All NaNs count as equal (their sign and payload are not part of it)."""
import numpy as np
import pytest
from tests import _oracle
from tests import _detmath_cases as K
from raytracing_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
ODD_LENGTHS = (1, 63, 65, 257)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def bits(v):
    return np.asarray(v, f32).view(np.uint32)


def mismatches(got, want):
    return np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def report(what, name, args, got, want, idx):
    lines = ["%s: fn %d (%s), %d of %d differ" % (what, K.FN[name], name, len(idx), got.size)]
    for i in idx[:8]:
        lines.append("  [%d] in %s  device %08x  host %08x" % (i, " ".join("%08x" % int(bits(a)[i]) for a in args), int(bits(got)[i]), int(bits(want)[i])))
    return "\n".join(lines)


def check(ctx, what, name, args):
    """device == host on `args`; returns the device's result"""
    got = ctx.debug_eval(K.FN[name], *args)
    want = _oracle.debug_eval(K.FN[name], *args)
    bad = mismatches(got, want)
    assert len(bad) == 0, report(what, name, args, got, want, bad)
    return got


@pytest.mark.parametrize("name,setname", K.all_cases(), ids=["%s-%s" % c for c in K.all_cases()])
def test_device_equals_host_on_every_edge_set(ctx, name, setname):
    args = K.sets(name)[setname]
    assert 0 < args[0].size <= 2 ** 16
    got = check(ctx, "set " + setname, name, args)
    if name in ("sqrt32", "div32"):            # and both are IEEE binary32, as numpy's
        with np.errstate(all="ignore"):
            want = np.sqrt(args[0]) if name == "sqrt32" else args[0] / args[1]
        bad = mismatches(got, want)
        assert len(bad) == 0, report("set %s against numpy" % setname, name, args, got, want, bad)


@pytest.mark.parametrize("name", list(K.FN))
def test_device_results_do_not_depend_on_what_the_wave_next_to_them_does(ctx, name):
    """All sets of one function in one array: shuffled, so that the lanes of a wave leave rt_powf, rtd_atan2 and rtd_sincos
    by different exits, and sorted by value, so that they mostly leave together.  Same bits both ways, and the host's."""
    s = K.sets(name)
    cols = [np.concatenate([args[j] for args in s.values()]) for j in range(len(next(iter(s.values()))))]
    n = cols[0].size
    assert n <= 2 ** 16
    perm = np.random.RandomState(109).permutation(n)
    shuffled = [c[perm] for c in cols]
    got = check(ctx, "shuffled", name, shuffled)
    order = np.lexsort([c.astype(np.float64) for c in reversed(shuffled)])        # by the first argument, then the second; NaN last
    again = check(ctx, "sorted", name, [c[order] for c in shuffled])
    bad = mismatches(again, got[order])
    assert len(bad) == 0, report("sorted against shuffled", name, [c[order] for c in shuffled], again, got[order], bad)
    for m in ODD_LENGTHS:                                                          # a lone lane, a partial wave, a partial block
        part = check(ctx, "first %d shuffled" % m, name, [c[:m].copy() for c in shuffled])
        assert len(mismatches(part, got[:m])) == 0
