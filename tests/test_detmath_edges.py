"""rt_detmath.h's host build (through oracle.c's orc_debug_eval) against mpmath at 200 bits, rounded once to binary32, on
the edge sets of tests/_detmath_cases.py; special values against the C99 / IEEE 754 tables written out below.

The header's own promise is the condition: every result within 1 ulp of the correctly rounded value, and -- at ~1e-7
misrounded per point and ~4000 points per set -- at most 1 result per set that is not equal to it (ldexp: exact, 0).
Measured with this file: 0 differing results in every set."""
import math
import mpmath
import numpy as np
import pytest
from tests import _oracle
from tests import _detmath_cases as K

PREC = 200
CPU_N = 4000
f32 = np.float32
INF, NAN = K.INF, K.NAN


def bits(v):
    return np.asarray(v, f32).view(np.uint32)


def ordered(v):
    """binary32 -> integers in value order, one step per ulp (-0 and +0 both 0)"""
    b = bits(v).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


def round_to_binary32(v):
    """An mpmath number rounded once to binary32: ties to even, ulp fixed at 2^-149 below 2^-126, overflow to inf.  A
    negative value that rounds to zero gives -0; an exact zero gives +0 (mpmath has no signed zero)."""
    v = mpmath.mpf(v)
    if mpmath.isnan(v):
        return NAN
    if mpmath.isinf(v):
        return INF if v > 0 else -INF
    sign, man, exp, _ = v._mpf_
    man = int(man)
    if man == 0:
        return f32(0.0)
    s = -1.0 if sign else 1.0
    e = man.bit_length() + exp                 # 2^(e-1) <= |v| < 2^e
    if e > 129:
        return f32(s * np.inf)
    if e < -151:
        return f32(s * 0.0)
    q = max(e - 24, -149)                      # exponent of the ulp
    shift = q - exp
    if shift <= 0:
        n = man << -shift
    else:
        n, rem, half = man >> shift, man & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (n & 1)):
            n += 1
    r = math.ldexp(n, q)                       # n <= 2^24: exact in binary64
    if r >= 2.0 ** 128:
        return f32(s * np.inf)
    return f32(s * r)


def test_the_rounding_helper_on_hand_written_values():
    two = mpmath.mpf(2)
    with mpmath.workprec(PREC):
        cases = [
            (mpmath.mpf(1), 0x3F800000),
            (mpmath.mpf(1) / 3, 0x3EAAAAAB),
            (1 + two ** -24, 0x3F800000),                       # tie -> even (down)
            (1 + two ** -24 + two ** -100, 0x3F800001),         # just above the tie
            (1 + 3 * two ** -24, 0x3F800002),                   # tie -> even (up)
            (-(1 + 3 * two ** -24), 0xBF800002),
            (two ** -150, 0x00000000),                          # half the smallest subnormal: tie -> 0
            (two ** -150 + two ** -300, 0x00000001),
            (-(two ** -151), 0x80000000),                       # negative underflow keeps its sign
            (3 * two ** -150, 0x00000002),                      # 1.5 subnormal ulps: tie -> even
            (two ** -126 - two ** -150, 0x00800000),            # the largest subnormal plus half an ulp: tie -> the smallest normal
            (two ** -126 - two ** -149, 0x007FFFFF),
            (two ** 128 - two ** 104, 0x7F7FFFFF),              # FLT_MAX
            (two ** 128 - two ** 103, 0x7F800000),              # FLT_MAX plus half an ulp: tie -> 2^128 = inf
            (two ** 128 - two ** 103 - two ** 20, 0x7F7FFFFF),
            (-(two ** 200), 0xFF800000),
            (mpmath.mpf(0), 0x00000000),
            (mpmath.mpf("inf"), 0x7F800000),
            (mpmath.pi, 0x40490FDB),
        ]
        for v, want in cases:
            assert int(bits(round_to_binary32(v))) == want, (v, hex(want))
        assert np.isnan(round_to_binary32(mpmath.mpf("nan")))


def reference(fn, *cols):
    """fn (an mpmath function of mpf arguments) over binary32 columns, each value rounded once to binary32"""
    with mpmath.workprec(PREC):
        return np.array([round_to_binary32(fn(*[mpmath.mpf(float(v)) for v in row])) for row in zip(*cols)], f32)


def report(name, setname, args, got, want, idx):
    lines = ["%s / %s: %d of %d" % (name, setname, len(idx), got.size)]
    for i in idx[:8]:
        lines.append("  in %s  got %08x  want %08x" % (" ".join("%08x" % int(bits(a)[i]) for a in args), int(bits(got)[i]), int(bits(want)[i])))
    return "\n".join(lines)


def same_bits(got, want):
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def check_accurate(name, setname, args, want, cap=1):
    got = _oracle.debug_eval(K.FN[name], *args)
    assert not np.isnan(want).any()
    differs = np.flatnonzero(~same_bits(got, want))
    far = np.flatnonzero(np.isnan(got) | (np.abs(ordered(got) - ordered(want)) > 1))
    print("%s / %s: %d points, %d differ from the correctly rounded value, %d by more than 1 ulp" % (name, setname, got.size, len(differs), len(far)))
    assert len(far) == 0, report(name, setname, args, got, want, far)
    assert len(differs) <= cap, report(name, setname, args, got, want, differs)


def check_table(name, args, want):
    got = _oracle.debug_eval(K.FN[name], *args)
    bad = np.flatnonzero(~same_bits(got, want))
    assert len(bad) == 0, report(name, "table", args, got, want, bad)


# ---- sin, cos, tan ---------------------------------------------------------------------------------------------------
MP_TRIG = {"sin": mpmath.sin, "cos": mpmath.cos, "tan": mpmath.tan}


@pytest.fixture(scope="module")
def trig():
    return K.trig_sets(CPU_N)


@pytest.mark.parametrize("setname", ["A", "B", "C"])
@pytest.mark.parametrize("name", ["sin", "cos", "tan"])
def test_trig_is_correctly_rounded_on_its_accurate_domain(trig, name, setname):
    args = trig[setname]
    check_accurate(name, setname, args, reference(MP_TRIG[name], *args))


def test_trig_special_values_and_the_range_gate(trig):
    """C99's values at +-0, inf and NaN; and the header's own gate: |x| >= 1e9 (1e9f itself included) is NaN by definition"""
    gate = K.TRIG_GATE
    x = np.array([0.0, -0.0, INF, -INF, NAN, K.FLT_MAX, -K.FLT_MAX, gate, -gate, K.up(gate), -K.up(gate)], f32)
    nan9 = [NAN] * 9
    check_table("sin", (x,), np.array([0.0, -0.0] + nan9, f32))
    check_table("cos", (x,), np.array([1.0, 1.0] + nan9, f32))
    check_table("tan", (x,), np.array([0.0, -0.0] + nan9, f32))
    (d,) = trig["D"]
    for name in ("sin", "cos", "tan"):
        got = _oracle.debug_eval(K.FN[name], d)
        assert np.array_equal(np.isnan(got), ~(np.abs(d) < gate)), report(name, "D", (d,), got, got, np.arange(d.size))


@pytest.mark.parametrize("name", ["sin", "cos"])
def test_trig_beyond_the_accurate_domain_stays_in_range(trig, name):
    """1e5 <= |x| < 1e9: the header claims the same bits everywhere, not accuracy -- so only finite and within [-1, 1].
    The two floats just below the gate belong here too."""
    gate = K.TRIG_GATE
    x = np.concatenate([trig["E"][0], [K.down(gate), -K.down(gate)]]).astype(f32)
    assert (np.abs(x) >= 1.0e5).all() and (np.abs(x) < gate).all()
    got = _oracle.debug_eval(K.FN[name], x)
    bad = np.flatnonzero(~(np.isfinite(got) & (np.abs(got) <= 1.0)))
    assert len(bad) == 0, report(name, "E", (x,), got, got, bad)


# ---- pow -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pows():
    return K.pow_sets(CPU_N)


def mp_pow(x, y):
    if y == 5:
        return x ** 5                     # exact in sign for negative x
    return mpmath.power(x, y)


@pytest.mark.parametrize("setname", ["wide", "gamma", "overflow", "fifth"])
def test_pow_is_correctly_rounded_away_from_its_ladder(pows, setname):
    args = pows[setname]
    check_accurate("pow", setname, args, reference(mp_pow, *args))


def is_odd_integer(y):
    return math.isfinite(y) and y == math.floor(y) and abs(y) < 2.0 ** 24 and int(y) % 2 == 1


def c99_pow(x, y):
    """C99 F.10.4.4 (OpenCL's pow has the same table), rule by rule; what no rule decides is x^y itself, correctly rounded"""
    x, y = float(x), float(y)
    odd = is_odd_integer(y)
    if y == 0:
        return f32(1)                                              # pow(x, +-0) = 1, even for NaN
    if x == 1:
        return f32(1)                                              # pow(1, y) = 1, even for NaN
    if math.isnan(x) or math.isnan(y):
        return NAN
    if x == 0:
        neg = odd and math.copysign(1.0, x) < 0                    # the sign of zero survives an odd integer y only
        return f32(-np.inf if neg else np.inf) if y < 0 else f32(-0.0 if neg else 0.0)
    if math.isinf(y):
        if x == -1:
            return f32(1)
        return f32(np.inf) if (abs(x) > 1) == (y > 0) else f32(0)
    if math.isinf(x):
        neg = odd and x < 0
        return f32(-0.0 if neg else 0.0) if y < 0 else f32(-np.inf if neg else np.inf)
    if x < 0 and y != math.floor(y):
        return NAN
    with mpmath.workprec(PREC):
        mag = mpmath.power(mpmath.mpf(abs(x)), mpmath.mpf(y))
        return round_to_binary32(-mag if (x < 0 and odd) else mag)


# a readable extract of the ladder, pinned literally: (x, y, bits of the result; None = NaN)
POW_PINS = [
    (NAN, 0.0, 0x3F800000), (NAN, -0.0, 0x3F800000), (1.0, NAN, 0x3F800000), (1.0, INF, 0x3F800000), (-1.0, INF, 0x3F800000),
    (-1.0, -INF, 0x3F800000), (NAN, 1.0, None), (2.0, NAN, None),
    (0.0, -1.0, 0x7F800000), (-0.0, -1.0, 0xFF800000), (-0.0, -3.0, 0xFF800000), (-0.0, -2.0, 0x7F800000), (-0.0, -0.5, 0x7F800000),
    (-0.0, -INF, 0x7F800000), (0.0, 3.0, 0x00000000), (-0.0, 3.0, 0x80000000), (-0.0, 5.0, 0x80000000), (-0.0, 2.0, 0x00000000),
    (-0.0, 0.5, 0x00000000), (-0.0, INF, 0x00000000), (0.0, 0.125, 0x00000000), (-0.0, -0.125, 0x7F800000), (0.0, 1.0e-30, 0x00000000),
    (-0.0, K.DENORM_MIN, 0x00000000), (0.0, -K.DENORM_MIN, 0x7F800000), (-0.0, 16777215.0, 0x80000000), (-0.0, 16777216.0, 0x00000000),
    (-INF, -1.0, 0x80000000), (-INF, -2.0, 0x00000000), (-INF, -0.5, 0x00000000), (-INF, 3.0, 0xFF800000), (-INF, 5.0, 0xFF800000),
    (-INF, 2.0, 0x7F800000), (-INF, 0.5, 0x7F800000), (-INF, INF, 0x7F800000), (-INF, -INF, 0x00000000), (-INF, -16777215.0, 0x80000000),
    (INF, -0.5, 0x00000000), (INF, 0.5, 0x7F800000), (0.5, INF, 0x00000000), (0.5, -INF, 0x7F800000), (2.0, INF, 0x7F800000),
    (-2.0, -INF, 0x00000000), (-2.0, 0.5, None), (-0.5, -0.5, None), (-2.0, 3.0, 0xC1000000), (-2.0, -3.0, 0xBE000000),
    (-2.0, 2.0, 0x40800000), (-2.0, 5.0, 0xC2000000), (-2.0, 16777215.0, 0xFF800000), (-2.0, -16777215.0, 0x80000000),
    (-0.5, 16777215.0, 0x80000000), (-2.0, 1.0e30, 0x7F800000), (-1.0, 1.0e30, 0x3F800000), (-1.0, 16777215.0, 0xBF800000),
    (K.DENORM_MIN, 2.0, 0x00000000), (K.DENORM_MIN, -1.0, 0x7F800000), (K.DENORM_MIN, 0.5, 0x1A3504F3), (K.FLT_MAX, 0.5, 0x5F7FFFFF),
    (K.FLT_MAX, -1.0, 0x00200000), (K.FLT_MAX, 2.0, 0x7F800000), (2.0, 0.5, 0x3FB504F3),
]


def test_pow_special_case_ladder(pows):
    x = np.array([p[0] for p in POW_PINS], f32)
    y = np.array([p[1] for p in POW_PINS], f32)
    want = np.array([0x7FC00000 if p[2] is None else p[2] for p in POW_PINS], np.uint32).view(f32)
    assert all(np.isnan(c99_pow(a, b)) if w is None else int(bits(c99_pow(a, b))) == w for a, b, w in POW_PINS)   # the rules say what the pins say
    check_table("pow", (x, y), want)
    lx, ly = pows["ladder"]
    assert lx.size == len(K.POW_LADDER_X) * len(K.POW_LADDER_Y)
    check_table("pow", (lx, ly), np.array([c99_pow(a, b) for a, b in zip(lx, ly)], f32))


# ---- atan2 -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def atans():
    return K.atan2_sets(CPU_N)


@pytest.mark.parametrize("setname", ["wide", "switch"])
def test_atan2_is_correctly_rounded(atans, setname):
    args = atans[setname]
    if setname == "switch":        # the set does sit on the switch points, on both sides of them and in both branches
        r = np.abs(args[0].astype(np.float64)) / np.abs(args[1].astype(np.float64))
        for s in K.ATAN2_SWITCH:
            assert (r == s).any() and ((r < s) & (r > s - 1e-6)).any() and ((r > s) & (r < s + 1e-6)).any()
            assert (1 / r == s).any()
    check_accurate("atan2", setname, args, reference(mpmath.atan2, *args))


PI, PIO2, PIO4, PI3O4 = 0x40490FDB, 0x3FC90FDB, 0x3F490FDB, 0x4016CBE4
NEG = 0x80000000
# C99 F.10.1.4, the 16 corners of zero and infinity: (y, x, bits)
ATAN2_CORNERS = [
    (0.0, 0.0, 0), (-0.0, 0.0, NEG), (0.0, -0.0, PI), (-0.0, -0.0, NEG | PI),
    (0.0, INF, 0), (-0.0, INF, NEG), (0.0, -INF, PI), (-0.0, -INF, NEG | PI),
    (INF, 0.0, PIO2), (-INF, 0.0, NEG | PIO2), (INF, -0.0, PIO2), (-INF, -0.0, NEG | PIO2),
    (INF, INF, PIO4), (-INF, INF, NEG | PIO4), (INF, -INF, PI3O4), (-INF, -INF, NEG | PI3O4),
]


def c99_atan2(y, x):
    y, x = float(y), float(x)
    if math.isnan(x) or math.isnan(y):
        return NAN
    if (y == 0 or math.isinf(y)) and (x == 0 or math.isinf(x)):
        return [np.uint32(b).view(f32) for cy, cx, b in ATAN2_CORNERS
                if (cy == y and math.copysign(1, cy) == math.copysign(1, y) and cx == x and math.copysign(1, cx) == math.copysign(1, x))][0]
    sy = NEG if math.copysign(1.0, y) < 0 else 0
    if y == 0 or math.isinf(x):                                    # finite y against an infinite x, zero y against a finite x
        return np.uint32(sy | (PI if x < 0 else 0)).view(f32)
    if x == 0 or math.isinf(y):
        return np.uint32(sy | PIO2).view(f32)
    with mpmath.workprec(PREC):
        return round_to_binary32(mpmath.atan2(mpmath.mpf(y), mpmath.mpf(x)))


def test_atan2_zero_infinity_and_nan_table(atans):
    with mpmath.workprec(PREC):
        assert [int(bits(round_to_binary32(v))) for v in (mpmath.pi, mpmath.pi / 2, mpmath.pi / 4, 3 * mpmath.pi / 4)] == [PI, PIO2, PIO4, PI3O4]
    y = np.array([c[0] for c in ATAN2_CORNERS], f32)
    x = np.array([c[1] for c in ATAN2_CORNERS], f32)
    check_table("atan2", (y, x), np.array([c[2] for c in ATAN2_CORNERS], np.uint32).view(f32))
    sy, sx = atans["special"]
    check_table("atan2", (sy, sx), np.array([c99_atan2(a, b) for a, b in zip(sy, sx)], f32))


# ---- acos ------------------------------------------------------------------------------------------------------------
def test_acos_is_correctly_rounded_up_to_and_at_the_ends():
    s = K.acos_sets(CPU_N)
    (z,) = s["inside"]
    assert {0x3F800000, 0xBF800000, 0, NEG, 0x3F7FFFFF, 0xBF7FFFFF} <= set(int(b) for b in bits(z))
    check_accurate("acos", "inside", (z,), reference(mpmath.acos, z))
    four = np.array([1.0, -1.0, 0.0, -0.0], f32)
    check_table("acos", (four,), np.array([0, PI, PIO2, PIO2], np.uint32).view(f32))
    (o,) = s["outside"]
    assert (~(np.abs(o) <= 1)).all()
    check_table("acos", (o,), np.full(o.size, NAN, f32))


# ---- exp -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setname", ["uniform", "tiny", "ln2", "thresholds", "special"])
def test_exp_is_correctly_rounded_into_the_subnormals_and_out_of_range(setname):
    (x,) = K.exp_sets(CPU_N)[setname]
    if setname == "special":
        t = np.array([0.0, -0.0, INF, -INF, NAN], f32)
        check_table("exp", (t,), np.array([1.0, 1.0, INF, 0.0, NAN], f32))
        x = x[np.isfinite(x)]
    want = reference(mpmath.exp, x)
    if setname == "thresholds":    # the set does cross all three thresholds
        assert {0x00000000, 0x00000001, 0x7F800000} <= set(int(b) for b in bits(want))
        assert ((want > 0) & (want < K.FLT_MIN)).any() and ((want >= K.FLT_MIN) & (want < 2 * K.FLT_MIN)).any()
        assert (np.isfinite(want) & (want > K.FLT_MAX / 2)).any()
    if setname == "uniform":
        assert (want == 0).any() and ((want > 0) & (want < K.FLT_MIN)).any() and np.isinf(want).any()
    check_accurate("exp", setname, (x,), want)


# ---- ldexp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setname", ["range", "clamp"])
def test_ldexp_is_exact(setname):
    """x 2^k rounded once.  Every finite nonzero binary32 lies in [2^-149, 2^128), so beyond |k| = 400 the result is 0 or inf
    whatever k is: the reference clamps k there only to keep the numbers small."""
    x, kb = K.ldexp_sets(CPU_N)[setname]
    k = kb.view(np.int32)
    if setname == "clamp":
        assert {600, -600, 601, -601, K.INT_MAX, K.INT_MIN} <= set(int(v) for v in k)
    want = np.empty_like(x)
    with mpmath.workprec(PREC):
        for i, (xv, kv) in enumerate(zip(x, k)):
            if xv == 0 or not np.isfinite(xv):
                want[i] = xv                                    # +-0, +-inf and NaN come back as they are
            else:
                want[i] = round_to_binary32(mpmath.ldexp(mpmath.mpf(float(xv)), int(np.clip(kv, -400, 400))))
    got = _oracle.debug_eval(K.FN["ldexp"], x, kb)
    bad = np.flatnonzero(~same_bits(got, want))
    print("ldexp / %s: %d points, %d differ" % (setname, x.size, len(bad)))
    assert len(bad) == 0, report("ldexp", setname, (x, kb), got, want, bad)


# ---- the IEEE leaves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["div32", "div64", "sqrt32", "sqrt64"])
def test_host_divide_and_sqrt_are_ieee(name):
    """the host side of codes 6, 7, 12 and 13 against numpy's binary32 and binary64 operations"""
    for setname, args in K.sets(name, CPU_N).items():
        with np.errstate(all="ignore"):
            if name == "div32":
                want = args[0] / args[1]
            elif name == "div64":
                want = (args[0].astype(np.float64) / args[1].astype(np.float64)).astype(f32)
            elif name == "sqrt32":
                want = np.sqrt(args[0])
            else:
                want = np.sqrt(args[0].astype(np.float64)).astype(f32)
        got = _oracle.debug_eval(K.FN[name], *args)
        bad = np.flatnonzero(~same_bits(got, want))
        assert len(bad) == 0, report(name, setname, args, got, want, bad)
    if name.startswith("div"):      # the pairs do reach subnormal quotients and both sides of the overflow boundary
        a, b = K.sets(name, CPU_N)["subnormal"]
        q = np.abs(a.astype(np.float64) / b.astype(np.float64))
        assert ((q < float(K.FLT_MIN)) & (q > float(K.DENORM_MIN))).any() and (q < float(K.DENORM_MIN) / 2).any()
        a, b = K.sets(name, CPU_N)["overflow"]
        q = np.abs(a.astype(np.float64) / b.astype(np.float64))
        assert (q > float(K.FLT_MAX)).any() and (q < float(K.FLT_MAX)).any()


def test_case_sets_are_seeded_binary32_and_small_enough_for_one_launch():
    for name in K.FN:
        total = 0
        for setname, args in K.sets(name).items():
            again = K.sets(name)[setname]
            for a, b in zip(args, again):
                assert a.dtype == np.float32 and a.ndim == 1 and a.size == args[0].size and 0 < a.size <= 2 ** 16
                assert np.array_equal(bits(a), bits(b))
            total += args[0].size
        assert total <= 2 ** 16, (name, total)
