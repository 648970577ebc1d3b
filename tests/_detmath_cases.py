"""Edge inputs for rt_detmath.h's functions and the IEEE leaf operations under them, shared by tests/test_detmath_edges.py
(host against a high-precision reference) and tests/test_gpu_detmath_edges.py (device against host, bit for bit).

Every generator is seeded, returns binary32 arrays and takes `n`, the number of points of each random part; what is
enumerated (specials, neighbours of a threshold, the pow ladder) does not scale with it.  sets(name, n) returns
{set name: (a,) or (a, b)} in debug_eval's argument order.  At the default n the sets of one function concatenate to
fewer than 2^16 elements, so that the divergence test is one launch."""
import itertools
import numpy as np

# debug_eval's function codes (k_debug_eval in raygen_kernels.h, orc_debug_eval in oracle.c)
FN = {"sin": 0, "cos": 1, "tan": 2, "pow": 3, "atan2": 4, "acos": 5, "sqrt32": 6, "div32": 7, "exp": 10, "ldexp": 11,
      "div64": 12, "sqrt64": 13}
DEVICE_N = 12000

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny           # 2^-126, the smallest normal
DENORM_MIN = np.uint32(1).view(np.float32)    # 2^-149
TRIG_GATE = f32(1.0e9)                        # rtd_sincos answers NaN from here on
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def up(x):
    return np.nextafter(np.asarray(x, f32), INF)


def down(x):
    return np.nextafter(np.asarray(x, f32), -INF)


def around(x, k=1):
    """x and its k float neighbours on either side, flattened"""
    x = np.asarray(x, f32).ravel()
    cols, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = down(lo), up(hi)
        cols += [lo, hi]
    return np.stack(cols, 1).ravel()


def signs(rng, n):
    return np.where(rng.rand(n) < 0.5, -1.0, 1.0)


def log_uniform(rng, n, lo, hi, signed=True):
    """+-10^U(lo, hi) rounded to binary32; never zero (what falls below the smallest subnormal becomes it) and never inf"""
    m = np.clip(10.0 ** rng.uniform(lo, hi, n), float(DENORM_MIN), float(FLT_MAX))
    return (m * (signs(rng, n) if signed else 1.0)).astype(f32)


def random_bits(rng, n):
    """uniformly random bit patterns; a NaN pattern becomes the infinity of its sign, so no payload goes in"""
    u = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = ((u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((u & np.uint32(0x007FFFFF)) != 0)
    u[nan] &= np.uint32(0xFF800000)
    return u.view(f32)


def int_bits(k):
    """ints carried as the bit pattern of a float (code 11's second argument)"""
    return np.asarray(k, np.int64).astype(np.int32).view(f32)


def cross(xs, ys):
    p = np.array(list(itertools.product(xs, ys)), f32)
    return p[:, 0].copy(), p[:, 1].copy()


# ---- sin, cos, tan ---------------------------------------------------------------------------------------------------
def trig_sets(n=DEVICE_N):
    rng = np.random.RandomState(101)
    k = np.concatenate([np.arange(-64, 65), rng.randint(-60000, 60001, n // 3)])
    a = around((k * (np.pi / 2)).astype(f32))                                  # A: next to k pi/2, where the reduction cancels
    b = rng.uniform(-1.0e5, 1.0e5, n).astype(f32)                              # B: the accurate domain
    c = log_uniform(rng, n, -45, 0)                                            # C: small down to subnormal
    gate = [TRIG_GATE, down(TRIG_GATE), up(TRIG_GATE)]
    d = np.array([0.0, -0.0, INF, -INF, NAN, FLT_MAX, -FLT_MAX] + gate + [-g for g in gate], f32)
    e = np.minimum(10.0 ** rng.uniform(5, 9, n), float(down(TRIG_GATE))) * signs(rng, n)   # E: deterministic, no accuracy claim
    return {"A": (a,), "B": (b,), "C": (c,), "D": (d,), "E": (e.astype(f32),)}


# ---- pow -------------------------------------------------------------------------------------------------------------
POW_LADDER_X = [0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, 2.0, -2.0, 0.5, -0.5, DENORM_MIN, FLT_MAX]
POW_LADDER_Y = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 5.0, INF, -INF, NAN, 16777216.0, -16777216.0,
                16777215.0, -16777215.0, 1.0e30, -1.0e30,
                # beyond the listed ladder: |y| so small that only rt_powf's own zero branch answers 0 or inf for x = +-0
                # (rtd_log(0) is about -709, so y log x leaves the range where exp underflows once |y| < 0.14)
                0.125, -0.125, 1.0e-30, -1.0e-30, DENORM_MIN, -DENORM_MIN]


def pow_sets(n=DEVICE_N):
    rng = np.random.RandomState(102)
    wide = (log_uniform(rng, n, -45, 38, signed=False), rng.uniform(-8, 8, n).astype(f32))
    lut = np.minimum(np.maximum(np.arange(256, dtype=f32) / f32(255.0), f32(0)), f32(1))    # k_fill_gamma_lut's inputs
    u = np.concatenate([log_uniform(rng, n, -45, 0, signed=False), lut])
    gamma = (u, np.full_like(u, 2.2))
    overflow = (rng.uniform(0.5, 2.0, n).astype(f32), rng.uniform(-120, 120, n).astype(f32))
    x5 = np.concatenate([log_uniform(rng, n, -45, 38.5), rng.uniform(-2, 2, n // 4).astype(f32)])
    fifth = (x5, np.full_like(x5, 5.0))
    return {"wide": wide, "gamma": gamma, "overflow": overflow, "fifth": fifth, "ladder": cross(POW_LADDER_X, POW_LADDER_Y)}


# ---- atan2 (argument order: y, x) ------------------------------------------------------------------------------------
ATAN2_SWITCH = (0.125, 0.375, 0.625, 0.875, 1.0)     # rtd_atan01's table switch points and the ay <= ax branch
ATAN2_FINITE = [1.0, -1.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, 0.75, -3.0]


def atan2_sets(n=DEVICE_N):
    rng = np.random.RandomState(103)
    wide = (log_uniform(rng, n, -45, 38), log_uniform(rng, n, -45, 38))
    m = n // 30
    nums, dens = [], []
    for ratio in ATAN2_SWITCH:
        den = (log_uniform(rng, m, -30, 30, signed=False).view(np.uint32) & np.uint32(0xFFFFFFF8)).view(f32)   # three low bits clear: ratio * den is exact
        nums.append(around((den.astype(np.float64) * ratio).astype(f32)))     # [on the ratio (or nearest to it), below, above] per den
        dens.append(np.repeat(den, 3))
    sm, bg = np.concatenate(nums), np.concatenate(dens)
    y = np.concatenate([sm, bg])                                              # ay <= ax, then swapped: ay >= ax
    x = np.concatenate([bg, sm])
    switch = ((y * signs(rng, y.size)).astype(f32), (x * signs(rng, x.size)).astype(f32))
    zi = [0.0, -0.0, INF, -INF]
    sy, sx = cross(zi, zi)                                                     # the 16 corners
    fy, fx = cross(ATAN2_FINITE, zi)
    gy, gx = cross(zi, ATAN2_FINITE)
    ny, nx = cross([NAN], zi + ATAN2_FINITE + [NAN])
    my, mx = cross(zi + ATAN2_FINITE, [NAN])
    special = (np.concatenate([sy, fy, gy, ny, my]), np.concatenate([sx, fx, gx, nx, mx]))
    return {"wide": wide, "switch": switch, "special": special}


# ---- acos ------------------------------------------------------------------------------------------------------------
def steps(x, toward, count):
    out, x = [], f32(x)
    for _ in range(count):
        out.append(x)
        x = np.nextafter(x, f32(toward))
    return np.array(out, f32)


def acos_sets(n=DEVICE_N):
    rng = np.random.RandomState(104)
    near = (1.0 - 10.0 ** rng.uniform(-8, 0, n // 2)).astype(f32)
    inside = np.concatenate([rng.uniform(-1, 1, n).astype(f32), near, -near, steps(1, 0, 64), steps(-1, 0, 64),
                             np.array([0.0, -0.0, 1.0, -1.0], f32)])
    outside = np.concatenate([steps(1, 2, 65)[1:], steps(-1, -2, 65)[1:], log_uniform(rng, 64, 0.001, 38),
                              np.array([INF, -INF, NAN, FLT_MAX, -FLT_MAX], f32)])
    return {"inside": (inside,), "outside": (outside,)}


# ---- exp -------------------------------------------------------------------------------------------------------------
EXP_THRESHOLDS = (-150 * np.log(2.0), -126 * np.log(2.0), 128 * np.log(2.0))   # result 0 / first subnormal result / overflow


def exp_sets(n=DEVICE_N):
    rng = np.random.RandomState(105)
    uniform = rng.uniform(-104, 89, n).astype(f32)
    tiny = log_uniform(rng, n, -40, 0)
    ln2 = around((np.arange(-150, 129) * np.log(2.0)).astype(f32))
    edge = np.concatenate([around(f32(t), 8) for t in EXP_THRESHOLDS] + [around(f32(-149 * np.log(2.0)), 8)])
    special = np.array([0.0, -0.0, INF, -INF, NAN, FLT_MAX, -FLT_MAX, DENORM_MIN, -DENORM_MIN, 700.0, -700.0, 701.0, -701.0], f32)
    return {"uniform": (uniform,), "tiny": (tiny,), "ln2": (ln2,), "thresholds": (edge,), "special": (special,)}


# ---- ldexp -----------------------------------------------------------------------------------------------------------
LDEXP_X = [0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, 1.5, DENORM_MIN, -DENORM_MIN, FLT_MIN, down(FLT_MIN), FLT_MAX, -FLT_MAX,
           f32(0.7), f32(-3.1415927)]
LDEXP_K = [0, 1, -1, 127, 128, -126, -127, -149, -150, 149, 150, 276, 277, -277, -278, 300, -300, 600, -600, 601, -601, INT_MAX, INT_MIN]


def ldexp_sets(n=DEVICE_N):
    rng = np.random.RandomState(106)
    x = random_bits(rng, n)
    sub = (rng.randint(1, 2 ** 23, n // 4).astype(np.uint32) | (rng.randint(0, 2, n // 4).astype(np.uint32) << np.uint32(31))).view(f32)
    x = np.concatenate([x, sub])
    k = rng.randint(-300, 301, x.size)
    cx = np.repeat(np.array(LDEXP_X, f32), len(LDEXP_K))
    ck = np.tile(np.array(LDEXP_K, np.int64), len(LDEXP_X))
    return {"range": (x, int_bits(k)), "clamp": (cx, int_bits(ck))}


# ---- IEEE divide and sqrt, in binary32 (codes 6, 7) and through binary64 (codes 12, 13) -----------------------------------
LEAF_SPECIAL = [0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, down(FLT_MIN), FLT_MAX, -FLT_MAX, 3.0]


def div_sets(n=DEVICE_N):
    rng = np.random.RandomState(107)
    bits = (random_bits(rng, n), random_bits(rng, n))
    m = n // 2
    den = log_uniform(rng, m, 0, 8)
    sub = (log_uniform(rng, m, -38, -30), den)                                 # quotients across the subnormal range, down to 0
    sub2 = ((rng.randint(1, 2 ** 23, m).astype(np.uint32)).view(f32), rng.uniform(0.25, 4, m).astype(f32))   # subnormal operands
    y = rng.uniform(0.5, 1.0, m).astype(f32)
    edge = (around((float(FLT_MAX) * y.astype(np.float64)).astype(f32)), np.repeat(y, 3))   # quotients on either side of FLT_MAX
    return {"bits": bits, "subnormal": (np.concatenate([sub[0], sub2[0]]), np.concatenate([sub[1], sub2[1]])),
            "overflow": edge, "special": cross(LEAF_SPECIAL, LEAF_SPECIAL)}


def sqrt_sets(n=DEVICE_N):
    rng = np.random.RandomState(108)
    sub = rng.randint(1, 2 ** 23, n // 4).astype(np.uint32).view(f32)
    return {"bits": (random_bits(rng, n),), "subnormal": (np.concatenate([sub, around(FLT_MIN, 8)]),),
            "special": (np.array(LEAF_SPECIAL, f32),)}


_SETS = {"sin": trig_sets, "cos": trig_sets, "tan": trig_sets, "pow": pow_sets, "atan2": atan2_sets, "acos": acos_sets,
         "exp": exp_sets, "ldexp": ldexp_sets, "div32": div_sets, "div64": div_sets, "sqrt32": sqrt_sets, "sqrt64": sqrt_sets}


def sets(name, n=DEVICE_N):
    return _SETS[name](n)


def all_cases(n=DEVICE_N):
    """[(function name, set name)] in a fixed order, for parametrising"""
    return [(name, s) for name in FN for s in sets(name, 8)]
