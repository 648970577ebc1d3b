/* rt_detmath.h -- deterministic transcendental library shared by every
 * implementation of the wavefront path in this repository.
 *
 * Why this exists: the reference kernels call the OpenCL builtins
 * tan/sin/cos/pow/atan2/acos/ldexp (raygeneration.cl:108, bxdf.h:53,73,160,167,
 * material.h:327-362, miss.cl:33, utils.h:156).  OpenCL leaves their rounding
 * implementation-defined (<= 4..16 ulp), so "the reference's result" is only
 * defined up to the builtin library of the device it runs on.  This project
 * pins ONE conformant definition -- evaluate in IEEE-754 binary64 with a fixed
 * sequence of + - * / sqrt operations, round once to binary32 -- and uses it in
 *   (1) the HIP kernels (raytracing_amd/csrc/, the ..._kernels.h files),
 *   (2) the C restatement oracle (oracle/oracle.c),
 *   (3) the builtin shim under the reference's own unmodified .cl kernels
 *       (oracle/ref_shim/cl_builtins.cpp, the reference-kernel build).
 * Because binary64 + - * / sqrt are correctly rounded on x86-64 and on gfx950
 * (and every translation unit is built with -ffp-contract=off and no
 * fast-math), the three agree BIT FOR BIT, which turns the radiance parity gate
 * from "rel-L2 < 1e-4" into exact equality.  Accuracy: each function is within
 * ~1e-15 relative of the true value before the final rounding, i.e. it returns
 * the correctly rounded binary32 result except in ~1e-7 of cases (<= 1 ulp).
 *
 * Plain C99, header only; compiles as C, C++ and HIP (host + device).
 * Domain notes: sin/cos/tan reduce with a 2-term Cody-Waite pi/2 and are
 * accurate for |x| < 1e5 (the path uses phi in [0, 2pi] and fov/2).  For
 * 1e5 <= |x| < 1e9 they are deterministic and within [-1, 1] but not accurate;
 * for |x| >= 1e9 (1e9f included), as for inf and NaN, they are NaN by definition.
 * Zeros, infinities and NaN follow C99 Annex F throughout (pow's and atan2's
 * tables, sin(-0) = tan(-0) = -0).  Measured edge by edge, host against a
 * 200-bit reference and device against host: tests/test_detmath_edges.py,
 * tests/test_gpu_detmath_edges.py.
 */
#ifndef RT_DETMATH_H
#define RT_DETMATH_H

#if defined(__HIPCC__)
#define RTD_FN __host__ __device__ static inline
#else
#define RTD_FN static inline
#endif

#define RTD_PIO2_HI 0x1.921fb54400000p+0
#define RTD_PIO2_LO 0x1.0b4611a626331p-34
#define RTD_TWO_OVER_PI 0x1.45f306dc9c883p-1
#define RTD_LN2_HI 0x1.62e42fee00000p-1
#define RTD_LN2_LO 0x1.a39ef35793c76p-33
#define RTD_INV_LN2 0x1.71547652b82fep+0
#define RTD_PI 0x1.921fb54442d18p+1
#define RTD_PIO2 0x1.921fb54442d18p+0
#define RTD_PIO4 0x1.921fb54442d18p-1
#define RTD_SQRT2 0x1.6a09e667f3bcdp+0

RTD_FN unsigned long long rtd_bits(double d)
{
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    return u;
}

RTD_FN double rtd_from_bits(unsigned long long u)
{
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

/* exact 2^k, k in [-1022, 1023] */
RTD_FN double rtd_pow2i(int k)
{
    return rtd_from_bits((unsigned long long)(k + 1023) << 52);
}

RTD_FN int rtd_isnan(double x) { return x != x; }

/* sin and cos of r, |r| <= pi/4 (Taylor, truncation < 1e-18) */
RTD_FN double rtd_ksin(double r)
{
    double z = r * r;
    double p = 1.0 / 355687428096000.0;               /* 1/17! */
    p = p * z - 1.0 / 1307674368000.0;                /* 1/15! */
    p = p * z + 1.0 / 6227020800.0;                   /* 1/13! */
    p = p * z - 1.0 / 39916800.0;                     /* 1/11! */
    p = p * z + 1.0 / 362880.0;                       /* 1/9!  */
    p = p * z - 1.0 / 5040.0;                         /* 1/7!  */
    p = p * z + 1.0 / 120.0;                          /* 1/5!  */
    p = p * z - 1.0 / 6.0;                            /* 1/3!  */
    return r + (r * z) * p;
}

RTD_FN double rtd_kcos(double r)
{
    double z = r * r;
    double p = 1.0 / 6402373705728000.0;              /* 1/18! */
    p = 1.0 / 20922789888000.0 - p * z;               /* 1/16! */
    p = 1.0 / 87178291200.0 - p * z;                  /* 1/14! */
    p = 1.0 / 479001600.0 - p * z;                    /* 1/12! */
    p = 1.0 / 3628800.0 - p * z;                      /* 1/10! */
    p = 1.0 / 40320.0 - p * z;                        /* 1/8!  */
    p = 1.0 / 720.0 - p * z;                          /* 1/6!  */
    p = 1.0 / 24.0 - p * z;                           /* 1/4!  */
    p = 0.5 - p * z;                                  /* 1/2!  */
    return 1.0 - z * p;
}

/* binary64 sin/cos of a binary32 argument; *s, *c may be NULL-free outputs */
RTD_FN void rtd_sincos(double x, double* s, double* c)
{
    if (!(x > -1.0e9 && x < 1.0e9))
    {
        /* outside the reduction's range, 1e9 itself included: NaN for inf and NaN as C99 has it, and NaN by definition
         * for a finite huge x (x - x would give sin = cos = 0 there); never hit on the path */
        *s = rtd_from_bits(0x7ff8000000000000ULL);
        *c = *s;
        return;
    }
    double kf = __builtin_floor(x * RTD_TWO_OVER_PI + 0.5);
    double r = (x - kf * RTD_PIO2_HI) - kf * RTD_PIO2_LO;
    int q = (int)((long long)kf & 3);
    double sr = rtd_ksin(r);
    double cr = rtd_kcos(r);
    if (q == 0)      { *s = sr;  *c = cr;  }
    else if (q == 1) { *s = cr;  *c = -sr; }
    else if (q == 2) { *s = -sr; *c = -cr; }
    else             { *s = -cr; *c = sr;  }
}

RTD_FN float rt_sinf(float x)
{
    double s, c;
    if (x == 0.0f) return x;   /* sin(-0) = -0: rtd_ksin's r + (r z) p gives -0 + +0 = +0 */
    rtd_sincos((double)x, &s, &c);
    return (float)s;
}

RTD_FN float rt_cosf(float x)
{
    double s, c;
    rtd_sincos((double)x, &s, &c);
    return (float)c;
}

RTD_FN float rt_tanf(float x)
{
    double s, c;
    if (x == 0.0f) return x;   /* tan(-0) = -0, as rt_sinf */
    rtd_sincos((double)x, &s, &c);
    return (float)(s / c);
}

/* natural log of a positive finite binary64 (normal range) */
RTD_FN double rtd_log(double x)
{
    unsigned long long b = rtd_bits(x);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    double m = rtd_from_bits((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);
    if (m > RTD_SQRT2)
    {
        m = m * 0.5;
        e = e + 1;
    }
    double s = (m - 1.0) / (m + 1.0);
    double z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    double lm = 2.0 * s + (2.0 * s) * (z * p);
    double ef = (double)e;
    return ef * RTD_LN2_HI + (ef * RTD_LN2_LO + lm);
}

/* e^t for finite t */
RTD_FN double rtd_exp(double t)
{
    if (t > 700.0) return rtd_from_bits(0x7ff0000000000000ULL);
    if (t < -700.0) return 0.0;
    double kf = __builtin_floor(t * RTD_INV_LN2 + 0.5);
    double r = (t - kf * RTD_LN2_HI) - kf * RTD_LN2_LO;
    double p = 1.0 / 87178291200.0;       /* 1/14! */
    p = p * r + 1.0 / 6227020800.0;       /* 1/13! */
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * rtd_pow2i((int)kf);
}

/* OpenCL pow(x, y) for binary32 arguments */
RTD_FN float rt_powf(float xf, float yf)
{
    double x = (double)xf;
    double y = (double)yf;
    if (yf == 0.0f) return 1.0f;
    if (xf == 1.0f) return 1.0f;
    /* pow(x, 5): Schlick's Fresnel term (bxdf.h:73), the only small-integer exponent on the path, evaluated twice
     * per shaded hit.  Three binary64 products (relative error < 4e-16 before the one rounding to binary32) instead
     * of exp(5 log x): the same definition for the kernels, the oracle and the reference shim, and with a literal
     * exponent the compiler drops everything below.  Sign, zeros, infinities and NaN come out as pow's. */
    if (yf == 5.0f)
    {
        double x2 = x * x;
        return (float)(x2 * x2 * x);
    }
    if (xf != xf || yf != yf) return xf + yf;
    /* is y an integer, and is it odd? (|y| >= 2^24 is always an even integer) */
    int y_is_int = 0, y_is_odd = 0;
    {
        double ay = y < 0.0 ? -y : y;
        if (ay >= 16777216.0) { y_is_int = 1; }
        else
        {
            double fl = __builtin_floor(ay);
            if (fl == ay)
            {
                y_is_int = 1;
                y_is_odd = (int)((long long)fl & 1);
            }
        }
    }
    double ax = x < 0.0 ? -x : x;
    double sign = 1.0;
    if (x < 0.0 || (x == 0.0 && rtd_bits(x) != 0ULL))
    {
        if (!y_is_int)
        {
            if (ax == 0.0) return y < 0.0 ? __builtin_inff() : 0.0f;
            /* a negative finite base: NaN.  pow(-inf, y) is +0 or +inf as for +inf: the infinity branch below, sign = 1 */
            if (!(ax > 1.7976931348623157e308)) return (float)((x - x) / (x - x));
        }
        if (y_is_odd) sign = -1.0;
    }
    if (ax == 0.0)
    {
        return y < 0.0 ? (float)(sign * (double)__builtin_inff()) : (float)(sign * 0.0);
    }
    if (ax > 1.7976931348623157e308)   /* inf */
    {
        return y < 0.0 ? (float)(sign * 0.0) : (float)(sign * (double)__builtin_inff());
    }
    if (y > 1.7976931348623157e308 || y < -1.7976931348623157e308)
    {
        int big = ax > 1.0;
        if (ax == 1.0) return 1.0f;
        return ((y > 0.0) == big) ? __builtin_inff() : 0.0f;
    }
    double t = y * rtd_log(ax);
    return (float)(sign * rtd_exp(t));
}

/* atan(a) for 0 <= a <= 1 */
RTD_FN double rtd_atan01(double a)
{
    int i = (int)(a * 4.0 + 0.5);
    double c = (double)i * 0.25;
    double base;
    if (i == 0)      base = 0.0;
    else if (i == 1) base = 0x1.f5b75f92c80ddp-3;   /* atan(0.25) */
    else if (i == 2) base = 0x1.dac670561bb4fp-2;   /* atan(0.5)  */
    else if (i == 3) base = 0x1.4978fa3269ee1p-1;   /* atan(0.75) */
    else             base = RTD_PIO4;               /* atan(1)    */
    double u = (a - c) / (1.0 + a * c);
    double z = u * u;
    double p = 1.0 / 21.0;
    p = 1.0 / 19.0 - p * z;
    p = 1.0 / 17.0 - p * z;
    p = 1.0 / 15.0 - p * z;
    p = 1.0 / 13.0 - p * z;
    p = 1.0 / 11.0 - p * z;
    p = 1.0 / 9.0 - p * z;
    p = 1.0 / 7.0 - p * z;
    p = 1.0 / 5.0 - p * z;
    p = 1.0 / 3.0 - p * z;
    return base + (u - (u * z) * p);
}

RTD_FN double rtd_atan2(double y, double x)
{
    if (rtd_isnan(x) || rtd_isnan(y)) return x + y;
    int xneg = (int)(rtd_bits(x) >> 63);
    int yneg = (int)(rtd_bits(y) >> 63);
    double ax = xneg ? -x : x;
    double ay = yneg ? -y : y;
    double r;
    if (ax == 0.0 && ay == 0.0)
    {
        r = 0.0;
    }
    else if (ax > 1.7976931348623157e308 && ay > 1.7976931348623157e308)
    {
        r = RTD_PIO4;
    }
    else if (ay <= ax)
    {
        r = rtd_atan01(ay / ax);
    }
    else
    {
        r = RTD_PIO2 - rtd_atan01(ax / ay);
    }
    if (xneg) r = RTD_PI - r;
    return yneg ? -r : r;
}

RTD_FN float rt_atan2f(float y, float x)
{
    return (float)rtd_atan2((double)y, (double)x);
}

RTD_FN float rt_acosf(float z)
{
    double zd = (double)z;
    return (float)(2.0 * rtd_atan2(__builtin_sqrt(1.0 - zd), __builtin_sqrt(1.0 + zd)));
}

/* ldexp(x, k) for binary32 x: exact scaling via binary64, single rounding */
RTD_FN float rt_ldexpf(float x, int k)
{
    if (k > 600) k = 600;
    if (k < -600) k = -600;
    return (float)((double)x * rtd_pow2i(k));
}

RTD_FN float rt_expf(float x)
{
    if (x != x) return x;
    return (float)rtd_exp((double)x);
}

#endif /* RT_DETMATH_H */
