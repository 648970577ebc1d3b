// wide_quant.h -- the frame and the 8-bit planes of one 64-byte record of the 4-wide tree (layout: wide_bvh.cpp, "Record"), as ONE function for everybody who
// writes such a record: build_wide_bvh on the host, k_fold_emit on the device, and the refit of both (refit.hip).  Plain header, host and device code share it;
// binary64 arithmetic without contraction, so the host's and the device's records agree bit for bit.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_WQ_HD __host__ __device__ inline
#else
#define RT_WQ_HD inline
#endif

// The frame of a record whose box is [nmin, nmax]: per axis cell = 2^e such that 254 cells span the box (one spare for the floor of the origin) and the grid stays
// exactly representable in binary32 (origin a multiple of the cell, |origin| / cell < 2^23 leaves room for + 255 below 2^24).
// false: the record does not qualify -- a cell above 2^20 or a coordinate beyond 2^28 (k_trace_w4 evaluates slab distances as q * (cell * inv) + (origin - org) * inv:
// bounded operands keep that finite for every ray it accepts), or an origin that binary32 cannot hold (cannot happen by construction).
RT_WQ_HD bool wide_frame(const float (&nmin)[3], const float (&nmax)[3], float (&origin)[3], int (&exps)[3])
{
    for (int a = 0; a < 3; ++a)
    {
        const double extent = (double)nmax[a] - (double)nmin[a];
        const double amax = fmax(fabs((double)nmin[a]), fabs((double)nmax[a]));
        if (!(amax < 268435456.0)) return false;                   // (before the loops below: they end for finite operands only)
        int e = -126;
        if (extent > 0.0)
        {
            int ex = 0;
            const double m = frexp(extent / 254.0, &ex);           // extent / 254 = m * 2^ex, m in [0.5, 1): ceil(log2) = ex, or ex - 1 for a power of two
            const int c = m == 0.5 ? ex - 1 : ex;
            e = c > e ? c : e;
        }
        while (ldexp(254.0, e) < extent) ++e;
        while (amax > 0.0 && amax / ldexp(1.0, e) >= 8388608.0 - 256.0) ++e;
        if (e > 20) return false;
        const double cell = ldexp(1.0, e);
        const double o = floor((double)nmin[a] / cell) * cell;
        origin[a] = (float)o;
        if ((double)origin[a] != o) return false;
        exps[a] = e;
    }
    return true;
}

RT_WQ_HD uint32_t wide_meta(const int (&exps)[3], uint32_t n_slots)
{
    return (uint32_t)(exps[0] + 127) | (uint32_t)(exps[1] + 127) << 8 | (uint32_t)(exps[2] + 127) << 16 | n_slots << 24;
}

// The grid coordinates of the box [cmin, cmax] in that frame, rounded OUTWARD.  false: the box does not lie inside the record's (cannot happen for a child of it).
RT_WQ_HD bool wide_quantise(const float (&cmin)[3], const float (&cmax)[3], const float (&origin)[3], const int (&exps)[3], uint32_t (&lo_out)[3], uint32_t (&hi_out)[3])
{
    for (int a = 0; a < 3; ++a)
    {
        const double cell = ldexp(1.0, exps[a]);
        double lo = floor(((double)cmin[a] - (double)origin[a]) / cell);
        double hi = ceil(((double)cmax[a] - (double)origin[a]) / cell);
        // the difference above is rounded (a bound of 1e-17 beside an origin of -0.2 vanishes in it): settle the
        // containment on the grid points themselves, which are exact in binary32 and binary64 alike
        while ((double)origin[a] + lo * cell > (double)cmin[a]) lo -= 1.0;
        while ((double)origin[a] + hi * cell < (double)cmax[a]) hi += 1.0;
        if (!(lo >= 0.0) || !(hi <= 255.0) || lo > hi) return false;
        lo_out[a] = (uint32_t)lo;
        hi_out[a] = (uint32_t)hi;
    }
    return true;
}
