/* bake.h -- the arithmetic of an occlusion bake (rt_scene_bake / rt_scene_bake_buffer / rt_debug_bake_rays / rt_debug_bake_reduce), stated
 * once for the kernels (bake_kernels.h) and the host restatement.  binary32 throughout except the sine and cosine (rt_detmath.h: binary64, rounded once),
 * -ffp-contract=off, correctly rounded divide and square root on both sides, so the two agree bit for bit.  tests/test_bake.py restates every step in numpy.
 *
 * A point = eight floats: position xyz, w ignored, normal xyz, w ignored.  With RT_BAKE_FROM_SURFACES a point is an rt_surface: its position, its shading
 * normal negated when flags bit 1 (back face) is set; a record with flags bit 0 clear (a miss) is skipped.
 * A point is SKIPPED (no ray of it is walked; unoccluded = RT_INVALID_ID, bent normal zeros) when one of the six floats is not finite, or when
 *   l2 = (nx nx + ny ny) + nz nz   is zero or not finite.
 *
 * Ray k (0 <= k < samples, samples a power of two) of the point with index i within the call (bake_ray):
 *   h1 = mix32(i ^ mix32(seed)),  h2 = mix32(h1 ^ 0x9E3779B9),   mix32(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16
 *   r1 = (h1 >> 8) * 2^-24,  r2 = (h2 >> 8) * 2^-24                                  (exact in binary32)
 *   u1 = wrap(((float)k + 0.5f) / (float)samples + r1),  wrap(x) = x >= 1 ? x - 1 : x  (the quotient is exact; one rounding in the sum, none in x - 1)
 *   u2 = wrap((float)(bitreverse32(k) >> 8) * 2^-24 + r2)                            (the radical inverse of k, cut to 24 bits, rotated)
 *   phi = RT_TWO_PI * u2;  rtd_sincos((double)phi, &s, &c);  sn = (float)s, cs = (float)c
 *   r = sqrtf(u1);  x = r * cs;  y = r * sn;  z = sqrtf(max(0, 1 - u1))               (a cosine-weighted direction about +z)
 * The frame (bake_frame): n = normal / sqrtf(l2), three divides (query.h's normalize3); with sg = copysignf(1, n.z), a = -1 / (sg + n.z), b = (n.x * n.y) * a:
 *   t  = (1 + ((sg * n.x) * n.x) * a,  sg * b,  (-sg) * n.x)
 *   bt = (b,  sg + (n.y * n.y) * a,  -n.y)                                           (Duff et al. 2017, "Building an Orthonormal Basis, Revisited")
 *   direction = (t * x + bt * y) + n * z,  origin = position + n * bias,  t_min = 0,  t_max = radius
 *
 * The reduction (bake_reduce_point): L = min(samples, 64) slots; ray k belongs to slot k % L; a slot starts at +0 and adds the directions of its unoccluded
 * rays in rising k; the L sums are combined by the halving tree v[l] += v[l + s] for s = L/2 .. 1, l < s; S = v[0].  unoccluded = the number of unoccluded
 * rays; bent normal = S / sqrtf(l2) with l2 = (S.x S.x + S.y S.y) + S.z S.z, zeros when l2 is zero or not finite. */
#ifndef RT_BAKE_H
#define RT_BAKE_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"

#define RT_BAKE_SLOTS_MAX 64u
#define RT_BAKE_FLAGS_KNOWN (RT_BAKE_FROM_SURFACES)

struct BakeFrame
{
    float origin[3];
    float n[3], t[3], bt[3];
    bool walked;
};

RTD_FN uint32_t bake_mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

RTD_FN uint32_t bake_bitreverse32(uint32_t v)
{
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
}

/* the two rotations of point i */
RTD_FN void bake_rotations(uint32_t i, uint32_t seed, float* r1, float* r2)
{
    const uint32_t h1 = bake_mix32(i ^ bake_mix32(seed));
    const uint32_t h2 = bake_mix32(h1 ^ 0x9E3779B9u);
    *r1 = (float)(h1 >> 8) * 0x1p-24f;
    *r2 = (float)(h2 >> 8) * 0x1p-24f;
}

/* position / normal of a point record: eight floats, or an rt_surface (from_surfaces); false: a miss record */
RTD_FN bool bake_point(const float* rec, bool from_surfaces, float p[3], float nrm[3])
{
    if (!from_surfaces)
    {
        for (int k = 0; k < 3; ++k) { p[k] = rec[k]; nrm[k] = rec[4 + k]; }
        return true;
    }
    uint32_t flags;
    __builtin_memcpy(&flags, rec + 15, 4);
    for (int k = 0; k < 3; ++k) { p[k] = rec[k]; nrm[k] = (flags & 2u) ? -rec[8 + k] : rec[8 + k]; }
    return (flags & 1u) != 0u;
}

RTD_FN BakeFrame bake_frame(const float p[3], const float nrm[3], bool record_ok, float bias)
{
    BakeFrame f;
    const float l2 = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2];
    const bool finite = __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) &&
                        __builtin_isfinite(nrm[0]) && __builtin_isfinite(nrm[1]) && __builtin_isfinite(nrm[2]);
    f.walked = record_ok && finite && l2 > 0.0f && __builtin_isfinite(l2);
    if (!f.walked)
    {
        for (int k = 0; k < 3; ++k) { f.origin[k] = 0.0f; f.n[k] = 0.0f; f.t[k] = 0.0f; f.bt[k] = 0.0f; }
        return f;
    }
    const float len = __builtin_sqrtf(l2);
    for (int k = 0; k < 3; ++k) f.n[k] = nrm[k] / len;
    const float sg = __builtin_copysignf(1.0f, f.n[2]);
    const float a = -1.0f / (sg + f.n[2]);
    const float b = (f.n[0] * f.n[1]) * a;
    f.t[0] = 1.0f + ((sg * f.n[0]) * f.n[0]) * a;
    f.t[1] = sg * b;
    f.t[2] = (-sg) * f.n[0];
    f.bt[0] = b;
    f.bt[1] = sg + (f.n[1] * f.n[1]) * a;
    f.bt[2] = -f.n[1];
    for (int k = 0; k < 3; ++k) f.origin[k] = p[k] + f.n[k] * bias;
    return f;
}

/* the direction of ray k of a walked point */
RTD_FN void bake_direction(const BakeFrame& f, float r1, float r2, uint32_t k, uint32_t samples, float d[3])
{
    float u1 = ((float)k + 0.5f) / (float)samples + r1;
    if (u1 >= 1.0f) u1 = u1 - 1.0f;
    float u2 = (float)(bake_bitreverse32(k) >> 8) * 0x1p-24f + r2;
    if (u2 >= 1.0f) u2 = u2 - 1.0f;
    const float phi = RT_TWO_PI * u2;
    double s, c;
    rtd_sincos((double)phi, &s, &c);
    const float sn = (float)s, cs = (float)c;
    const float r = __builtin_sqrtf(u1);
    const float x = r * cs, y = r * sn;
    const float zz = 1.0f - u1;
    const float z = __builtin_sqrtf(zz > 0.0f ? zz : 0.0f);
    for (int q = 0; q < 3; ++q) d[q] = (f.t[q] * x + f.bt[q] * y) + f.n[q] * z;
}

/* bent normal of a point's sum S */
RTD_FN void bake_bent(const float S[3], float out[3])
{
    const float l2 = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2];
    if (l2 > 0.0f && __builtin_isfinite(l2))
    {
        const float len = __builtin_sqrtf(l2);
        for (int q = 0; q < 3; ++q) out[q] = S[q] / len;
    }
    else
        for (int q = 0; q < 3; ++q) out[q] = 0.0f;
}

#endif /* RT_BAKE_H */
