/* nearest.h -- the nearest surface point to a caller-supplied point (rt_scene_nearest / rt_scene_nearest_buffer / rt_debug_nearest / rt_debug_nearest_walk;
 * DESIGN.md section 7j), stated once for the kernels (nearest.hip: k_nearest, k_nearest_brute) and the host (rt_debug_nearest(NULL, ...), rt_debug_nearest_walk).
 * binary32 throughout, -ffp-contract=off, correctly rounded divide and square root on both sides, so the two agree bit for bit.
 *
 * dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z everywhere below.
 *
 * nearest_point_triangle(p, p1, p2, p3): the region test of Ericson, Real-Time Collision Detection, section 5.1.5, in its order -- vertex A, vertex B, edge AB,
 * vertex C, edge AC, edge BC, face -- with A = p1, B = p2, C = p3:
 *   ab = p2 - p1, ac = p3 - p1, ap = p - p1, bp = p - p2, cp = p - p3
 *   d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp)
 *   vertex A  d1 <= 0 && d2 <= 0                                     (bu, bv) = (0, 0)
 *   vertex B  d3 >= 0 && d4 <= d3                                    (1, 0)
 *   edge AB   vc = d1 d4 - d3 d2 <= 0 && d1 >= 0 && d3 <= 0          (d1 / (d1 - d3), 0)
 *   vertex C  d6 >= 0 && d5 <= d6                                    (0, 1)
 *   edge AC   vb = d5 d2 - d1 d6 <= 0 && d2 >= 0 && d6 <= 0          (0, d2 / (d2 - d6))
 *   edge BC   va = d3 d6 - d5 d4 <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0      w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (1 - w, w)
 *   face      otherwise                                              s = (va + vb) + vc: (vb / s, vc / s)
 * (bu, bv) are rt_hit's: the weight of p2, the weight of p3.  From them, in this order:
 *   w0 = 1 - bu - bv
 *   q  = p1 w0 + p2 bu + p3 bv            per component, summed left to right (query.h's operand order for `position`)
 *   q  = clamped per component to [min(p1, p2, p3), max(p1, p2, p3)] with select forms (x < lo ? lo : x, then x > hi ? hi : x): a NaN passes through;
 *        lo = min(min(p1, p2), p3) with min(a, b) = b < a ? b : a, hi likewise with b > a ? b : a
 *   d  = p - q
 *   d2 = dot3(d, d)
 * A triangle whose d2 is NaN (a degenerate triangle whose quotient is 0 / 0, squares that overflow to inf - inf) is never accepted: every comparison with it is false.
 *
 * nearest_box_d2(p, lo, hi), the bound that prunes: per axis g = lo - p; t = p - hi; g = t > g ? t : g; g = g > 0 ? g : 0; then dot3(g, g).  The clamped q
 * lies component-wise inside every box that holds the triangle's corners, round-to-nearest subtraction, squaring and addition of non-negatives are each
 * monotone, so nearest_box_d2 <= d2 holds in binary32 itself and a subtree is skipped exactly when nearest_box_d2 > best (strict: a tie is visited).
 *
 * The answer for a point: best = r2 = max_distance * max_distance (rounded once; +inf stays +inf), best_prim = RT_INVALID_ID; triangle `prim` is accepted when
 * d2 < best || (d2 == best && prim < best_prim).  A point with a non-finite position component or a max_distance that is NaN or negative is not searched. */
#ifndef RT_NEAREST_H
#define RT_NEAREST_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"

#define NP_REGION_FACE 0u
#define NP_REGION_EDGE 1u
#define NP_REGION_VERTEX 2u

struct NpTriangle
{
    float q[3];          /* the clamped closest point */
    float d[3];          /* p - q */
    float d2;
    float bu, bv;
    uint32_t region;
};

RTD_FN float np_dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RTD_FN float np_min(float a, float b) { return b < a ? b : a; }
RTD_FN float np_max(float a, float b) { return b > a ? b : a; }

RTD_FN NpTriangle nearest_point_triangle(const float p[3], const float p1[3], const float p2[3], const float p3[3])
{
    NpTriangle r;
    float ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) { ab[k] = p2[k] - p1[k]; ac[k] = p3[k] - p1[k]; ap[k] = p[k] - p1[k]; bp[k] = p[k] - p2[k]; cp[k] = p[k] - p3[k]; }
    const float d1 = np_dot3(ab, ap), d2 = np_dot3(ac, ap), d3 = np_dot3(ab, bp), d4 = np_dot3(ac, bp), d5 = np_dot3(ab, cp), d6 = np_dot3(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) { r.bu = 0.0f; r.bv = 0.0f; r.region = NP_REGION_VERTEX; }
    else if (d3 >= 0.0f && d4 <= d3) { r.bu = 1.0f; r.bv = 0.0f; r.region = NP_REGION_VERTEX; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { r.bu = d1 / (d1 - d3); r.bv = 0.0f; r.region = NP_REGION_EDGE; }
    else if (d6 >= 0.0f && d5 <= d6) { r.bu = 0.0f; r.bv = 1.0f; r.region = NP_REGION_VERTEX; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { r.bu = 0.0f; r.bv = d2 / (d2 - d6); r.region = NP_REGION_EDGE; }
    else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f)
    {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        r.bu = 1.0f - w; r.bv = w; r.region = NP_REGION_EDGE;
    }
    else
    {
        const float s = (va + vb) + vc;
        r.bu = vb / s; r.bv = vc / s; r.region = NP_REGION_FACE;
    }
    const float w0 = 1.0f - r.bu - r.bv;
    for (int k = 0; k < 3; ++k)
    {
        const float lo = np_min(np_min(p1[k], p2[k]), p3[k]), hi = np_max(np_max(p1[k], p2[k]), p3[k]);
        float x = p1[k] * w0 + p2[k] * r.bu + p3[k] * r.bv;
        x = x < lo ? lo : x;
        x = x > hi ? hi : x;
        r.q[k] = x;
        r.d[k] = p[k] - x;
    }
    r.d2 = np_dot3(r.d, r.d);
    return r;
}

RTD_FN float nearest_box_d2(const float p[3], const float lo[3], const float hi[3])
{
    float g[3];
    for (int k = 0; k < 3; ++k)
    {
        float x = lo[k] - p[k];
        const float t = p[k] - hi[k];
        x = t > x ? t : x;
        g[k] = x > 0.0f ? x : 0.0f;
    }
    return np_dot3(g, g);
}

/* decided before any walk */
RTD_FN bool nearest_searched(const float p[3], float max_distance)
{
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) && max_distance >= 0.0f;     /* a NaN max_distance fails the comparison */
}

RTD_FN bool nearest_accepts(float d2, uint32_t prim, float best, uint32_t best_prim) { return d2 < best || (d2 == best && prim < best_prim); }

RTD_FN rt_nearest nearest_none(void)
{
    rt_nearest o;
    o.position[0] = o.position[1] = o.position[2] = 0.0f;
    o.distance = 0.0f; o.bc[0] = o.bc[1] = 0.0f;
    o.primitive_id = RT_INVALID_ID; o.flags = 0u;
    return o;
}

/* the record of the accepted triangle: flags = FOUND | BACK_SIDE when dot3(p - q, cross3(p2 - p1, p3 - p1)) < 0 | the region */
RTD_FN rt_nearest nearest_record(const float p[3], const float p1[3], const float p2[3], const float p3[3], uint32_t prim)
{
    const NpTriangle t = nearest_point_triangle(p, p1, p2, p3);
    const float ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
    const float bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
    const float g[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};          /* query.h's geometric normal, not normalised */
    rt_nearest o;
    for (int k = 0; k < 3; ++k) o.position[k] = t.q[k];
    o.distance = __builtin_sqrtf(t.d2);
    o.bc[0] = t.bu; o.bc[1] = t.bv;
    o.primitive_id = prim;
    o.flags = RT_NEAREST_FOUND | (np_dot3(t.d, g) < 0.0f ? RT_NEAREST_BACK_SIDE : 0u) | (t.region << RT_NEAREST_FEATURE_SHIFT);
    return o;
}

#endif /* RT_NEAREST_H */
