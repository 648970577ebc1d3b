/* all_hits.h -- every surface a caller's ray crosses (rt_scene_trace_all / rt_scene_trace_all_buffer / rt_frame_pick_all / rt_debug_trace_all; DESIGN.md
 * section 7k), stated once for the kernels (all_hits.hip: k_all_hits, k_all_hits_brute) and the host (rt_debug_trace_all(NULL, ...)).  binary32 throughout,
 * -ffp-contract=off, correctly rounded divide on both sides, so the two agree bit for bit.
 *
 * dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z and cross3(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x): device_math.h's.
 *
 * ah_triangle is RayTriangle (trace_kernels.h's ray_triangle, trace_bvh.cl:28-73) on a trace-triangle record (p1, e1 = fl(p2 - p1), e2 = fl(p3 - p1)) with ONE
 * rule changed: ray_triangle rejects every det < 1e-8, i.e. it culls back faces; ah_triangle rejects only |det| < 1e-8 and hands det back, so a crossing from
 * behind is a member too -- without it there would be no exits to count.  For det >= 1e-8 the operations and their order are ray_triangle's: bc and t of an
 * ENTERING member are bit for bit the ray query's.  For det <= -1e-8 the same formulas run with a negative 1/det (two-sided Moeller-Trumbore).  The range
 * test is written t >= t_min && t <= t_max, so a NaN (det, u, v or t from an overflowing intermediate) is no member, where ray_triangle's negated form lets
 * one through: the one difference on front faces, and only for coordinates whose products overflow binary32.
 *
 * ah_box is RayBounds (trace_kernels.h's box_test, trace_bvh.cl:85-97) in its select forms.  box_test_fast, which the device takes for rays that are not
 * RT_SIGN_SLOW, gives the same verdict for them (no NaN can arise: trace_kernels.h), so the host uses this one form for every ray.
 *
 * AhList keeps the RT_ALL_HITS_MAX smallest (t, primitive_id) pairs in ascending order, t compared as binary32.  Insertion is a compare-and-shift chain over
 * static indices (registers on the device, never an indexed per-lane array). */
#ifndef RT_ALL_HITS_H
#define RT_ALL_HITS_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"

/* a ray that is walked: every component finite and a direction that is not all zeros (walk::ray_walkable's rule) */
RTD_FN bool ah_walkable(const float o[4], const float d[4])
{
    bool finite = true;
    for (int k = 0; k < 4; ++k) finite = finite && __builtin_isfinite(o[k]) && __builtin_isfinite(d[k]);
    return finite && !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f);
}

/* 1 / dir (ray_inverse's; the slow flag only chooses the device's box-test form, which changes no verdict) */
RTD_FN void ah_inverse(const float d[3], float inv[3])
{
    for (int k = 0; k < 3; ++k) inv[k] = 1.0f / d[k];
}

RTD_FN float ah_min(float x, float y) { return y < x ? y : x; }       /* OpenCL 1.2 6.12.4 */
RTD_FN float ah_max(float x, float y) { return x < y ? y : x; }

RTD_FN bool ah_box(const float lo[3], const float hi[3], const float o[3], const float inv[3], float t_min, float t_max)
{
    const float t0x = (lo[0] - o[0]) * inv[0], t0y = (lo[1] - o[1]) * inv[1], t0z = (lo[2] - o[2]) * inv[2];
    const float t1x = (hi[0] - o[0]) * inv[0], t1y = (hi[1] - o[1]) * inv[1], t1z = (hi[2] - o[2]) * inv[2];
    const float lox = ah_min(t0x, t1x), loy = ah_min(t0y, t1y), loz = ah_min(t0z, t1z);
    const float hix = ah_max(t0x, t1x), hiy = ah_max(t0y, t1y), hiz = ah_max(t0z, t1z);
    const float tmin = ah_max(ah_max(ah_max(lox, loy), loz), t_min);
    const float tmax = ah_min(ah_min(ah_min(hix, hiy), hiz), t_max);
    return tmax >= tmin;
}

RTD_FN bool ah_triangle(const float o[3], const float d[3], const float p1[3], const float e1[3], const float e2[3], float t_min, float t_max,
    float* u_out, float* v_out, float* t_out, float* det_out)
{
    const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (!(det >= 1e-8f || -det >= 1e-8f)) return false;
    const float inv_det = 1.0f / det;
    const float tv[3] = {o[0] - p1[0], o[1] - p1[1], o[2] - p1[2]};
    const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv_det;
    if (u < 0.0f || u > 1.0f) return false;
    const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv_det;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv_det;
    if (!(t >= t_min && t <= t_max)) return false;
    *u_out = u; *v_out = v; *t_out = t; *det_out = det;
    return true;
}

struct AhList
{
    float t[RT_ALL_HITS_MAX];
    uint32_t prim[RT_ALL_HITS_MAX];
};

RTD_FN void ah_list_clear(AhList& l)
{
    for (int k = 0; k < RT_ALL_HITS_MAX; ++k) { l.t[k] = __builtin_inff(); l.prim[k] = RT_INVALID_ID; }
}

/* (t, prim) into its place; the largest of nine leaves.  A member's t is finite, so the +inf of an empty place is above every member. */
RTD_FN void ah_list_insert(AhList& l, float t, uint32_t prim)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = RT_ALL_HITS_MAX - 1; k >= 0; --k)
    {
        const bool before = t < l.t[k] || (t == l.t[k] && prim < l.prim[k]);                       /* the new pair sorts before place k */
        const bool before_prev = k > 0 && (t < l.t[k - 1] || (t == l.t[k - 1] && prim < l.prim[k - 1]));
        const float nt = before ? (before_prev ? l.t[k - (k > 0 ? 1 : 0)] : t) : l.t[k];
        const uint32_t np = before ? (before_prev ? l.prim[k - (k > 0 ? 1 : 0)] : prim) : l.prim[k];
        l.t[k] = nt; l.prim[k] = np;
    }
}

/* a ray's record; exits = bit 8 + j set when stored hit j is met from behind (det < 0) */
RTD_FN rt_ray_hits ah_record(uint32_t count, uint32_t entering, uint32_t max_hits, uint32_t exits, bool walked)
{
    rt_ray_hits r;
    r.count = count; r.entering = entering;
    r.stored = count < max_hits ? count : max_hits;
    r.flags = (walked ? RT_RAY_HITS_WALKED : 0u) | (exits << RT_RAY_HITS_EXIT_SHIFT);
    return r;
}

#endif /* RT_ALL_HITS_H */
