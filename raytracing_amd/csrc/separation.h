/* separation.h -- the nearest scene triangle to a caller's triangle (a PROBE), how far it is and where the two closest points lie (rt_scene_separation /
 * rt_scene_separation_buffer / rt_scene_separation_self / rt_scene_separation_self_buffer / rt_debug_separation / rt_debug_separation_walk /
 * rt_debug_separation_self), stated once for the kernels (separation.hip: k_separation, k_separation_brute) and the host
 * (rt_debug_separation(NULL, ...), rt_debug_separation_walk, rt_debug_separation_self(NULL, ...)).  binary32 throughout, -ffp-contract=off, correctly
 * rounded divide and square root on both sides, so the device and the host agree bit for bit.
 *
 * dot3, fl, cross_min and cross_max are cross.h's; nearest_point_triangle, its clamp and its select forms are nearest.h's.
 *
 * A PROBE Q = (q1, q2, q3) is SEARCHED when its nine coordinates are finite and max_distance >= 0 (+inf is allowed, a NaN fails the comparison).  A scene
 * triangle T = (p1, p2, p3) enters on its shading record's three corners (k_nearest's and k_cross's operands).
 *
 * SEP(Q, T), a squared distance d2, a point on Q, a point on T and a feature:
 *   CROSSING   when cross_test(Q, T) (cross.h) holds: d2 = 0, both points are cross_pair's c0, feature = 15 (RT_SEPARATION_FEATURE_CROSSING).  Two triangles
 *              can pass through each other with every corner and edge far apart, so no candidate below could stand in for this step.
 *   otherwise  fifteen CANDIDATES, in this order:
 *     0..2     r = nearest_point_triangle(q_k, p1, p2, p3):  on Q: q_k, on T: r.q, d2 = r.d2
 *     3..5     r = nearest_point_triangle(p_k, q1, q2, q3):  on Q: r.q, on T: p_k, d2 = r.d2
 *     6..14    6 + 3 i + j: edge i of Q against edge j of T, edges numbered as cross.h numbers them (0: 1->2, 1: 2->3, 2: 3->1), by sep_segments below:
 *              on Q: c1, on T: c2, d = fl(c1 - c2), d2 = dot3(d, d)
 *   the pair's d2 is the least candidate d2; among equal ones the lowest candidate index; a NaN d2 never wins.  (No candidate without a NaN: d2 = NaN,
 *   feature 0, zero points; such a pair is never accepted.)
 *
 * sep_segments(a1, b1, a2, b2): Ericson, Real-Time Collision Detection, section 5.1.9, in that book's order, with d1 = fl(b1 - a1), d2 = fl(b2 - a2),
 * r = fl(a1 - a2), a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r); clamp01(x) = (x < 0 ? 0 : x), then (x > 1 ? 1 : x), so a NaN passes through:
 *   a == 0 && e == 0   s = t = 0
 *   a == 0             s = 0, t = clamp01(f / e)
 *   otherwise c = dot3(d1, r) and
 *     e == 0           t = 0, s = clamp01(-c / a)
 *     otherwise        b = dot3(d1, d2); denom = a e - b b; s = clamp01((b f - c e) / denom) when denom > 0 || denom < 0, else 0 (zero or NaN: parallel)
 *                      t = (b s + f) / e;   t < 0: t = 0, s = clamp01(-c / a);   else t > 1: t = 1, s = clamp01((b - c) / a)
 *   c1 = a1 + s d1, c2 = a2 + t d2 per component, the product rounded, then the sum; then each is clamped per component into ITS OWN SEGMENT's box,
 *   [np_min(a, b), np_max(a, b)], with nearest.h's select forms (x < lo ? lo : x, then x > hi ? hi : x): a NaN passes through.
 * "Degenerate" is a squared length == 0 and nothing else: an absolute epsilon made for unit vectors would call small triangles degenerate (cross.h says the
 * same of ah_triangle's determinant).  The routine is NOT symmetric in its two segments (s is found first), so SEP(Q, T) and SEP(T, Q) may differ in the last
 * bit; a layer that holds both directions of a pair (host.Render.clearances) takes the smaller.
 *
 * sep_box_d2(lo_Q, hi_Q, lo_B, hi_B), the bound that prunes: per axis g = lo_B - hi_Q; t = lo_Q - hi_B; g = t > g ? t : g; g = g > 0 ? g : 0 -- nearest_box_d2's
 * select forms -- then dot3(g, g).
 *
 * WHY A WALK IS EXACT.  Let B be a box that holds T's corners, lo_B[k] <= p[k] <= hi_B[k], and box Q, box T the triangles' own boxes (cross_box_of).
 *   (1) Both points of every candidate lie component-wise inside their own triangle's box: a corner does; nearest_point_triangle's q is clamped into its
 *       triangle's box (nearest.h); c1 and c2 are clamped into their segment's box, which lies inside the triangle's.  A NaN point makes d2 NaN: no claim, and
 *       such a candidate never wins.
 *   (2) So on an axis where g = fl(lo_B - hi_Q) > 0: x_T >= lo_T >= lo_B and x_Q <= hi_Q, hence x_T - x_Q >= lo_B - hi_Q exactly, and round-to-nearest
 *       subtraction is monotone: |fl(x_Q - x_T)| = fl(x_T - x_Q) >= g.  Likewise for t.  Every candidate forms its d as one rounded subtraction of its two
 *       points per component (r.d = p - q in nearest.h, fl(c1 - c2) here; the sign does not matter to the square).
 *   (3) Squaring and dot3's additions of non-negatives are monotone under round to nearest, overflow to +inf included, and every d2 is dot3(d, d) in the one
 *       operand order.  Hence  sep_box_d2(box Q, B) <= sep_box_d2(box Q, box T) <= d2  in binary32 itself.
 *   (4) A crossing pair has passed cross.h's step 1: lo_Q <= hi_T and lo_T <= hi_Q on every axis, so both differences are <= 0 before and after rounding and
 *       its bound is 0 = d2, for box T and for every B around it.
 * So a subtree is skipped exactly when sep_box_d2 > best (strict: a tie is visited), and the answer is a statement about triangles and this header alone,
 * whichever records, fold or order is walked.  INSIDE A LEAF the same bound on the two triangles' own boxes may skip the pair function (sep_maybe_nearer);
 * by (3) that changes no result, and the brute force takes the same shortcut.
 *
 * THE ANSWER of a probe: best = fl(max_distance * max_distance) (+inf stays +inf), best_prim = RT_INVALID_ID; triangle `prim` is accepted when
 * d2 < best || (d2 == best && prim < best_prim) (nearest_accepts).  The record is made after the walk by sep_pair on the kept triangle's corners: the same
 * function on the same operands, so the same bits; distance = sqrtf(d2).
 *
 * THE SELF FORM.  Probe i is triangle first + i of the same array.  A pair is SKIPPED when both are the same index or share a corner (cross_shares_corner);
 * RT_SEPARATION_OTHER_OBJECTS also skips a pair of one object.  The skip looks at the two triangles (and their objects) alone. */
#ifndef RT_SEPARATION_H
#define RT_SEPARATION_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"
#include "nearest.h"
#include "cross.h"

struct SepPair
{
    float d2;
    float on_probe[3], on_scene[3];
    uint32_t feature;           /* 0..14, or RT_SEPARATION_FEATURE_CROSSING */
};

RTD_FN float sep_clamp01(float x)
{
    x = x < 0.0f ? 0.0f : x;
    return x > 1.0f ? 1.0f : x;
}

RG_FN float sep_box_d2(const float lo_q[3], const float hi_q[3], const float lo_b[3], const float hi_b[3])
{
    float g[3];
    for (int k = 0; k < 3; ++k)
    {
        float x = lo_b[k] - hi_q[k];
        const float t = lo_q[k] - hi_b[k];
        x = t > x ? t : x;
        g[k] = x > 0.0f ? x : 0.0f;
    }
    return np_dot3(g, g);
}

/* the segments a1 -> b1 and a2 -> b2: their closest points c1, c2 (clamped into the segments' boxes) and dot3(c1 - c2, c1 - c2) */
RG_FN float sep_segments(const float a1[3], const float b1[3], const float a2[3], const float b2[3], float c1[3], float c2[3])
{
    const float d1[3] = {b1[0] - a1[0], b1[1] - a1[1], b1[2] - a1[2]}, d2[3] = {b2[0] - a2[0], b2[1] - a2[1], b2[2] - a2[2]};
    const float r[3] = {a1[0] - a2[0], a1[1] - a2[1], a1[2] - a2[2]};
    const float a = np_dot3(d1, d1), e = np_dot3(d2, d2), f = np_dot3(d2, r);
    float s, t;
    if (a == 0.0f && e == 0.0f) { s = 0.0f; t = 0.0f; }
    else if (a == 0.0f) { s = 0.0f; t = sep_clamp01(f / e); }
    else
    {
        const float c = np_dot3(d1, r);
        if (e == 0.0f) { t = 0.0f; s = sep_clamp01(-c / a); }
        else
        {
            const float b = np_dot3(d1, d2);
            const float denom = a * e - b * b;
            s = (denom > 0.0f || denom < 0.0f) ? sep_clamp01((b * f - c * e) / denom) : 0.0f;
            t = (b * s + f) / e;
            if (t < 0.0f) { t = 0.0f; s = sep_clamp01(-c / a); }
            else if (t > 1.0f) { t = 1.0f; s = sep_clamp01((b - c) / a); }
        }
    }
    float d[3];
    for (int k = 0; k < 3; ++k)
    {
        float x = a1[k] + s * d1[k], y = a2[k] + t * d2[k];
        const float lo1 = np_min(a1[k], b1[k]), hi1 = np_max(a1[k], b1[k]), lo2 = np_min(a2[k], b2[k]), hi2 = np_max(a2[k], b2[k]);
        x = x < lo1 ? lo1 : x; x = x > hi1 ? hi1 : x;
        y = y < lo2 ? lo2 : y; y = y > hi2 ? hi2 : y;
        c1[k] = x; c2[k] = y;
        d[k] = x - y;
    }
    return np_dot3(d, d);
}

#if defined(__clang__)
#define SEP_ROLLED _Pragma("nounroll")
#else
#define SEP_ROLLED
#endif

/* (a, b, c) becomes (b, c, a) */
RG_FN void sep_rotate(float a[3], float b[3], float c[3])
{
    for (int k = 0; k < 3; ++k) { const float t = a[k]; a[k] = b[k]; b[k] = c[k]; c[k] = t; }
}

/* candidate k's turn: it wins when its d2 is no NaN and nothing has won yet or it is smaller */
RG_FN void sep_offer(SepPair& best, bool& have, float d2, const float on_probe[3], const float on_scene[3], uint32_t feature)
{
    const bool wins = have ? d2 < best.d2 : d2 == d2;
    if (!wins) return;
    have = true;
    best.d2 = d2;
    best.feature = feature;
    for (int k = 0; k < 3; ++k) { best.on_probe[k] = on_probe[k]; best.on_scene[k] = on_scene[k]; }
}

/* SEP(Q, T) */
RG_FN SepPair sep_pair(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3])
{
    SepPair r;
    if (cross_test(q, p1, p2, p3))
    {
        float c0[3], c1[3];
        cross_pair(q, p1, p2, p3, c0, c1);
        r.d2 = 0.0f;
        r.feature = RT_SEPARATION_FEATURE_CROSSING;
        for (int k = 0; k < 3; ++k) { r.on_probe[k] = c0[k]; r.on_scene[k] = c0[k]; }
        return r;
    }
    r.d2 = __builtin_nanf("");
    r.feature = 0u;
    for (int k = 0; k < 3; ++k) { r.on_probe[k] = 0.0f; r.on_scene[k] = 0.0f; }
    bool have = false;
    /* Rotating copies of the corners: candidate k reads the first of them and every loop ends with the corners back in their order, so the three loops stay
     * loops on the device (nothing is indexed by a loop counter, nothing is unrolled: DESIGN.md section 7o has the registers of both forms).  The operands
     * and their order are those of the header comment whichever way the loops are compiled. */
    float qa[3] = {q.q1[0], q.q1[1], q.q1[2]}, qb[3] = {q.q2[0], q.q2[1], q.q2[2]}, qc[3] = {q.q3[0], q.q3[1], q.q3[2]};
    float ta[3] = {p1[0], p1[1], p1[2]}, tb[3] = {p2[0], p2[1], p2[2]}, tc[3] = {p3[0], p3[1], p3[2]};
    SEP_ROLLED
    for (uint32_t k = 0; k < 3u; ++k)
    {
        const NpTriangle c = nearest_point_triangle(qa, p1, p2, p3);
        sep_offer(r, have, c.d2, qa, c.q, k);
        sep_rotate(qa, qb, qc);
    }
    SEP_ROLLED
    for (uint32_t k = 0; k < 3u; ++k)
    {
        const NpTriangle c = nearest_point_triangle(ta, q.q1, q.q2, q.q3);
        sep_offer(r, have, c.d2, c.q, ta, 3u + k);
        sep_rotate(ta, tb, tc);
    }
    SEP_ROLLED
    for (uint32_t i = 0; i < 3u; ++i)
    {
        SEP_ROLLED
        for (uint32_t j = 0; j < 3u; ++j)
        {
            float c1[3], c2[3];
            const float d2 = sep_segments(qa, qb, ta, tb, c1, c2);
            sep_offer(r, have, d2, c1, c2, 6u + 3u * i + j);
            sep_rotate(ta, tb, tc);
        }
        sep_rotate(qa, qb, qc);
    }
    return r;
}

/* inside a leaf, and in the brute force alike: false only when the two triangles' own boxes are already farther apart than `best` (strict; a NaN bound
 * is not), so that SEP(Q, T) could not be accepted */
RG_FN bool sep_maybe_nearer(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3], float best)
{
    float lo[3], hi[3];
    cross_box_of(p1, p2, p3, lo, hi);
    return !(sep_box_d2(q.lo, q.hi, lo, hi) > best);
}

/* decided before any walk */
RTD_FN bool sep_searched(const CrossProbe& q, float max_distance) { return q.searched && max_distance >= 0.0f; }

RTD_FN rt_separation sep_none(bool searched)
{
    rt_separation o;
    for (int k = 0; k < 3; ++k) { o.on_probe[k] = 0.0f; o.on_scene[k] = 0.0f; }
    o.distance = 0.0f;
    o.primitive_id = RT_INVALID_ID;
    o.flags = searched ? RT_SEPARATION_SEARCHED : 0u;
    o.feature = 0u;
    o.pad[0] = o.pad[1] = 0u;
    return o;
}

/* the record of the accepted triangle */
RG_FN rt_separation sep_record(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3], uint32_t prim)
{
    const SepPair s = sep_pair(q, p1, p2, p3);
    rt_separation o;
    for (int k = 0; k < 3; ++k) { o.on_probe[k] = s.on_probe[k]; o.on_scene[k] = s.on_scene[k]; }
    o.distance = __builtin_sqrtf(s.d2);
    o.primitive_id = prim;
    o.flags = RT_SEPARATION_SEARCHED | RT_SEPARATION_FOUND | (s.feature == RT_SEPARATION_FEATURE_CROSSING ? RT_SEPARATION_CROSSING : 0u);
    o.feature = s.feature;
    o.pad[0] = o.pad[1] = 0u;
    return o;
}

/* what every entry refuses of max_distance-independent shape (self: a self form, which alone takes RT_SEPARATION_OTHER_OBJECTS); NULL: fine */
static inline const char* sep_shape_refused(uint32_t options, bool self)
{
    if (options & ~RT_SEPARATION_OTHER_OBJECTS) return "unknown option bits";
    if ((options & RT_SEPARATION_OTHER_OBJECTS) && !self) return "RT_SEPARATION_OTHER_OBJECTS is the self forms' (rt_scene_separation_self, rt_debug_separation_self)";
    return nullptr;
}

#endif /* RT_SEPARATION_H */
