/* cross.h -- every scene triangle a caller's triangle (a PROBE) crosses, and where (rt_scene_cross / rt_scene_cross_buffer / rt_scene_cross_self /
 * rt_scene_cross_self_buffer / rt_debug_cross / rt_debug_cross_walk / rt_debug_cross_self), stated once for the kernels (cross.hip:
 * k_cross, k_cross_self, k_cross_brute) and the host (rt_debug_cross(NULL, ...), rt_debug_cross_walk, rt_debug_cross_self(NULL, ...)).  binary32 throughout,
 * -ffp-contract=off, correctly rounded divide on both sides, so the device and the host agree bit for bit.
 *
 * fl(x) is x rounded once.  dot3(a, b) = (a0 b0 + a1 b1) + a2 b2 (np_dot3's order) and cross3(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), every
 * product and every sum rounded once.  cross_min(x, y) = y < x ? y : x and cross_max(x, y) = x < y ? y : x.
 *
 * A PROBE Q = (q1, q2, q3) is SEARCHED when its nine coordinates are finite.  Of a searched probe:
 *   box     lo_Q[a] = cross_min(cross_min(q1[a], q2[a]), q3[a]), hi_Q[a] likewise with cross_max: exact
 *   plane   n = cross3(fl(q2 - q1), fl(q3 - q1)), d = -dot3(n, q1); the plane is USED when n0, n1, n2 and d are all finite
 *
 * A scene triangle T = (p1, p2, p3) enters on its shading record's three corners (k_nearest's and k_region's operands).  CROSS(Q, T) holds when all three hold:
 *   1. BOXES   lo_Q[a] <= hi_T[a] && lo_T[a] <= hi_Q[a] on every axis a, T's box made as Q's is.
 *   2. PLANE   (only when the plane is used) T is not rejected by region_classify(2, {(n, d), (-n, -d)}, p1, p2, p3), region.h's classification on the two
 *              half-spaces of the probe's own plane.  Negation commutes with rounding, so the second plane's s is exactly -s of the first, and rejected
 *              means: s(p1), s(p2), s(p3) all > 0, or all < 0, s = region_plane((n, d), .).  cross_plane_rejects is written that way.  A corner ON the
 *              plane (s == 0) or a NaN s is on neither side.
 *   3. EDGES   at least one of six segment-triangle tests accepts.  Bits 0..2: Q's edges q1->q2, q2->q3, q3->q1 against the triangle
 *              (p1, fl(p2 - p1), fl(p3 - p1)); bits 3..5: T's edges p1->p2, p2->p3, p3->p1 against the triangle (q1, fl(q2 - q1), fl(q3 - q1)).
 * A segment a->b against a triangle (o, e1, e2) is all_hits.h's ah_triangle -- two-sided Moeller-Trumbore -- with origin a, dir = fl(b - a), the range
 * 0 <= t <= 1 and ONE rule changed: the determinant rejects only when !(det > 0 || det < 0), zero or NaN.  (ah_triangle's absolute 1e-8 is a threshold for
 * unit directions; here det scales with the cube of the edge length and would reject small triangles.)  In ah_triangle's operand order:
 *   pv = cross3(dir, e2); det = dot3(e1, pv); inv = 1 / det; tv = fl(a - o)
 *   u = dot3(tv, pv) * inv, rejected when u < 0 || u > 1;   qv = cross3(tv, e1)
 *   v = dot3(dir, qv) * inv, rejected when v < 0 || fl(u + v) > 1;   t = dot3(e2, qv) * inv, accepted when t >= 0 && t <= 1 (a NaN t is rejected)
 * COPLANAR pairs do not cross: a segment in the triangle's plane has det == 0 in exact arithmetic, and all six segments of a coplanar pair lie in the other's
 * plane.  (Rounding may leave a tiny nonzero det; the verdict of such a pair is still the same on the device and the host, and in every tree.)
 *
 * CONTACT POINTS of a member: for each accepted test x = a + t * dir per component (the product rounded, then the sum).  c0 is the point of the lowest set
 * bit, c1 that of the second lowest; one bit: c1 = c0.  In exact arithmetic a generic crossing sets exactly two bits and c0 c1 is the intersection
 * segment; rounding may set one bit (an end point that grazes an edge is accepted on one side only) or three (a segment through a corner or an edge).
 *
 * WHY A WALK IS EXACT.  A node's box is skipped when (i) its closed box misses the probe's box, !(lo_Q[a] <= hi_B[a] && lo_B[a] <= hi_Q[a]) on some axis,
 * or (ii) the plane is used and one of the two planes rejects it (region_plane_rejects_box).  Let T's corners lie in B: lo_B[a] <= p[a] <= hi_B[a].  (i)
 * T's box lies in B's, lo_B <= lo_T and hi_T <= hi_B, so lo_Q > hi_B implies lo_Q > hi_T and lo_B > hi_Q implies lo_T > hi_Q: plain comparisons of
 * binary32 values, no arithmetic.  (ii) is region.h's argument unchanged -- the rounded plane evaluation is monotone in each coordinate, overflow included,
 * for FINITE coefficients, which is what "the plane is used" guarantees -- so a box a plane rejects holds only triangles with all three corners > 0 on that
 * plane: step 2 rejects them.  The decoded 4-wide boxes hold their triangles' corners (wide_frame), as the child-pair boxes do.  Hence the member set, the
 * count and the lowest ids are a statement about triangles and this header alone, whichever records, fold or order is walked.
 *
 * THE LIST keeps ids only, the crossing triangles with the LOWEST primitive ids, ascending: it is region.h's RgList, reused (RT_CROSS_LIST_MAX ==
 * RT_REGION_LIST_MAX).  A listed member's flags and points are made again after the walk by cross_pair on the kept triangle's corners: the same function on
 * the same operands, so the same bits.
 *
 * THE SELF FORM.  Probe i is triangle first + i of the same array.  A pair (Q, T) is SKIPPED -- no member, not counted -- when both are the same index, or
 * when some corner of Q equals some corner of T on all three coordinates by == (cross_shares_corner): such neighbours share a vertex, so they always touch.
 * RT_CROSS_OTHER_OBJECTS also skips a pair of one object.  The skip looks at the two triangles (and their objects) alone. */
#ifndef RT_CROSS_H
#define RT_CROSS_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"
#include "region.h"

#if defined(__cplusplus)
static_assert(RT_CROSS_LIST_MAX == RT_REGION_LIST_MAX, "the list is region.h's RgList");
#endif

RTD_FN float cross_min(float x, float y) { return y < x ? y : x; }
RTD_FN float cross_max(float x, float y) { return x < y ? y : x; }

struct CrossProbe
{
    float q1[3], q2[3], q3[3];
    float lo[3], hi[3];
    float pl[4];                /* (n, d) */
    bool searched, plane;       /* nine finite coordinates; n and d finite: step 2 and the planes' box test run */
};

RG_FN void cross_box_of(const float p1[3], const float p2[3], const float p3[3], float lo[3], float hi[3])
{
    for (int a = 0; a < 3; ++a)
    {
        lo[a] = cross_min(cross_min(p1[a], p2[a]), p3[a]);
        hi[a] = cross_max(cross_max(p1[a], p2[a]), p3[a]);
    }
}

RG_FN void cross_probe_make(CrossProbe& q, const float q1[3], const float q2[3], const float q3[3])
{
    bool finite = true;
    for (int a = 0; a < 3; ++a)
    {
        q.q1[a] = q1[a]; q.q2[a] = q2[a]; q.q3[a] = q3[a];
        finite = finite && __builtin_isfinite(q1[a]) && __builtin_isfinite(q2[a]) && __builtin_isfinite(q3[a]);
    }
    q.searched = finite;
    cross_box_of(q1, q2, q3, q.lo, q.hi);
    const float e1[3] = {q2[0] - q1[0], q2[1] - q1[1], q2[2] - q1[2]}, e2[3] = {q3[0] - q1[0], q3[1] - q1[1], q3[2] - q1[2]};
    region_cross3(e1, e2, q.pl);
    q.pl[3] = -np_dot3(q.pl, q1);
    q.plane = __builtin_isfinite(q.pl[0]) && __builtin_isfinite(q.pl[1]) && __builtin_isfinite(q.pl[2]) && __builtin_isfinite(q.pl[3]);
}

/* step 1, and the walk's test (i): two closed boxes overlap on every axis */
RG_FN bool cross_boxes_overlap(const float lo_q[3], const float hi_q[3], const float lo_t[3], const float hi_t[3])
{
    return lo_q[0] <= hi_t[0] && lo_t[0] <= hi_q[0] && lo_q[1] <= hi_t[1] && lo_t[1] <= hi_q[1] && lo_q[2] <= hi_t[2] && lo_t[2] <= hi_q[2];
}

/* step 2: region_classify(2, {(n, d), (-n, -d)}, ...) == RT_REGION_REJECTED, the second plane's s being exactly the first's negated */
RG_FN bool cross_plane_rejects(const float pl[4], const float p1[3], const float p2[3], const float p3[3])
{
    const float s1 = region_plane(pl, p1), s2 = region_plane(pl, p2), s3 = region_plane(pl, p3);
    return (s1 > 0.0f && s2 > 0.0f && s3 > 0.0f) || (s1 < 0.0f && s2 < 0.0f && s3 < 0.0f);
}

/* the walk's test (ii): one of the two planes rejects the box */
RG_FN bool cross_planes_reject_box(const float pl[4], const float lo[3], const float hi[3])
{
    const float neg[4] = {-pl[0], -pl[1], -pl[2], -pl[3]};
    return region_plane_rejects_box(pl, lo, hi) || region_plane_rejects_box(neg, lo, hi);
}

/* the segment a -> b against the triangle (o, e1, e2); dir = fl(b - a) and t are handed back when it accepts */
RG_FN bool cross_segment(const float a[3], const float b[3], const float o[3], const float e1[3], const float e2[3], float dir[3], float* t_out)
{
    const float d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (!(det > 0.0f || det < 0.0f)) return false;
    const float inv_det = 1.0f / det;
    const float tv[3] = {a[0] - o[0], a[1] - o[1], a[2] - o[2]};
    const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv_det;
    if (u < 0.0f || u > 1.0f) return false;
    const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv_det;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv_det;
    if (!(t >= 0.0f && t <= 1.0f)) return false;
    dir[0] = d[0]; dir[1] = d[1]; dir[2] = d[2];
    *t_out = t;
    return true;
}

/* steps 1 and 2 */
RG_FN bool cross_culled(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3])
{
    float lo[3], hi[3];
    cross_box_of(p1, p2, p3, lo, hi);
    if (!cross_boxes_overlap(q.lo, q.hi, lo, hi)) return true;
    return q.plane && cross_plane_rejects(q.pl, p1, p2, p3);
}

/* CROSS(Q, T) as a member's flags (0: no member) with its contact points; the six tests in bit order */
RG_FN uint32_t cross_pair(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3], float c0[3], float c1[3])
{
    c0[0] = c0[1] = c0[2] = 0.0f; c1[0] = c1[1] = c1[2] = 0.0f;
    if (cross_culled(q, p1, p2, p3)) return 0u;
    const float te1[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]}, te2[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
    const float qe1[3] = {q.q2[0] - q.q1[0], q.q2[1] - q.q1[1], q.q2[2] - q.q1[2]}, qe2[3] = {q.q3[0] - q.q1[0], q.q3[1] - q.q1[1], q.q3[2] - q.q1[2]};
    const float* const from[6] = {q.q1, q.q2, q.q3, p1, p2, p3};
    const float* const to[6] = {q.q2, q.q3, q.q1, p2, p3, p1};
    uint32_t flags = 0u, set = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 6; ++k)
    {
        float dir[3], t;
        const bool hit = k < 3 ? cross_segment(from[k], to[k], p1, te1, te2, dir, &t) : cross_segment(from[k], to[k], q.q1, qe1, qe2, dir, &t);
        if (!hit) continue;
        const float x[3] = {from[k][0] + t * dir[0], from[k][1] + t * dir[1], from[k][2] + t * dir[2]};
        if (set == 0u) { c0[0] = x[0]; c0[1] = x[1]; c0[2] = x[2]; }
        if (set <= 1u) { c1[0] = x[0]; c1[1] = x[1]; c1[2] = x[2]; }
        flags |= 1u << k;
        ++set;
    }
    return flags;
}

/* the verdict alone, as a walk needs it: cross_pair(...) != 0, the six tests tried in the same order until one accepts */
RG_FN bool cross_test(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3])
{
    if (cross_culled(q, p1, p2, p3)) return false;
    const float te1[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]}, te2[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
    const float qe1[3] = {q.q2[0] - q.q1[0], q.q2[1] - q.q1[1], q.q2[2] - q.q1[2]}, qe2[3] = {q.q3[0] - q.q1[0], q.q3[1] - q.q1[1], q.q3[2] - q.q1[2]};
    float dir[3], t;
    return cross_segment(q.q1, q.q2, p1, te1, te2, dir, &t) || cross_segment(q.q2, q.q3, p1, te1, te2, dir, &t) || cross_segment(q.q3, q.q1, p1, te1, te2, dir, &t) ||
           cross_segment(p1, p2, q.q1, qe1, qe2, dir, &t) || cross_segment(p2, p3, q.q1, qe1, qe2, dir, &t) || cross_segment(p3, p1, q.q1, qe1, qe2, dir, &t);
}

/* the self form's skip: some corner of one equals some corner of the other on all three coordinates */
RG_FN bool cross_same_point(const float a[3], const float b[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
RG_FN bool cross_shares_corner(const CrossProbe& q, const float p1[3], const float p2[3], const float p3[3])
{
    return cross_same_point(q.q1, p1) || cross_same_point(q.q1, p2) || cross_same_point(q.q1, p3) ||
           cross_same_point(q.q2, p1) || cross_same_point(q.q2, p2) || cross_same_point(q.q2, p3) ||
           cross_same_point(q.q3, p1) || cross_same_point(q.q3, p2) || cross_same_point(q.q3, p3);
}

/* a probe's record; lowest: the lowest crossing id met (RT_INVALID_ID: none).  An RT_CROSS_ANY answer lists nothing and names no triangle. */
RTD_FN rt_probe_hits cross_record(uint32_t count, uint32_t lowest, uint32_t max_list, bool searched, bool any)
{
    rt_probe_hits r;
    r.count = count;
    r.stored = any ? 0u : (count < max_list ? count : max_list);
    r.first_primitive = any || count == 0u ? RT_INVALID_ID : lowest;
    r.flags = searched ? RT_PROBE_HITS_SEARCHED | (any ? RT_PROBE_HITS_ANY : 0u) : 0u;
    return r;
}

/* what every entry refuses of max_list and options (self: a self form, which alone takes RT_CROSS_OTHER_OBJECTS); NULL: fine */
static inline const char* cross_shape_refused(uint32_t max_list, uint32_t options, bool self, bool members)
{
    if (max_list > RT_CROSS_LIST_MAX) return "max_list is above RT_CROSS_LIST_MAX";
    if (options & ~(RT_CROSS_ANY | RT_CROSS_OTHER_OBJECTS)) return "unknown option bits";
    if ((options & RT_CROSS_OTHER_OBJECTS) && !self) return "RT_CROSS_OTHER_OBJECTS is the self forms' (rt_scene_cross_self, rt_debug_cross_self)";
    if (max_list == 0u && members) return "members given with max_list == 0: pass NULL";
    if ((options & RT_CROSS_ANY) && members) return "RT_CROSS_ANY lists no members (which one is met first depends on the tree): pass NULL";
    return nullptr;
}

#endif /* RT_CROSS_H */
