/* within.h -- every triangle within a radius of a caller-supplied point (rt_scene_within / rt_scene_within_buffer / rt_debug_within / rt_debug_within_walk;
 * DESIGN.md section 7l), stated once for the kernels (within.hip: k_within, k_within_brute) and the host (rt_debug_within(NULL, ...), rt_debug_within_walk).
 * The arithmetic is nearest.h's, unchanged: d2 of a triangle is nearest_point_triangle's, the bound that prunes is nearest_box_d2, a searched point is
 * nearest_searched's.  binary32 throughout, -ffp-contract=off, so the device and the host agree bit for bit.
 *
 * THE MEMBER SET of a searched point: every triangle with d2 <= r2, r2 = max_distance * max_distance rounded once (+inf stays +inf).  A NaN d2 is no member:
 * the comparison is false.  Members are ordered by ascending (d2, primitive_id), d2 compared as binary32.
 *
 * WnList keeps the first max_near members (at most RT_WITHIN_MAX) in that order.  Insertion is all_hits.h's compare-and-shift chain over static indices
 * (registers on the device, never an indexed per-lane array), keyed (d2, prim).  An empty place is (+inf, RT_INVALID_ID): a member's d2 may itself be +inf
 * (r2 = +inf, squares that overflow), and then its primitive_id, which is below RT_INVALID_ID, still sorts it before every empty place.
 *
 * The bound of a walk.  Counting mode: r2, never lowered.  K-nearest mode (RT_WITHIN_K_NEAREST, 1 <= k <= RT_WITHIN_MAX): r2 until the list's k-th place
 * is taken, that place's d2 from then on.  A subtree is skipped exactly when nearest_box_d2 > bound (strict: a tie with the last entry is visited, and the
 * lower primitive_id then takes the place, as in nearest_accepts).
 *
 * Why a walk gives the brute force's set: nearest_box_d2 <= d2 holds in binary32 for every box that holds a triangle's corners (nearest.h).  Counting: a
 * skipped subtree has nearest_box_d2 > r2, so every triangle in it has d2 > r2 and is no member.  K-nearest: the bound only falls, and at every moment it is
 * >= the final k-th smallest d2; a skipped subtree's triangles have d2 > bound at that moment >= the final last entry's d2, so none of them is among the
 * first k.  Either way the set is a statement about triangles alone, whichever records, fold or order is walked. */
#ifndef RT_WITHIN_H
#define RT_WITHIN_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"
#include "nearest.h"

/* the list's functions take it by reference: on the device they must be inlined, or the list would have an address and live in scratch */
#if defined(__HIPCC__)
#define WN_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define WN_FN static inline
#endif

struct WnList
{
    float d2[RT_WITHIN_MAX];
    uint32_t prim[RT_WITHIN_MAX];
};

/* where the members of a list that keeps max(max_near, 1) of them start: they are kept RIGHT-ALIGNED, so that the last one wanted is always place
 * RT_WITHIN_MAX - 1 -- a static index, where a place chosen by max_near would be an indexed per-lane array */
RTD_FN uint32_t wn_list_first(uint32_t max_near) { return RT_WITHIN_MAX - (max_near > 0u ? max_near : 1u); }

/* the places before wn_list_first are (-inf, 0): no member sorts before them (a d2 is a sum of squares), so the chain below never moves them */
WN_FN void wn_list_clear(WnList& l, uint32_t max_near)
{
    const uint32_t first = wn_list_first(max_near);
    for (int k = 0; k < RT_WITHIN_MAX; ++k)
    {
        const bool used = (uint32_t)k >= first;
        l.d2[k] = used ? __builtin_inff() : -__builtin_inff();
        l.prim[k] = used ? RT_INVALID_ID : 0u;
    }
}

/* (d2, prim) into its place; the largest of the kept and the new leaves */
WN_FN void wn_list_insert(WnList& l, float d2, uint32_t prim)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = RT_WITHIN_MAX - 1; k >= 0; --k)
    {
        const bool before = d2 < l.d2[k] || (d2 == l.d2[k] && prim < l.prim[k]);                    /* the new pair sorts before place k */
        const bool before_prev = k > 0 && (d2 < l.d2[k - 1] || (d2 == l.d2[k - 1] && prim < l.prim[k - 1]));
        const float nd = before ? (before_prev ? l.d2[k - (k > 0 ? 1 : 0)] : d2) : l.d2[k];
        const uint32_t np = before ? (before_prev ? l.prim[k - (k > 0 ? 1 : 0)] : prim) : l.prim[k];
        l.d2[k] = nd; l.prim[k] = np;
    }
}

/* the membership rule: false for a NaN d2 */
RTD_FN bool within_member(float d2, float r2) { return d2 <= r2; }

/* A k-nearest walk's bound after an insertion: r2 until the last place is taken, its d2 from then on.  That d2 is <= r2, a member's. */
WN_FN float within_knn_bound(const WnList& l, float r2)
{
    return l.prim[RT_WITHIN_MAX - 1] != RT_INVALID_ID ? l.d2[RT_WITHIN_MAX - 1] : r2;
}

/* a point's record.  count: the members met (counting mode: all of them; k-nearest: at least the listed ones); first: the list's first place, or the running
 * nearest member where no list is kept */
RTD_FN rt_point_hits within_record(uint32_t count, uint32_t max_near, uint32_t options, uint32_t first, bool searched)
{
    rt_point_hits r;
    const uint32_t stored = count < max_near ? count : max_near;
    r.count = (options & RT_WITHIN_K_NEAREST) ? stored : count;
    r.stored = stored;
    r.nearest_primitive = first;
    r.flags = searched ? RT_POINT_HITS_SEARCHED | ((options & RT_WITHIN_K_NEAREST) ? RT_POINT_HITS_K_NEAREST : 0u) : 0u;
    return r;
}

#endif /* RT_WITHIN_H */
