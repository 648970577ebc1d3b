// separation_kernels.h -- the kernels of a separation query (rt_scene_separation / rt_scene_separation_buffer / rt_scene_separation_self /
// rt_scene_separation_self_buffer / rt_debug_separation / rt_debug_separation_self): for each CALLER-supplied triangle (a probe), or
// each scene triangle of a range (the self form), the nearest triangle of the uploaded scene, how far it is and the two closest points.  The rule -- the
// crossing verdict, the fifteen candidates, the bound, the self form's skip -- is separation.h's.
//
//   k_separation<WIDE, SELF>   one lane per probe, 64-thread blocks: rt_probe in (48 bytes; SELF: scene triangle first + i, read from the shading records,
//                              nothing is uploaded), rt_separation out (48 bytes, three dwordx4)
//   k_separation_brute         one lane per probe over ALL triangles of an rt_triangle array (rt_debug_separation's and rt_debug_separation_self's device form)
//
// The walk is walk_kernels.h's volume walk (persistent strided chunks of 64 probes, walk::Stack in the ray queries' spill area, the family's status word) on
// walk::volume_step for the fetch and the leaf chain, with walk::probe_box_step at a box record: k_nearest's ordering with sep_box_d2 as the key -- the
// nearest passing box is visited next, the others wait with their bound, farthest deepest, and a pop re-tests !(entry > best).  sep_box_d2 <= d2 holds in
// binary32 itself for every box that holds a triangle's corners (separation.h), so no order, fold or quantisation of a box changes the result.  The lane's
// state is the probe's 9 corner floats, 6 box floats and 4 plane floats (cross_test's), `best` and `best_prim`: registers, no LDS beside the stack's.  At a
// leaf the pair function is skipped when the two triangles' own boxes are already farther apart than `best` (sep_maybe_nearer).  A probe that is not
// searched is never walked.  After the walk the record is made again by sep_pair on the kept triangle's corners: the same function on the same operands.
#pragma once
#include "walk_kernels.h"
#include "separation.h"

namespace separation
{
// an rt_separation as three 16-byte pieces
RT_DEV void store_record(float4* o, const rt_separation& r)
{
    q_store(o, make_float4(r.on_probe[0], r.on_probe[1], r.on_probe[2], r.distance));
    q_store(o + 1, make_float4(r.on_scene[0], r.on_scene[1], r.on_scene[2], __uint_as_float(r.primitive_id)));
    q_store(o + 2, make_float4(__uint_as_float(r.flags), __uint_as_float(r.feature), __uint_as_float(r.pad[0]), __uint_as_float(r.pad[1])));
}

// SELF: probe i is scene triangle first + i and `ids` (nullptr: RT_SEPARATION_OTHER_OBJECTS is off) is the objects' table.
template <bool WIDE, bool SELF>
__global__ __launch_bounds__(64) void k_separation(DScene sc, const float4* __restrict__ probes, const uint32_t* __restrict__ ids, uint32_t first, uint32_t n,
    float max_distance, float4* __restrict__ out, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, best_prim = RT_INVALID_ID, self_prim = RT_INVALID_ID, self_object = RT_INVALID_ID;
        float best = 0.0f;
        stack.sp = 0;
        CrossProbe q;
        {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
            if (i < n)
            {
                if (SELF)
                {
                    self_prim = first + i;
                    const float4* tp = sc.tris_sh + (size_t)self_prim * 8;
                    a = tp[0]; b = tp[1]; c = tp[2];
                    if (ids) self_object = ids[self_prim];
                }
                else { a = probes[(size_t)i * 3u]; b = probes[(size_t)i * 3u + 1u]; c = probes[(size_t)i * 3u + 2u]; }
            }
            const float q1[3] = {a.x, a.y, a.z}, q2[3] = {b.x, b.y, b.z}, q3[3] = {c.x, c.y, c.z};
            cross_probe_make(q, q1, q2, q3);
        }
        const bool searched = i < n && sep_searched(q, max_distance);
        if (searched)
        {
            best = max_distance * max_distance;
            ref = WIDE ? sc.w_entry_ref : sc.entry_ref;
        }

        auto leaf = [&](uint32_t prim, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
        {
            bool skipped = false;
            if (SELF)
            {
                skipped = prim == self_prim || cross_shares_corner(q, p1, p2, p3);
                if (!skipped && ids) skipped = ids[prim] == self_object;
            }
            if (!skipped && sep_maybe_nearer(q, p1, p2, p3, best))
            {
                const float d2 = sep_pair(q, p1, p2, p3).d2;
                if (nearest_accepts(d2, prim, best, best_prim)) { best = d2; best_prim = prim; }
            }
        };
        auto key = [&](const float (&lo)[3], const float (&hi)[3]) { return sep_box_d2(q.lo, q.hi, lo, hi); };
        auto box = [&](float4 q0, float4 q1, float4 q2, float4 q3) { walk::probe_box_step<WIDE>(q0, q1, q2, q3, key, best, ref, stack); };
        auto keep = [&](float entry) { return !(entry > best); };
        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF) walk::volume_step<WIDE>(sc, ref, stack, leaf, box, keep);

        if (i < n)
        {
            rt_separation o = sep_none(searched);
            if (best_prim != RT_INVALID_ID)
            {
                const float4* tp = sc.tris_sh + (size_t)best_prim * 8;
                const float4 a = tp[0], b = tp[1], c = tp[2];
                const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
                o = sep_record(q, p1, p2, p3, best_prim);
            }
            store_record(out + (size_t)i * 3u, o);
        }
    }
    stack.report(status);
}

// separation.h over every triangle, no tree.  probes == nullptr: the self form, probe i is tris[first + i] (ids: as above).
__global__ __launch_bounds__(64) void k_separation_brute(const rt_triangle* __restrict__ tris, uint32_t n_tris, const float4* __restrict__ probes,
    const uint32_t* __restrict__ ids, uint32_t first, uint32_t n, float max_distance, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const bool self = probes == nullptr;
    const uint32_t self_prim = self ? first + i : RT_INVALID_ID;
    float p1[3], p2[3], p3[3];
    CrossProbe q;
    if (self)
    {
        walk::triangle_corners(tris[self_prim], p1, p2, p3);
        cross_probe_make(q, p1, p2, p3);
    }
    else
    {
        const float4 a = probes[(size_t)i * 3u], b = probes[(size_t)i * 3u + 1u], c = probes[(size_t)i * 3u + 2u];
        const float q1[3] = {a.x, a.y, a.z}, q2[3] = {b.x, b.y, b.z}, q3[3] = {c.x, c.y, c.z};
        cross_probe_make(q, q1, q2, q3);
    }
    const uint32_t self_object = self && ids ? ids[self_prim] : RT_INVALID_ID;
    const bool searched = sep_searched(q, max_distance);
    rt_separation o = sep_none(searched);
    if (searched)
    {
        float best = max_distance * max_distance;
        uint32_t best_prim = RT_INVALID_ID;
        for (uint32_t t = 0; t < n_tris; ++t)
        {
            walk::triangle_corners(tris[t], p1, p2, p3);
            if (self && (t == self_prim || cross_shares_corner(q, p1, p2, p3) || (ids && ids[t] == self_object))) continue;
            if (!sep_maybe_nearer(q, p1, p2, p3, best)) continue;
            const float d2 = sep_pair(q, p1, p2, p3).d2;
            if (nearest_accepts(d2, t, best, best_prim)) { best = d2; best_prim = t; }
        }
        if (best_prim != RT_INVALID_ID)
        {
            walk::triangle_corners(tris[best_prim], p1, p2, p3);
            o = sep_record(q, p1, p2, p3, best_prim);
        }
    }
    store_record(out + (size_t)i * 3u, o);
}
} // namespace separation
