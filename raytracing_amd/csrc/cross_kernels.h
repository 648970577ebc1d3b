// cross_kernels.h -- the kernels of a crossing query (rt_scene_cross / rt_scene_cross_buffer / rt_scene_cross_self / rt_scene_cross_self_buffer /
// rt_debug_cross / rt_debug_cross_self): for each CALLER-supplied triangle (a probe), or each scene triangle of a range (the self
// form), every triangle of the uploaded scene it crosses.  The rule -- the boxes, the probe's plane, the six segment tests, the contact points, the self
// form's skip -- is cross.h's.
//
//   k_cross<WIDE, LIST, ANY>   one lane per probe, 64-thread blocks: rt_probe in (48 bytes), rt_probe_hits out (16 bytes) and max_list rt_cross_member (LIST)
//   k_cross_self<WIDE, LIST>   the same walk where probe i is scene triangle first + i, read from the shading records: nothing is uploaded.  A pair of one
//                              index, of a shared corner or (ids given) of one object is skipped; RT_CROSS_ANY is a run-time flag here
//   k_cross_brute              one lane per probe over ALL triangles of an rt_triangle array (rt_debug_cross's and rt_debug_cross_self's device form)
//
// The walk is walk_kernels.h's volume walk (persistent strided chunks of 64 probes, walk::Stack in the ray queries' spill area, the family's status word) on
// walk::volume_step for the fetch and the leaf chain -- it costs no scratch and no register here (the resource table of DESIGN.md section 7n was read with
// it) -- with walk::cross_box_step at a box record: a counting walk, every passing child but one is pushed, no key, no sort, a pop always accepts.  ANY
// leaves the loop at the first member.  The lane's state is its 9 corner floats, 6 box floats and 4 plane floats: registers, no LDS beside the stack's.
// A probe that is not searched is never walked.
//
// LIST = false keeps `count` and the lowest id.  LIST = true also keeps an RgList (region.h): 8 registers of ids, right-aligned; after the walk a listed
// member's flags and contact points are made again by cross_pair on the kept triangle's corners: the same function on the same operands, so the same bits.
#pragma once
#include "walk_kernels.h"
#include "cross.h"

namespace cross
{
RT_DEV void store_record(float4* o, const rt_probe_hits& r)
{
    q_store(o, make_float4(__uint_as_float(r.count), __uint_as_float(r.stored), __uint_as_float(r.first_primitive), __uint_as_float(r.flags)));
}

// an rt_cross_member as two 16-byte pieces
RT_DEV void store_member(float4* o, uint32_t prim, uint32_t flags, const float (&c0)[3], const float (&c1)[3])
{
    q_store(o, make_float4(__uint_as_float(prim), __uint_as_float(flags), c0[0], c0[1]));
    q_store(o + 1, make_float4(c0[2], c1[0], c1[1], c1[2]));
}

// member j of a probe from the corners of triangle `prim`; j >= stored: an invalid entry
RT_DEV void write_member(float4* o, const CrossProbe& q, bool valid, uint32_t prim, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
{
    float c0[3] = {0.0f, 0.0f, 0.0f}, c1[3] = {0.0f, 0.0f, 0.0f};
    uint32_t flags = 0u;
    if (valid) flags = cross_pair(q, p1, p2, p3, c0, c1);
    store_member(o, valid ? prim : RT_INVALID_ID, flags, c0, c1);
}

// The walk of both kernels.  SELF: probe i is scene triangle first + i and `ids` (nullptr: RT_CROSS_OTHER_OBJECTS is off) is the objects' table.
template <bool WIDE, bool LIST, bool ANY, bool SELF>
RT_DEV void walk_probes(const DScene& sc, walk::StackLds& lds, const float4* __restrict__ probes, const uint32_t* __restrict__ ids, uint32_t first_probe, uint32_t n,
    uint32_t max_list, bool any, float4* __restrict__ out, float4* __restrict__ members, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);
    const bool stop_at_first = ANY || (SELF && any);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, count = 0u, lowest = RT_INVALID_ID, self_prim = RT_INVALID_ID, self_object = RT_INVALID_ID;
        RgList list;
        if (LIST) rg_list_clear(list, max_list);
        stack.sp = 0;
        CrossProbe q;
        {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
            if (i < n)
            {
                if (SELF)
                {
                    self_prim = first_probe + i;
                    const float4* tp = sc.tris_sh + (size_t)self_prim * 8;
                    a = tp[0]; b = tp[1]; c = tp[2];
                    if (ids) self_object = ids[self_prim];
                }
                else { a = probes[(size_t)i * 3u]; b = probes[(size_t)i * 3u + 1u]; c = probes[(size_t)i * 3u + 2u]; }
            }
            const float q1[3] = {a.x, a.y, a.z}, q2[3] = {b.x, b.y, b.z}, q3[3] = {c.x, c.y, c.z};
            cross_probe_make(q, q1, q2, q3);
        }
        if (i < n && q.searched) ref = WIDE ? sc.w_entry_ref : sc.entry_ref;

        auto leaf = [&](uint32_t prim, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
        {
            bool skipped = false;
            if (SELF)
            {
                skipped = prim == self_prim || cross_shares_corner(q, p1, p2, p3);
                if (!skipped && ids) skipped = ids[prim] == self_object;
            }
            if (!skipped && cross_test(q, p1, p2, p3))
            {
                ++count;
                lowest = prim < lowest ? prim : lowest;
                if (LIST) rg_list_insert(list, prim);
            }
        };
        auto box = [&](float4 q0, float4 q1, float4 q2, float4 q3) { walk::cross_box_step<WIDE>(q0, q1, q2, q3, q.lo, q.hi, q.pl, q.plane, ref, stack); };
        auto keep = [](float) { return true; };
        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF)
            {
                walk::volume_step<WIDE>(sc, ref, stack, leaf, box, keep);
                if (stop_at_first && count != 0u) ref = RT_IDLE_REF;
            }

        if (i < n)
        {
            if (LIST)
            {
                // place t holds member t - first (region.h: the list is kept right-aligned)
                const uint32_t stored = count < max_list ? count : max_list, first = rg_list_first(max_list);
#pragma unroll
                for (uint32_t t = 0; t < RT_CROSS_LIST_MAX; ++t)
                    if (t >= first)
                    {
                        const uint32_t j = t - first;
                        const bool valid = j < stored;
                        const uint32_t prim = valid ? list.key[t] - 1u : 0u;
                        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
                        if (valid)
                        {
                            const float4* tp = sc.tris_sh + (size_t)prim * 8;
                            a = tp[0]; b = tp[1]; c = tp[2];
                        }
                        const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
                        write_member(members + ((size_t)i * max_list + j) * 2u, q, valid, prim, p1, p2, p3);
                    }
            }
            store_record(out + i, cross_record(count, lowest, max_list, q.searched, stop_at_first));
        }
    }
    stack.report(status);
}

template <bool WIDE, bool LIST, bool ANY>
__global__ __launch_bounds__(64) void k_cross(DScene sc, const float4* __restrict__ probes, uint32_t n, uint32_t max_list, float4* __restrict__ out,
    float4* __restrict__ members, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk_probes<WIDE, LIST, ANY, false>(sc, lds, probes, nullptr, 0u, n, max_list, ANY, out, members, spill, status);
}

template <bool WIDE, bool LIST>
__global__ __launch_bounds__(64) void k_cross_self(DScene sc, const uint32_t* __restrict__ ids, uint32_t first, uint32_t n, uint32_t max_list, uint32_t any,
    float4* __restrict__ out, float4* __restrict__ members, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk_probes<WIDE, LIST, false, true>(sc, lds, nullptr, ids, first, n, max_list, any != 0u, out, members, spill, status);
}

// cross.h over every triangle, no tree.  probes == nullptr: the self form, probe i is tris[first + i] (ids: as above).  members may be nullptr when
// max_list == 0.  An RT_CROSS_ANY answer stops at the first member in array order: count 0 or 1, which is all it reports.
__global__ __launch_bounds__(64) void k_cross_brute(const rt_triangle* __restrict__ tris, uint32_t n_tris, const float4* __restrict__ probes,
    const uint32_t* __restrict__ ids, uint32_t first, uint32_t n, uint32_t max_list, uint32_t any, float4* __restrict__ out, float4* __restrict__ members)
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
    uint32_t count = 0u, lowest = RT_INVALID_ID;
    RgList list;
    rg_list_clear(list, max_list);
    if (q.searched)
        for (uint32_t t = 0; t < n_tris && !(any != 0u && count != 0u); ++t)
        {
            walk::triangle_corners(tris[t], p1, p2, p3);
            if (self && (t == self_prim || cross_shares_corner(q, p1, p2, p3) || (ids && ids[t] == self_object))) continue;
            if (!cross_test(q, p1, p2, p3)) continue;
            ++count;
            lowest = t < lowest ? t : lowest;
            rg_list_insert(list, t);
        }
    const uint32_t stored = any != 0u ? 0u : (count < max_list ? count : max_list), place = rg_list_first(max_list);
#pragma unroll
    for (uint32_t t = 0; t < RT_CROSS_LIST_MAX; ++t)
        if (t >= place)
        {
            const uint32_t j = t - place;
            if (j >= max_list) continue;
            const bool valid = j < stored;
            const uint32_t prim = valid ? list.key[t] - 1u : 0u;
            if (valid) walk::triangle_corners(tris[prim], p1, p2, p3);
            write_member(members + ((size_t)i * max_list + j) * 2u, q, valid, prim, p1, p2, p3);
        }
    store_record(out + i, cross_record(count, lowest, max_list, q.searched, any != 0u));
}
} // namespace cross
