// within_kernels.h -- the kernels of a range query (rt_scene_within / rt_scene_within_buffer / rt_debug_within): for each
// CALLER-supplied point every triangle of the uploaded scene within max_distance, counted, the nearest RT_WITHIN_MAX of them sorted.  The arithmetic is
// nearest.h's, the membership rule and the list within.h's.
//
//   k_within<WIDE, LIST, KNN>   one lane per point, 64-thread blocks: rt_point in (16 bytes), rt_point_hits out (16 bytes) and max_near rt_nearest (LIST)
//   k_within_brute              one lane per point over ALL triangles of an rt_triangle array (rt_debug_within's device form: within.h with no tree)
//   k_within_surface            one lane per (point, listed member): rt_surface (64 bytes) of the member's nearest point, by query.h's query_surface
//
// The walk: walk_kernels.h's volume_step with walk::point_box_step at a box record, as k_nearest's (nearest_kernels.h) -- with another bound.  k_nearest prunes by the best d2 so far; a counting walk (KNN = false) prunes by r2 and never lowers it, so it reaches every leaf whose box
// the sphere touches; a k-nearest walk (KNN = true, 1 <= max_near) prunes by r2 until the list's place max_near - 1 is taken and by that place's d2 from then
// on.  within.h says why either gives the brute force's members bit for bit, whichever records are walked.
//
// LIST = false keeps `count` and the running (best, best_prim) of nearest_accepts for nearest_primitive.  LIST = true keeps a WnList (within.h): 16 registers,
// the records not kept; its members are right-aligned, so the k-th is a static place.  After the walk the listed members' records are made again by nearest_record on the kept triangles' corners: the same function on the
// same operands, so the same bits.  KNN implies LIST.
//
// Stack, spill area, status word and grid: k_nearest's (walk::Stack with (ref, nearest_box_d2) entries; a push beyond RT_W4_STACK_MAX is not written and raises
// the ray queries' status word; persistent strided chunks of 64 consecutive points).
#pragma once
#include "walk_kernels.h"
#include "within.h"

namespace within
{
RT_DEV void store_record(float4* o, const rt_point_hits& r)
{
    q_store(o, make_float4(__uint_as_float(r.count), __uint_as_float(r.stored), __uint_as_float(r.nearest_primitive), __uint_as_float(r.flags)));
}

// near[(i * max_near + j) * near_stride]: member j of point i (near_stride 4: the first 32 bytes of each surface record, for a query that returns surfaces only)
template <bool WIDE, bool LIST, bool KNN>
__global__ __launch_bounds__(64) void k_within(DScene sc, const float4* __restrict__ points, uint32_t n, uint32_t max_near, uint32_t options,
    float4* __restrict__ out, float4* __restrict__ near, uint32_t near_stride /* in float4 */, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    static_assert(LIST || !KNN, "a k-nearest walk keeps the list");
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, best_prim = RT_INVALID_ID, count = 0u;
        float p[3] = {0.0f, 0.0f, 0.0f};
        float r2 = 0.0f, bound = 0.0f;          // bound: what prunes (KNN: lowered by the list); !LIST: the running best of nearest_accepts, which prunes nothing
        bool searched = false;
        WnList list;
        if (LIST) wn_list_clear(list, max_near);
        stack.sp = 0;
        if (i < n)
        {
            const float4 q = q_load(points + i);
            p[0] = q.x; p[1] = q.y; p[2] = q.z;
            searched = nearest_searched(p, q.w);
            if (searched)
            {
                r2 = q.w * q.w;
                bound = r2;
                ref = WIDE ? sc.w_entry_ref : sc.entry_ref;
            }
        }

        auto leaf = [&](uint32_t prim, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
        {
            const NpTriangle t = nearest_point_triangle(p, p1, p2, p3);
            if (within_member(t.d2, r2))
            {
                ++count;
                if (LIST)
                {
                    wn_list_insert(list, t.d2, prim);
                    if (KNN) bound = within_knn_bound(list, r2);
                }
            }
            if (!LIST && nearest_accepts(t.d2, prim, bound, best_prim)) { bound = t.d2; best_prim = prim; }
        };
        auto box = [&](float4 q0, float4 q1, float4 q2, float4 q3) { walk::point_box_step<WIDE>(q0, q1, q2, q3, p, KNN ? bound : r2, ref, stack); };
        auto keep = [&](float entry) { return !(entry > (KNN ? bound : r2)); };
        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF) walk::volume_step<WIDE>(sc, ref, stack, leaf, box, keep);

        if (i < n)
        {
            if (LIST)
            {
                // place t holds member t - first (within.h: the list is kept right-aligned)
                const uint32_t stored = count < max_near ? count : max_near, first = wn_list_first(max_near);
#pragma unroll
                for (uint32_t t = 0; t < RT_WITHIN_MAX; ++t)
                    if (t >= first)
                    {
                        const uint32_t j = t - first;
                        rt_nearest o = nearest_none();
                        if (j < stored)
                        {
                            const uint32_t prim = list.prim[t];
                            const float4* tp = sc.tris_sh + (size_t)prim * 8;
                            const float4 a = tp[0], b = tp[1], c = tp[2];
                            const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
                            o = nearest_record(p, p1, p2, p3, prim);
                        }
                        if (j == 0u) best_prim = o.primitive_id;
                        walk::store_nearest(near + ((size_t)i * max_near + j) * near_stride, o);
                    }
            }
            store_record(out + i, within_record(count, max_near, options, best_prim, searched));
        }
    }
    stack.report(status);
}

// within.h over every triangle, no tree.  near may be nullptr when max_near == 0.
__global__ __launch_bounds__(256) void k_within_brute(const rt_triangle* __restrict__ tris, uint32_t n_tris, const float4* __restrict__ points, uint32_t n,
    uint32_t max_near, uint32_t options, float4* __restrict__ out, float4* __restrict__ near)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    const float p[3] = {q.x, q.y, q.z};
    const bool searched = nearest_searched(p, q.w);
    uint32_t count = 0u;
    WnList list;
    wn_list_clear(list, max_near);
    float p1[3], p2[3], p3[3];
    if (searched)
    {
        const float r2 = q.w * q.w;
        for (uint32_t t = 0; t < n_tris; ++t)
        {
            walk::triangle_corners(tris[t], p1, p2, p3);
            const NpTriangle c = nearest_point_triangle(p, p1, p2, p3);
            if (!within_member(c.d2, r2)) continue;
            ++count;
            wn_list_insert(list, c.d2, t);
        }
    }
    // the list keeps max(max_near, 1) members, so its first place names the nearest one also where none is listed
    const uint32_t stored = count < max_near ? count : max_near, first = wn_list_first(max_near);
    uint32_t first_prim = RT_INVALID_ID;
#pragma unroll
    for (uint32_t t = 0; t < RT_WITHIN_MAX; ++t)
        if (t >= first)
        {
            const uint32_t j = t - first;
            if (j == 0u) first_prim = list.prim[t];
            if (j >= max_near) continue;
            rt_nearest o = nearest_none();
            if (j < stored)
            {
                walk::triangle_corners(tris[list.prim[t]], p1, p2, p3);
                o = nearest_record(p, p1, p2, p3, list.prim[t]);
            }
            walk::store_nearest(near + 2 * ((size_t)i * max_near + j), o);
        }
    store_record(out + i, within_record(count, max_near, options, first_prim, searched));
}

// k_nearest_surface's body (walk::point_surface) with member j of point i reading point i.  found[k * found_stride .. + 1] may be the first 32 bytes of
// out[k] itself: lane k reads it before it writes.
__global__ __launch_bounds__(256) void k_within_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ points, const float4* found, uint32_t found_stride, uint32_t max_near, unsigned long long total, float4* out)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k < total) walk::point_surface(tris, n_tris, object_of_triangle, points + (size_t)(k / max_near), found, found_stride, (size_t)k, out);
}
} // namespace within
