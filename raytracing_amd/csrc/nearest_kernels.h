// nearest_kernels.h -- the kernels of a nearest-point query (rt_scene_nearest / rt_scene_nearest_buffer / rt_debug_nearest): for each
// CALLER-supplied point the nearest triangle of the uploaded scene, where on it, and how far.  The arithmetic is nearest.h's.
//
//   k_nearest<WIDE>    one lane per point, 64-thread blocks: rt_point in (16 bytes, one dwordx4), rt_nearest out (32 bytes, two dwordx4)
//   k_nearest_brute    one lane per point over ALL triangles of an rt_triangle array (rt_debug_nearest's device form: the same nearest.h with no tree)
//   k_nearest_surface  one lane per point: rt_surface (64 bytes) of the nearest point, by query.h's query_surface
//
// The walk: walk_kernels.h's volume_step (the fetch, the leaf chain, the `last` rule) with walk::point_box_step at a box record.  What differs from a ray's
// walk is the test and the order: a box is passed when !(nearest_box_d2 > best),
// the nearest passing box is visited next, and the others wait on the stack with their nearest_box_d2 as the entry value, farthest deepest; a pop re-tests
// !(entry > best).  nearest_box_d2 <= d2 holds in binary32 itself for every box that holds a triangle's corners (nearest.h), so no order, no fold and no
// quantisation of a box can change the result: it is the brute-force minimum bit for bit.
//   * a 4-wide record: the four slots' boxes are origin + q * cell, exactly representable (wide_quant.h: wide_frame keeps the grid in binary32's reach,
//     wide_quantise rounds outward), so the bound applies to them as to any box; RT_EMPTY_REF slots are skipped.
//   * a child-pair record: the two children's exact boxes, the same step with two candidates.
//   * a leaf: its triangles in array order.  The leaf's exact box in the trace record is not tested again:
//     a slot's box is that box rounded outward by less than a cell, and the test would cost every leaf a pass of its own.
//   * a point that is not searched (nearest.h) is not walked.  Points far outside the scene need no special walk: the gaps stay finite or overflow to +inf on
//     both sides of every comparison.
// WIDE is the launch's, not the lane's: nearest::launch takes the 4-wide records when Scene::wide_ok holds (query::launch's rule), the child-pair records
// otherwise (RT_CTX_OPT_WIDE_BVH = 0, a refit that disqualified the wide tree).
//
// Stack: walk::Stack with (ref, nearest_box_d2) entries, in the ray queries' spill area (at most three pending slots per wide level, one pending child per
// pair level).  A push beyond RT_W4_STACK_MAX is not written; it raises the ray queries' status word.
//
// Grid: k_query_trace's persistent strided chunks of 64 consecutive points.
#pragma once
#include "walk_kernels.h"
#include "nearest.h"

namespace nearest
{
template <bool WIDE>
__global__ __launch_bounds__(64) void k_nearest(DScene sc, const float4* __restrict__ points, uint32_t n, float4* __restrict__ out, uint32_t out_stride /* in float4 */,
    uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, best_prim = RT_INVALID_ID;
        float p[3] = {0.0f, 0.0f, 0.0f};
        float best = 0.0f;
        stack.sp = 0;
        if (i < n)
        {
            const float4 q = q_load(points + i);
            p[0] = q.x; p[1] = q.y; p[2] = q.z;
            if (nearest_searched(p, q.w))
            {
                best = q.w * q.w;
                ref = WIDE ? sc.w_entry_ref : sc.entry_ref;
            }
        }

        auto leaf = [&](uint32_t prim, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
        {
            const NpTriangle t = nearest_point_triangle(p, p1, p2, p3);
            if (nearest_accepts(t.d2, prim, best, best_prim)) { best = t.d2; best_prim = prim; }
        };
        auto box = [&](float4 q0, float4 q1, float4 q2, float4 q3) { walk::point_box_step<WIDE>(q0, q1, q2, q3, p, best, ref, stack); };
        auto keep = [&](float entry) { return !(entry > best); };
        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF) walk::volume_step<WIDE>(sc, ref, stack, leaf, box, keep);

        if (i < n)
        {
            rt_nearest o = nearest_none();
            if (best_prim != RT_INVALID_ID)
            {
                const float4* tp = sc.tris_sh + (size_t)best_prim * 8;
                const float4 a = tp[0], b = tp[1], c = tp[2];
                const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
                o = nearest_record(p, p1, p2, p3, best_prim);
            }
            walk::store_nearest(out + (size_t)i * out_stride, o);
        }
    }
    stack.report(status);
}

__global__ __launch_bounds__(256) void k_nearest_brute(const rt_triangle* __restrict__ tris, uint32_t n_tris, const float4* __restrict__ points, uint32_t n,
    float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    const float p[3] = {q.x, q.y, q.z};
    rt_nearest o = nearest_none();
    if (nearest_searched(p, q.w))
    {
        float best = q.w * q.w;
        uint32_t best_prim = RT_INVALID_ID;
        float p1[3], p2[3], p3[3];
        for (uint32_t t = 0; t < n_tris; ++t)
        {
            walk::triangle_corners(tris[t], p1, p2, p3);
            const NpTriangle c = nearest_point_triangle(p, p1, p2, p3);
            if (nearest_accepts(c.d2, t, best, best_prim)) { best = c.d2; best_prim = t; }
        }
        if (best_prim != RT_INVALID_ID)
        {
            walk::triangle_corners(tris[best_prim], p1, p2, p3);
            o = nearest_record(p, p1, p2, p3, best_prim);
        }
    }
    walk::store_nearest(out + 2 * (size_t)i, o);
}

// found[i * found_stride .. + 1] = point i's rt_nearest; it may be the first 32 bytes of out[i] itself (a query that returns surfaces only keeps its records
// there): lane i reads it before it writes.  `tris` = the scene's 128-byte shading records (walk::read_shading_triangle).
__global__ __launch_bounds__(256) void k_nearest_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ points, const float4* found, uint32_t found_stride, uint32_t n, float4* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) walk::point_surface(tris, n_tris, object_of_triangle, points + i, found, found_stride, i, out);
}
} // namespace nearest
