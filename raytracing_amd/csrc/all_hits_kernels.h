// all_hits_kernels.h -- the kernels of an all-hits query (rt_scene_trace_all / rt_scene_trace_all_buffer / rt_frame_pick_all / rt_debug_trace_all, DESIGN.md
// section 7k): every surface a CALLER's ray crosses, counted, the nearest RT_ALL_HITS_MAX of them sorted.
//
//   k_all_hits<LIST>     one lane per ray, 64-thread blocks, k_query_trace's strided chunks: rt_ray in, rt_ray_hits (16 bytes) and max_hits rt_hit out
//   k_all_hits_surface   one lane per (ray, stored hit): rt_surface from the hit and the triangle's 128-byte shading record (query.h's arithmetic)
//   k_all_hits_brute     one lane per ray over every leaf of an rt_bvh_node array and rt_triangles: the device half of rt_debug_trace_all
//
// The walk is walk_kernels.h's: walk::Stack, walk::ray_setup, walk::ray_entry<true> and walk::ray_step<walk::RAY_ALL_HITS> -- the any-hit walk (the shadow
// rays' 4-wide tree in stored order; the child-pair records for slow or far rays and when there is no usable 4-wide tree) that does not stop at an accepted
// triangle and never lowers t_max.  The hit set does not depend on the records walked: a leaf is reached exactly when its box passes with the ray's own range
// ("leaf box passes => stored box passes", trace_kernels.h), and it is reached once.  The pop's re-test t_max >= entry always passes: t_max is constant.
//
// LIST = false keeps two counters.  LIST = true also keeps an AhList (all_hits.h): 16 registers, bc not kept.  After the walk the stored hits' bc are made
// again by ah_triangle on the kept triangles' records: the same function on the same operands, so the same bits.
#pragma once
#include "walk_kernels.h"

namespace all_hits
{
RT_DEV float4 hit_none() { return make_float4(0.0f, 0.0f, __uint_as_float(RT_INVALID_ID), 0.0f); }

RT_DEV void store_record(float4* o, const rt_ray_hits& r)
{
    q_store(o, make_float4(__uint_as_float(r.count), __uint_as_float(r.entering), __uint_as_float(r.stored), __uint_as_float(r.flags)));
}

// hits[(i * max_hits + j) * hit_stride]: hit j of ray i (hit_stride 4: the first 16 bytes of each surface record, for a query that returns surfaces only)
template <bool LIST>
__global__ __launch_bounds__(64) void k_all_hits(DScene sc, const float4* __restrict__ rays, uint32_t n, uint32_t max_hits, float4* __restrict__ out,
    float4* __restrict__ hits, uint32_t hit_stride /* in float4 */, uint2* __restrict__ spill, uint32_t use_wide, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, unused_prim = RT_INVALID_ID, count = 0u, entering = 0u;
        walk::Ray ray = walk::ray_idle();
        float t_min = 0.0f, t_max = 0.0f, unused_u = 0.0f, unused_v = 0.0f;
        bool walked = false;
        AhList list;
        if (LIST) ah_list_clear(list);
        stack.sp = 0;
        if (i < n)
        {
            const float4 q0 = q_load(rays + 2 * (size_t)i), q1 = q_load(rays + 2 * (size_t)i + 1);
            walked = walk::ray_walkable(q0, q1);
            if (walked)
            {
                t_min = q0.w; t_max = q1.w;
                ray = walk::ray_setup(F3(q0.x, q0.y, q0.z), F3(q1.x, q1.y, q1.z), use_wide);
                ref = walk::ray_entry<true>(sc, ray);
            }
        }

        auto sink = [&](uint32_t prim, float t, float det)
        {
            ++count;
            if (det > 0.0f) ++entering;
            if (LIST) ah_list_insert(list, t, prim);
        };
        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF) (void)walk::ray_step<walk::RAY_ALL_HITS>(sc, ray, t_min, t_max, ref, stack, unused_u, unused_v, unused_prim, sink);

        if (i < n)
        {
            uint32_t exits = 0u;
            if (LIST)
            {
                const float o[3] = {ray.org.x, ray.org.y, ray.org.z}, d[3] = {ray.dir.x, ray.dir.y, ray.dir.z};
#pragma unroll
                for (uint32_t j = 0; j < RT_ALL_HITS_MAX; ++j)
                    if (j < max_hits)
                    {
                        float4 h = hit_none();
                        if (j < count)
                        {
                            const uint32_t prim = list.prim[j];
                            const float4* rp = sc.tris_rt + (size_t)prim * 4;
                            const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2];
                            const float p1[3] = {q0.x, q0.y, q0.z}, e1[3] = {q1.x, q1.y, q1.z}, e2[3] = {q2.x, q2.y, q2.z};
                            float u = 0.0f, v = 0.0f, t = 0.0f, det = 0.0f;
                            (void)ah_triangle(o, d, p1, e1, e2, t_min, t_max, &u, &v, &t, &det);
                            if (det < 0.0f) exits |= 1u << j;
                            h = make_float4(u, v, __uint_as_float(prim), t);
                        }
                        q_store(hits + ((size_t)i * max_hits + j) * hit_stride, h);
                    }
            }
            store_record(out + i, ah_record(count, entering, max_hits, exits, walked));
        }
    }
    stack.report(status);
}

// k_query_surface's body (walk::ray_surface) with hit j of ray i reading ray i.  hits[k * hit_stride] may be the first 16 bytes of out[k] itself: lane k reads it before it writes.
__global__ __launch_bounds__(256) void k_all_hits_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ rays, const float4* hits, uint32_t hit_stride, uint32_t max_hits, unsigned long long total, float4* out)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k < total) walk::ray_surface<true>(tris, n_tris, object_of_triangle, rays + 2 * (size_t)(k / max_hits), hits, hit_stride, (size_t)k, out);
}

// Every leaf of `nodes` (the host has checked that each leaf's triangles lie inside the array): the leaf's box test -- box_test_fast, or box_test for an
// RT_SIGN_SLOW ray -- then ah_triangle on p1, fl(p2 - p1), fl(p3 - p1) of its triangles.
__global__ __launch_bounds__(256) void k_all_hits_brute(const rt_bvh_node* __restrict__ nodes, uint32_t nn, const rt_triangle* __restrict__ tris,
    const float4* __restrict__ rays, uint32_t n, uint32_t max_hits, float4* __restrict__ out, float4* __restrict__ hits)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    const bool walked = walk::ray_walkable(r0, r1);
    uint32_t count = 0u, entering = 0u, exits = 0u;
    AhList list;
    ah_list_clear(list);
    const float o[3] = {r0.x, r0.y, r0.z}, d[3] = {r1.x, r1.y, r1.z};
    const float t_min = r0.w, t_max = r1.w;
    auto corners = [&](uint32_t prim, float (&p1)[3], float (&e1)[3], float (&e2)[3])
    {
        float p2[3], p3[3];
        walk::triangle_corners(tris[prim], p1, p2, p3);
        for (int a = 0; a < 3; ++a) { e1[a] = p2[a] - p1[a]; e2[a] = p3[a] - p1[a]; }
    };
    if (walked)
    {
        const float4 q = ray_inverse(F3(d[0], d[1], d[2]));
        const f3 org = F3(o[0], o[1], o[2]), inv = F3(q.x, q.y, q.z);
        const bool slow = (__float_as_uint(q.w) & RT_SIGN_SLOW) != 0u;
        for (uint32_t k = 0; k < nn; ++k)
        {
            const rt_bvh_node nd = nodes[k];
            const uint32_t np = nd.num_primitives_axis >> 16;
            if (np == 0u) continue;
            float entry;
            const bool inside = slow ? box_test(nd.bounds_min.x, nd.bounds_min.y, nd.bounds_min.z, nd.bounds_max.x, nd.bounds_max.y, nd.bounds_max.z, org, inv, t_min, t_max, entry)
                                     : box_test_fast(nd.bounds_min.x, nd.bounds_min.y, nd.bounds_min.z, nd.bounds_max.x, nd.bounds_max.y, nd.bounds_max.z, org, inv, t_min, t_max, entry);
            if (!inside) continue;
            for (uint32_t prim = nd.offset; prim < nd.offset + np; ++prim)
            {
                float p1[3], e1[3], e2[3], u, v, t, det;
                corners(prim, p1, e1, e2);
                if (!ah_triangle(o, d, p1, e1, e2, t_min, t_max, &u, &v, &t, &det)) continue;
                ++count;
                if (det > 0.0f) ++entering;
                ah_list_insert(list, t, prim);
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < RT_ALL_HITS_MAX; ++j)
        if (j < max_hits)
        {
            float4 h = hit_none();
            if (j < count)
            {
                float p1[3], e1[3], e2[3], u = 0.0f, v = 0.0f, t = 0.0f, det = 0.0f;
                corners(list.prim[j], p1, e1, e2);
                (void)ah_triangle(o, d, p1, e1, e2, t_min, t_max, &u, &v, &t, &det);
                if (det < 0.0f) exits |= 1u << j;
                h = make_float4(u, v, __uint_as_float(list.prim[j]), t);
            }
            hits[(size_t)i * max_hits + j] = h;
        }
    store_record(out + i, ah_record(count, entering, max_hits, exits, walked));
}
} // namespace all_hits
