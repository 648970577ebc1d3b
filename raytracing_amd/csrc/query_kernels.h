// query_kernels.h -- the kernels of a ray query (rt_scene_trace / rt_scene_trace_buffer / rt_frame_pick): CALLER-supplied rays against the
// uploaded scene's trees.
//
//   k_query_trace<ANY_HIT>   one lane per ray, 64-thread blocks: rt_ray in (32 bytes, two dwordx4), rt_hit (16 bytes) or one dword out
//   k_query_surface<RECORDS> one lane per ray: rt_surface (64 bytes) from the hit and the triangle's 128-byte shading record (query.h's arithmetic)
//
// The walk -- its step, its stack, a ray's set-up, and the argument for its exactness -- is walk_kernels.h's, shared with k_bake and k_nearest; k_query_trace is
// the loop around it: block b takes chunks b, b + blocks, ... of 64 consecutive rays and finishes a chunk before it takes the next (no refill of single lanes:
// a query has no queue counters or work heads to share).
#pragma once
#include "walk_kernels.h"

namespace query
{
template <bool ANY_HIT>
__global__ __launch_bounds__(64) void k_query_trace(DScene sc, const float4* __restrict__ rays, uint32_t n, float4* __restrict__ hits, uint32_t hit_stride /* in float4 */,
    uint32_t* __restrict__ occluded, uint2* __restrict__ spill, uint32_t use_wide, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);          // (n + 63 would wrap above 2^32 - 64)

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, hit_prim = RT_INVALID_ID;
        walk::Ray ray = walk::ray_idle();
        float t_min = 0.0f, t_max = 0.0f, hit_u = 0.0f, hit_v = 0.0f;
        bool walked = false;
        stack.sp = 0;
        if (i < n)
        {
            const float4 q0 = q_load(rays + 2 * (size_t)i), q1 = q_load(rays + 2 * (size_t)i + 1);
            walked = walk::ray_walkable(q0, q1);
            if (walked)
            {
                t_min = q0.w; t_max = q1.w;
                ray = walk::ray_setup(F3(q0.x, q0.y, q0.z), F3(q1.x, q1.y, q1.z), use_wide);
                ref = walk::ray_entry<ANY_HIT>(sc, ray);
            }
        }

        while (__ballot(ref != RT_IDLE_REF) != 0ull)
            if (ref != RT_IDLE_REF) (void)walk::ray_step<ANY_HIT>(sc, ray, t_min, t_max, ref, stack, hit_u, hit_v, hit_prim);

        if (i < n)
        {
            if (hits)
                q_store(hits + (size_t)i * hit_stride, walked ? make_float4(hit_u, hit_v, __uint_as_float(hit_prim), t_max)
                                                              : make_float4(0.0f, 0.0f, __uint_as_float(RT_INVALID_ID), 0.0f));
            if (occluded) occluded[i] = hit_prim != RT_INVALID_ID ? 1u : 0u;
        }
    }
    stack.report(status);
}

// RECORDS: `tris` = the scene's 128-byte shading records (walk::read_shading_triangle); otherwise rt_triangle[]
// (rt_debug_query_surface: they stand in for the records).  hits[i * hit_stride] may be the first 16 bytes of out[i] itself (a query that returns surfaces only
// keeps its hits there): lane i reads it before it writes.
template <bool RECORDS>
__global__ __launch_bounds__(256) void k_query_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ rays, const float4* hits, uint32_t hit_stride, uint32_t n, float4* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) walk::ray_surface<RECORDS>(tris, n_tris, object_of_triangle, rays + 2 * (size_t)i, hits, hit_stride, i, out);
}
} // namespace query
