// bake_kernels.h -- the kernels of an occlusion bake (rt_scene_bake / rt_scene_bake_buffer / rt_debug_bake_rays): a hemisphere of any-hit
// rays per CALLER-supplied point, generated, walked and reduced on the device.  The arithmetic is bake.h's.
//
//   k_bake       one wave per group of points, 64-thread blocks: a point record in (32 or 64 bytes), rt_bake_result (16 bytes) out
//   k_bake_rays  one lane per ray: the rays k_bake would walk, written out as rt_ray (rt_debug_bake_rays's device form)
//
// Mapping.  L = min(samples, 64) lanes own one point, a wave owns 64 / L points (1, 2 or 4); the persistent grid strides over such groups.  Lane l of a
// point is its reduction slot l: it generates and walks rays l, l + L, l + 2 L, ... itself, in this order, and adds every unoccluded direction to a sum of its
// own -- so a lane whose ray has ended starts its next one at once (the lane refill k_query_trace cannot have: a query's lanes share nothing that says which
// ray is next), and no result depends on which lane ends when.  The wave moves on to its next group when every lane has run dry.
//
// The walk is k_query_trace<true>'s with t_min = 0 and t_max = radius: walk_kernels.h's ray_setup, ray_step<true> and Stack, which explains it and argues its
// exactness -- the 4-wide shadow records with w4_test_slots in stored order, the exact child-pair records for RT_SIGN_SLOW rays, origins beyond 2^29 and scenes
// without a usable 4-wide tree; RT_QUERY_STACK_LDS stack entries per lane in LDS, the rest in the lane's slice of a spill area sized by the grid,
// RT_W4_STACK_MAX in all, an overrun raises *status and stores nothing.  An any-hit walk ends where a triangle is accepted, so the step's lowered t_max and its
// barycentrics are dropped: the verdict is all a bake keeps.
//
// Reduction.  The count: every lane counts its own unoccluded rays (at most 64); per bit of that count one ballot, masked to the point's lanes and popcounted.
// The bent normal: bake.h's halving tree over the L slot sums with __shfl_down inside the point's L lanes (lanes l >= s read values that no later step uses).
#pragma once
#include "walk_kernels.h"
#include "bake.h"

namespace bake
{
__global__ __launch_bounds__(64) void k_bake(DScene sc, const float4* __restrict__ points, uint32_t from_surfaces, uint32_t n, uint32_t first_index,
    uint32_t samples, uint32_t seed, float bias, float radius, float4* __restrict__ out, uint2* __restrict__ spill, uint32_t use_wide,
    uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const uint32_t L = samples < 64u ? samples : 64u;            // lanes (= reduction slots) per point
    const uint32_t per_wave = 64u / L;
    const uint32_t sub = lane / L, slot = lane % L;
    const unsigned long long seg_mask = (L == 64u ? ~0ull : ((1ull << L) - 1ull)) << (sub * L);
    const uint32_t n_groups = n / per_wave + (n % per_wave != 0u ? 1u : 0u);
    const uint32_t stride = from_surfaces ? 4u : 2u;             // float4 per point record

    for (uint32_t group = blockIdx.x; group < n_groups; group += gridDim.x)
    {
        const unsigned long long p = (unsigned long long)group * per_wave + sub;
        BakeFrame f;
        f.walked = false;
        float r1 = 0.0f, r2 = 0.0f;
        if (p < n)
        {
            const float4* rec = points + (size_t)p * stride;
            const float4 a = rec[0], b = rec[from_surfaces ? 2 : 1];
            float pos[3] = {a.x, a.y, a.z}, nrm[3] = {b.x, b.y, b.z};
            bool record_ok = true;
            if (from_surfaces)
            {
                const uint32_t flags = __float_as_uint(rec[3].w);
                record_ok = (flags & QS_FLAG_HIT) != 0u;
                if (flags & QS_FLAG_BACK_FACE) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
            }
            f = bake_frame(pos, nrm, record_ok, bias);
            bake_rotations(first_index + (uint32_t)p, seed, &r1, &r2);
            // an origin that the bias made non-finite: its rays are not walked by a query either (ray_walkable) -- every ray a miss
        }
        const f3 org = F3(f.origin[0], f.origin[1], f.origin[2]);
        const bool origin_ok = __builtin_isfinite(org.x) && __builtin_isfinite(org.y) && __builtin_isfinite(org.z);

        uint32_t ref = RT_IDLE_REF, k = slot, cnt = 0u;
        walk::Ray ray = walk::ray_idle();
        f3 sum = F3s(0.0f);
        bool hit = false;

        // ray k of this lane's point: its direction and where its walk starts
        auto start = [&]()
        {
            float d[3];
            bake_direction(f, r1, r2, k, samples, d);
            ray = walk::ray_setup(org, F3(d[0], d[1], d[2]), use_wide);
            hit = false;
            stack.sp = 0;
            const bool walkable = origin_ok && __builtin_isfinite(d[0]) && __builtin_isfinite(d[1]) && __builtin_isfinite(d[2]) &&
                                  !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f);
            ref = walkable ? walk::ray_entry<true>(sc, ray) : RT_IDLE_REF;
        };
        // a ray has ended: its verdict joins the lane's sum, and the lane's next ray starts
        auto finish = [&]()
        {
            if (!hit) { sum = sum + ray.dir; ++cnt; }
            k += L;
        };
        if (f.walked)
        {
            start();
            while (ref == RT_IDLE_REF && k < samples) { finish(); if (k < samples) start(); }    // (rays that are not walked end at once)
        }
        else k = samples;

        while (__ballot(ref != RT_IDLE_REF) != 0ull)
        {
            if (ref != RT_IDLE_REF)
            {
                float t_max = radius, hit_u = 0.0f, hit_v = 0.0f;             // the step's own copies: only its verdict is kept
                uint32_t hit_prim = RT_INVALID_ID;
                if (walk::ray_step<true>(sc, ray, 0.0f, t_max, ref, stack, hit_u, hit_v, hit_prim)) hit = true;
                if (ref == RT_IDLE_REF)                                       // this lane's ray ended in this pass: the refill
                {
                    finish();
                    if (k < samples) start();
                    while (ref == RT_IDLE_REF && k < samples) { finish(); if (k < samples) start(); }
                }
            }
        }

        // the whole wave is here: count and bent normal of each of its points
        uint32_t unoccluded = 0u;
#pragma unroll
        for (uint32_t bit = 0; bit < 7u; ++bit)                                  // a lane's count is at most 4096 / 64
            unoccluded += (uint32_t)__popcll(__ballot(((cnt >> bit) & 1u) != 0u) & seg_mask) << bit;
        for (uint32_t s = L >> 1; s > 0u; s >>= 1)
        {
            const float x = __shfl_down(sum.x, s, (int)L), y = __shfl_down(sum.y, s, (int)L), z = __shfl_down(sum.z, s, (int)L);
            sum = F3(sum.x + x, sum.y + y, sum.z + z);
        }
        if (slot == 0u && p < n)
        {
            const float S[3] = {sum.x, sum.y, sum.z};
            float bent[3];
            bake_bent(S, bent);
            out[p] = f.walked ? make_float4(bent[0], bent[1], bent[2], __uint_as_float(unoccluded)) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(RT_INVALID_ID));
        }
    }
    stack.report(status);
}

// rays[p * samples + k] = ray k of point p as k_bake walks it; a skipped point's rays are all zeros (a zero direction: a ray no query walks)
__global__ __launch_bounds__(256) void k_bake_rays(const float4* __restrict__ points, uint32_t from_surfaces, uint32_t n, uint32_t first_index, uint32_t samples,
    uint32_t seed, float bias, float radius, float4* __restrict__ rays)
{
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned long long)n * samples) return;
    const uint32_t p = (uint32_t)(idx / samples), k = (uint32_t)(idx % samples);
    const float* rec = reinterpret_cast<const float*>(points + (size_t)p * (from_surfaces ? 4u : 2u));
    float pos[3], nrm[3];
    const bool record_ok = bake_point(rec, from_surfaces != 0u, pos, nrm);
    const BakeFrame f = bake_frame(pos, nrm, record_ok, bias);
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = o;
    if (f.walked)
    {
        float r1, r2, dd[3];
        bake_rotations(first_index + p, seed, &r1, &r2);
        bake_direction(f, r1, r2, k, samples, dd);
        o = make_float4(f.origin[0], f.origin[1], f.origin[2], 0.0f);
        d = make_float4(dd[0], dd[1], dd[2], radius);
    }
    rays[2 * idx] = o;
    rays[2 * idx + 1] = d;
}
} // namespace bake
