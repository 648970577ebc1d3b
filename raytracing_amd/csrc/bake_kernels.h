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
// The walk is k_query_trace<true>'s, restated with t_min = 0 and t_max = radius (query_kernels.h explains it and argues its exactness; the step code is restated
// rather than shared so that the query kernels' instructions stay what they were): the 4-wide shadow records with w4_test_slots in stored order, the exact
// child-pair records for RT_SIGN_SLOW rays, origins beyond 2^29 and scenes without a usable 4-wide tree; the same stack -- RT_QUERY_STACK_LDS entries per lane
// in LDS, the rest in the lane's slice of a spill area sized by the grid, RT_W4_STACK_MAX in all, an overrun raises *status and stores nothing.
//
// Reduction.  The count: every lane counts its own unoccluded rays (at most 64); per bit of that count one ballot, masked to the point's lanes and popcounted.
// The bent normal: bake.h's halving tree over the L slot sums with __shfl_down inside the point's L lanes (lanes l >= s read values that no later step uses).
#pragma once
#include "query_kernels.h"
#include "bake.h"

namespace bake
{
__global__ __launch_bounds__(64) void k_bake(DScene sc, const float4* __restrict__ points, uint32_t from_surfaces, uint32_t n, uint32_t first_index,
    uint32_t samples, uint32_t seed, float bias, float radius, float4* __restrict__ out, uint2* __restrict__ spill, uint32_t use_wide,
    uint32_t* __restrict__ status)
{
    __shared__ uint2 stack[RT_QUERY_STACK_LDS][64];
    const uint32_t lane = threadIdx.x;
    uint2* const my_spill = spill + (size_t)(blockIdx.x * 64u + lane) * RT_QUERY_SPILL_PER_LANE;
    const char* const wide_base = reinterpret_cast<const char*>(sc.wnodes_sh);
    const char* const pair_base = reinterpret_cast<const char*>(sc.nodes);
    const char* const tri_base = reinterpret_cast<const char*>(sc.tris_rt);
    const float INF = __builtin_inff();
    const uint32_t L = samples < 64u ? samples : 64u;            // lanes (= reduction slots) per point
    const uint32_t per_wave = 64u / L;
    const uint32_t sub = lane / L, slot = lane % L;
    const unsigned long long seg_mask = (L == 64u ? ~0ull : ((1ull << L) - 1ull)) << (sub * L);
    const uint32_t n_groups = n / per_wave + (n % per_wave != 0u ? 1u : 0u);
    const uint32_t stride = from_surfaces ? 4u : 2u;             // float4 per point record
    bool overflow = false;

    for (uint32_t group = blockIdx.x; group < n_groups; group += gridDim.x)
    {
        const unsigned long long p = (unsigned long long)group * per_wave + sub;
        BakeFrame f;
        f.walked = false;
        float r1 = 0.0f, r2 = 0.0f;
        bool far_origin = false;
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
            far_origin = !(hw_max3(__builtin_fabsf(f.origin[0]), __builtin_fabsf(f.origin[1]), __builtin_fabsf(f.origin[2])) < 0x1p29f);
            // an origin that the bias made non-finite: its rays are not walked by a query either (ray_walkable) -- every ray a miss
        }
        const f3 org = F3(f.origin[0], f.origin[1], f.origin[2]);
        const bool origin_ok = __builtin_isfinite(org.x) && __builtin_isfinite(org.y) && __builtin_isfinite(org.z);

        uint32_t ref = RT_IDLE_REF, k = slot, cnt = 0u, sign_bits = 0u, octant4 = 0u;
        f3 dir = F3s(0.0f), inv = F3s(0.0f), sum = F3s(0.0f);
        bool pairs = false, hit = false;
        int sp = 0;

        // ray k of this lane's point: its direction and where its walk starts
        auto start = [&]()
        {
            float d[3];
            bake_direction(f, r1, r2, k, samples, d);
            dir = F3(d[0], d[1], d[2]);
            const float4 q = ray_inverse(dir);                                // trace_bvh.cl:125-129
            inv = F3(q.x, q.y, q.z);
            sign_bits = __float_as_uint(q.w) & 0xFFu;
            octant4 = 4u * (sign_bits & 7u);
            pairs = use_wide == 0u || (sign_bits & RT_SIGN_SLOW) != 0u || far_origin;
            hit = false;
            sp = 0;
            const bool walkable = origin_ok && __builtin_isfinite(dir.x) && __builtin_isfinite(dir.y) && __builtin_isfinite(dir.z) &&
                                  !(dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f);
            ref = walkable ? (pairs ? sc.entry_ref : sc.w_sh_entry_ref) : RT_IDLE_REF;
        };
        // a ray has ended: its verdict joins the lane's sum, and the lane's next ray starts
        auto finish = [&]()
        {
            if (!hit) { sum = sum + dir; ++cnt; }
            k += L;
        };
        if (f.walked)
        {
            start();
            while (ref == RT_IDLE_REF && k < samples) { finish(); if (k < samples) start(); }    // (rays that are not walked end at once)
        }
        else k = samples;

        auto push = [&](uint32_t r, float entry)
        {
            const uint2 e = make_uint2(r, __float_as_uint(entry));
            if (sp < RT_QUERY_STACK_LDS) stack[sp][lane] = e;
            else if (sp < RT_W4_STACK_MAX) my_spill[sp - RT_QUERY_STACK_LDS] = e;
            else { overflow = true; return; }
            ++sp;
        };
        auto pop = [&]()
        {
            ref = RT_IDLE_REF;
            while (sp > 0)
            {
                --sp;
                const uint2 e = sp < RT_QUERY_STACK_LDS ? stack[sp][lane] : spill_load64(my_spill + (sp - RT_QUERY_STACK_LDS));
                if (radius >= __uint_as_float(e.y)) { ref = e.x; break; }
            }
        };
        auto tested = [](uint32_t r) { return (int)r < -1 ? r | RT_LEAF_CONT_BIT : r; };

        while (__ballot(ref != RT_IDLE_REF) != 0ull)
        {
            if (ref != RT_IDLE_REF)
            {
                const bool at_leaf = (int)ref < -1;
                const uint32_t prim = ref & ~(RT_LEAF_BIT | RT_LEAF_CONT_BIT);
                const float4* rp = reinterpret_cast<const float4*>(at_leaf ? tri_base + ((size_t)prim << 6) : (pairs ? pair_base : wide_base) + ((size_t)ref << 6));
                const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
                if (at_leaf)
                {
                    bool inside = true;
                    if (!(ref & RT_LEAF_CONT_BIT))
                    {
                        float entry;
                        inside = box_test_fast(q1.w, q2.w, q3.x, q3.y, q3.z, q3.w, org, inv, 0.0f, radius, entry);
                    }
                    if (!inside) pop();
                    else
                    {
                        const bool last = q0.w != 0.0f;
                        float t = 0.0f, hu = 0.0f, hv = 0.0f;
                        const bool accepted = ray_triangle(org, dir, F3(q0.x, q0.y, q0.z), F3(q1.x, q1.y, q1.z), F3(q2.x, q2.y, q2.z), 0.0f, radius, hu, hv, t);
                        if (accepted) { hit = true; ref = RT_IDLE_REF; }         // goto endtrace, trace_bvh.cl:164-167
                        else if (last) pop();
                        else ref = (RT_LEAF_BIT | RT_LEAF_CONT_BIT) | (prim + 1u);
                    }
                }
                else if (pairs)
                {
                    const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y), axis = __float_as_uint(q3.z);
                    float a0, a1;
                    bool h0, h1;
                    if (sign_bits & RT_SIGN_SLOW)
                    {
                        h0 = box_test(RT_NODE_C0(q0, q1, q2), org, inv, 0.0f, radius, a0);
                        h1 = box_test(RT_NODE_C1(q0, q1, q2), org, inv, 0.0f, radius, a1);
                    }
                    else
                    {
                        h0 = box_test_fast(RT_NODE_C0(q0, q1, q2), org, inv, 0.0f, radius, a0);
                        h1 = box_test_fast(RT_NODE_C1(q0, q1, q2), org, inv, 0.0f, radius, a1);
                    }
                    h1 = h1 && c1 != RT_EMPTY_REF;
                    const bool swap = ((sign_bits >> axis) & 1u) != 0u;
                    const uint32_t near_ref = swap ? c1 : c0, far_ref = swap ? c0 : c1;
                    const bool near_hit = swap ? h1 : h0, far_hit = swap ? h0 : h1;
                    if (near_hit && far_hit) push(tested(far_ref), swap ? a0 : a1);
                    if (near_hit) ref = tested(near_ref);
                    else if (far_hit) ref = tested(far_ref);
                    else pop();
                }
                else
                {
                    uint32_t r[4];
                    float e[4];
                    w4_test_slots<true>(q0, q1, q2, q3, org, inv, sign_bits, octant4, 0.0f, radius, r, e);
                    const bool v0 = e[0] < INF, v1 = e[1] < INF, v2 = e[2] < INF, v3 = e[3] < INF;
                    if (v3 && (v0 || v1 || v2)) push(r[3], e[3]);
                    if (v2 && (v0 || v1)) push(r[2], e[2]);
                    if (v1 && v0) push(r[1], e[1]);
                    if (v0) ref = r[0];
                    else if (v1) ref = r[1];
                    else if (v2) ref = r[2];
                    else if (v3) ref = r[3];
                    else pop();
                }
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
    if (overflow) *status = 1u;                                  // pinned host memory, as k_query_trace's
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
