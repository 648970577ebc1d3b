// light_bake_kernels.h -- the kernels of a light bake (rt_scene_light_bake / rt_scene_light_bake_buffer / rt_scene_atlas_bake_light / rt_debug_light_bake_rays,
// DESIGN.md section 7s): per CALLER-supplied point a hemisphere of any-hit rays that look the environment up where they escape, and one any-hit ray per
// analytic light of the scene, generated, walked and reduced on the device.  The arithmetic is light_bake.h's.
//
//   k_bake_light       one wave per group of points, 64-thread blocks: a point record in (32 or 64 bytes), rt_light_bake_result (32 bytes) out
//   k_light_bake_rays  one lane per item: the rays k_bake_light would walk, written out as rt_ray (rt_debug_light_bake_rays's device form)
//
// Mapping: k_bake's (bake_kernels.h).  L = min(samples, 64) lanes own one point, a wave owns 64 / L points; the persistent grid strides over such groups.
// Lane l of a point is its reduction slot l: it makes and walks items l, l + L, l + 2 L, ... of the point's samples + M itself, in this order -- the sky rays
// first, then the lights' -- and starts its next item the moment a ray ends; no result depends on which lane ends when.  An item that makes no ray
// (a light below the horizon, a disabled half) ends at once.
//
// The walk is k_bake's: walk_kernels.h's ray_setup, ray_entry<true>, ray_step<true> and Stack (LDS plus spill, an overrun raises *status), with the item's own
// t_max -- sky_distance, or 1 for the segment to a point light.
//
// finish().  A sky ray that met nothing looks the environment up there and then (light_bake_sky: the fp64 atan2 / acos of rt_detmath.h and four float4 gathers,
// paid by unoccluded sky rays only) and adds it to the lane's sky sum; a light's ray that met nothing adds the E its item computed when it started.
//
// Reduction.  The two counts: per bit of a lane's count one ballot, masked to the point's lanes and popcounted.  The six sums: bake.h's halving tree with
// __shfl_down inside the point's L lanes.
#pragma once
#include "walk_kernels.h"
#include "light_bake.h"

namespace light_bake
{
__global__ __launch_bounds__(64) void k_bake_light(DScene sc, const float4* __restrict__ points, uint32_t n, uint32_t first_index, uint32_t samples,
    uint32_t seed, uint32_t flags, float bias, float sky_distance, float4* __restrict__ out, uint2* __restrict__ spill, uint32_t use_wide,
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
    const uint32_t from_surfaces = flags & RT_BAKE_FROM_SURFACES;
    const uint32_t stride = from_surfaces ? 4u : 2u;             // float4 per point record
    const uint32_t items = samples + sc.light_count;
    const uint32_t lane_items_max = items / L + 1u;              // no lane handles more items than this: the bits its counts need

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
                const uint32_t sflags = __float_as_uint(rec[3].w);
                record_ok = (sflags & QS_FLAG_HIT) != 0u;
                if (sflags & QS_FLAG_BACK_FACE) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
            }
            f = bake_frame(pos, nrm, record_ok, bias);
            bake_rotations(first_index + (uint32_t)p, seed, &r1, &r2);
        }
        const f3 org = F3(f.origin[0], f.origin[1], f.origin[2]);
        const bool origin_ok = __builtin_isfinite(org.x) && __builtin_isfinite(org.y) && __builtin_isfinite(org.z);

        uint32_t ref = RT_IDLE_REF, k = slot, cnt_sky = 0u, cnt_lights = 0u;
        walk::Ray ray = walk::ray_idle();
        f3 sky = F3s(0.0f), lit = F3s(0.0f), E = F3s(0.0f);
        float t_far = 0.0f;
        bool hit = false, made = false;

        // item k of this lane's point: its ray, if it makes one, and where that ray's walk starts
        auto start = [&]()
        {
            LightBakeItem it;
            if (k < samples) it = light_bake_sky_item(f, r1, r2, k, samples, flags, sky_distance);
            else
            {
                const float4* l = sc.lights + (size_t)(k - samples) * 3u;
                const float4 lo4 = l[0], lr4 = l[1];
                const float lo[3] = {lo4.x, lo4.y, lo4.z}, lr[3] = {lr4.x, lr4.y, lr4.z};
                it = light_bake_light_item(f, lo, lr, __float_as_uint(l[2].x), flags, sky_distance);
            }
            made = it.made;
            E = F3(it.E[0], it.E[1], it.E[2]);
            t_far = it.t_max;
            ray = walk::ray_setup(org, F3(it.dir[0], it.dir[1], it.dir[2]), use_wide);
            hit = false;
            stack.sp = 0;
            const bool walkable = made && origin_ok && __builtin_isfinite(it.dir[0]) && __builtin_isfinite(it.dir[1]) && __builtin_isfinite(it.dir[2]) &&
                                  !(it.dir[0] == 0.0f && it.dir[1] == 0.0f && it.dir[2] == 0.0f);
            ref = walkable ? walk::ray_entry<true>(sc, ray) : RT_IDLE_REF;
        };
        // an item has ended: what its ray found joins the lane's sums, and the lane's next item starts
        auto finish = [&]()
        {
            const bool adds = made && !hit, is_sky = k < samples;
            if (adds && is_sky)
            {
                const float d[3] = {ray.dir.x, ray.dir.y, ray.dir.z};
                float rgb[3];
                light_bake_sky(sc.env, sc.env_w, sc.env_h, d, rgb);
                sky = F3(sky.x + rgb[0], sky.y + rgb[1], sky.z + rgb[2]);
            }
            if (adds && !is_sky) lit = F3(lit.x + E.x, lit.y + E.y, lit.z + E.z);
            cnt_sky += adds && is_sky ? 1u : 0u;               // (two selects: as two branches' increments the counts became an indexed pair in scratch)
            cnt_lights += adds && !is_sky ? 1u : 0u;
            k += L;
        };
        if (f.walked)
        {
            start();
            while (ref == RT_IDLE_REF && k < items) { finish(); if (k < items) start(); }       // (items without a walk end at once)
        }
        else k = items;

        while (__ballot(ref != RT_IDLE_REF) != 0ull)
        {
            if (ref != RT_IDLE_REF)
            {
                float t_max = t_far, hit_u = 0.0f, hit_v = 0.0f;              // the step's own copies: only its verdict is kept
                uint32_t hit_prim = RT_INVALID_ID;
                if (walk::ray_step<true>(sc, ray, 0.0f, t_max, ref, stack, hit_u, hit_v, hit_prim)) hit = true;
                if (ref == RT_IDLE_REF)                                       // this lane's ray ended in this pass: the refill
                {
                    finish();
                    if (k < items) start();
                    while (ref == RT_IDLE_REF && k < items) { finish(); if (k < items) start(); }
                }
            }
        }

        // the whole wave is here: the counts and the sums of each of its points
        uint32_t sky_unoccluded = 0u, lights_unshadowed = 0u;
        for (uint32_t bit = 0; (lane_items_max >> bit) != 0u; ++bit)
        {
            sky_unoccluded += (uint32_t)__popcll(__ballot(((cnt_sky >> bit) & 1u) != 0u) & seg_mask) << bit;
            lights_unshadowed += (uint32_t)__popcll(__ballot(((cnt_lights >> bit) & 1u) != 0u) & seg_mask) << bit;
        }
        for (uint32_t s = L >> 1; s > 0u; s >>= 1)
        {
            const float sx = __shfl_down(sky.x, s, (int)L), sy = __shfl_down(sky.y, s, (int)L), sz = __shfl_down(sky.z, s, (int)L);
            const float lx = __shfl_down(lit.x, s, (int)L), ly = __shfl_down(lit.y, s, (int)L), lz = __shfl_down(lit.z, s, (int)L);
            sky = F3(sky.x + sx, sky.y + sy, sky.z + sz);
            lit = F3(lit.x + lx, lit.y + ly, lit.z + lz);
        }
        if (slot == 0u && p < n)
        {
            const float S[3] = {sky.x, sky.y, sky.z};
            float irr[3];
            light_bake_finish(S, samples, irr);
            const float none = __uint_as_float(RT_INVALID_ID);
            out[2 * p] = f.walked ? make_float4(irr[0], irr[1], irr[2], __uint_as_float(sky_unoccluded)) : make_float4(0.0f, 0.0f, 0.0f, none);
            out[2 * p + 1] = f.walked ? make_float4(lit.x, lit.y, lit.z, __uint_as_float(lights_unshadowed)) : make_float4(0.0f, 0.0f, 0.0f, none);
        }
    }
    stack.report(status);
}

// rays[p * (samples + num_lights) + r] = the ray of item r of point p as k_bake_light walks it; all zeros for an item without a ray and for a skipped point.
// lights: 3 x float4 per light (origin, radiance, type bits), an rt_light's layout and DScene's
__global__ __launch_bounds__(256) void k_light_bake_rays(const float4* __restrict__ points, uint32_t n, uint32_t first_index, uint32_t samples, uint32_t seed,
    uint32_t flags, float bias, float sky_distance, const float4* __restrict__ lights, uint32_t num_lights, float4* __restrict__ rays)
{
    const unsigned long long items = (unsigned long long)samples + num_lights;
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned long long)n * items) return;
    const uint32_t p = (uint32_t)(idx / items), r = (uint32_t)(idx % items);
    const bool from_surfaces = (flags & RT_BAKE_FROM_SURFACES) != 0u;
    const float* rec = reinterpret_cast<const float*>(points + (size_t)p * (from_surfaces ? 4u : 2u));
    float pos[3], nrm[3];
    const bool record_ok = bake_point(rec, from_surfaces, pos, nrm);
    const BakeFrame f = bake_frame(pos, nrm, record_ok, bias);
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = o;
    if (f.walked)
    {
        LightBakeItem it;
        if (r < samples)
        {
            float r1, r2;
            bake_rotations(first_index + p, seed, &r1, &r2);
            it = light_bake_sky_item(f, r1, r2, r, samples, flags, sky_distance);
        }
        else
        {
            const float4* l = lights + (size_t)(r - samples) * 3u;
            const float4 lo4 = l[0], lr4 = l[1];
            const float lo[3] = {lo4.x, lo4.y, lo4.z}, lr[3] = {lr4.x, lr4.y, lr4.z};
            it = light_bake_light_item(f, lo, lr, __float_as_uint(l[2].x), flags, sky_distance);
        }
        if (it.made)
        {
            o = make_float4(f.origin[0], f.origin[1], f.origin[2], 0.0f);
            d = make_float4(it.dir[0], it.dir[1], it.dir[2], it.t_max);
        }
    }
    rays[2 * idx] = o;
    rays[2 * idx + 1] = d;
}
} // namespace light_bake
