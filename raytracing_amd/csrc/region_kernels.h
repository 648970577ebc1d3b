// region_kernels.h -- the kernels of an overlap query (rt_scene_overlap / rt_scene_overlap_buffer / rt_scene_select / rt_debug_overlap / rt_debug_select,
// DESIGN.md section 7m): for each CALLER-supplied convex region (up to 8 half-spaces) every triangle of the uploaded scene it touches or encloses.  The rule
// -- plane evaluation, classification, the box test, the list -- is region.h's.
//
//   k_region<WIDE, LIST>   one lane per region, 64-thread blocks: rt_region in (144 bytes), rt_region_hits out (16 bytes) and max_list rt_region_member (LIST)
//   k_region_brute         one lane per region over ALL triangles of an rt_triangle array (rt_debug_overlap's device form: region.h with no tree)
//   k_select               one lane per TRIANGLE against up to 32 regions: a bit per region in a word per triangle, ORed into a word per object
//   k_select_finish        one lane per object: object_inside from what k_select gathered
//
// The walk is walk_kernels.h's volume walk (persistent strided chunks of 64 regions, walk::Stack in the ray queries' spill area) with walk::region_box_step at
// a box record, which needs no key and no sort: a counting walk visits every passing child, and its pop always accepts.  The fetch and the leaf chain are
// written out here, word for word walk::volume_step's: on that step the LIST kernels measured 1.4 to 4 % slower at unchanged registers (DESIGN.md section
// 7m, "the volume walks on one step"), so this one loop stays until that is understood.  A rule changed in volume_step is changed here too.  The lane's planes live in LDS (walk::RegionLds, 8 KiB per block beside the stack's 6 KiB): a lane writes its
// own column at the chunk's start and reads only that, so there is no barrier.  A region that is not searched is never walked.
//
// LIST = false keeps `count` and `inside`.  LIST = true also keeps an RgList (region.h): 8 registers of ids, right-aligned, the flags not kept; after the
// walk a listed member's flags are made again by region_classify on the kept triangle's corners: the same function on the same operands, so the same bits.
#pragma once
#include "walk_kernels.h"
#include "region.h"

namespace region
{
RT_DEV void store_record(float4* o, const rt_region_hits& r)
{
    q_store(o, make_float4(__uint_as_float(r.count), __uint_as_float(r.inside), __uint_as_float(r.stored), __uint_as_float(r.flags)));
}

// a lane's region: the planes into its LDS column, num_planes returned -- 0 when the region is not searched (it is then not walked)
RT_DEV uint32_t load_region(const float4* __restrict__ g /* 9 pieces */, walk::RegionLds& planes)
{
    const uint32_t np = __float_as_uint(g[0].x);
    bool finite = true;
#pragma unroll
    for (uint32_t k = 0; k < RT_REGION_MAX_PLANES; ++k)
    {
        const float4 p = g[1u + k];
        planes[k][threadIdx.x] = p;
        if (k < np) finite = finite && __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z) && __builtin_isfinite(p.w);
    }
    return np >= 1u && np <= RT_REGION_MAX_PLANES && finite ? np : 0u;
}

// region_classify with the planes read from the lane's LDS column
RT_DEV uint32_t classify(const walk::RegionLds& planes, uint32_t np, const float (&p1)[3], const float (&p2)[3], const float (&p3)[3])
{
    uint32_t flags = 0u;
    bool rejected = false;
    for (uint32_t k = 0; k < np; ++k)
    {
        const float4 p4 = planes[k][threadIdx.x];
        const float pl[4] = {p4.x, p4.y, p4.z, p4.w};
        const uint32_t out = region_corners_outside(pl, p1, p2, p3);
        rejected = rejected || out == 3u;
        if (out != 0u) flags |= 1u << (RT_REGION_MEMBER_CROSSING_SHIFT + k);
    }
    if (rejected) return RT_REGION_REJECTED;
    return flags != 0u ? flags : RT_REGION_MEMBER_INSIDE;
}

template <bool WIDE, bool LIST>
__global__ __launch_bounds__(64) void k_region(DScene sc, const float4* __restrict__ regions, uint32_t n, uint32_t max_list, float4* __restrict__ out,
    uint2* __restrict__ members, uint2* __restrict__ spill, uint32_t* __restrict__ status)
{
    __shared__ walk::StackLds lds;
    __shared__ walk::RegionLds planes;
    walk::Stack stack(lds, spill);
    const uint32_t lane = threadIdx.x;
    const char* const node_base = reinterpret_cast<const char*>(WIDE ? sc.wnodes : sc.nodes);
    const char* const tri_base = reinterpret_cast<const char*>(sc.tris_sh);
    const float* const flag_base = reinterpret_cast<const float*>(sc.tris_rt);
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF, count = 0u, inside = 0u, np = 0u;
        RgList list;
        if (LIST) rg_list_clear(list, max_list);
        stack.sp = 0;
        if (i < n)
        {
            np = load_region(regions + (size_t)i * 9u, planes);
            if (np != 0u) ref = WIDE ? sc.w_entry_ref : sc.entry_ref;
        }

        while (__ballot(ref != RT_IDLE_REF) != 0ull)
        {
            if (ref != RT_IDLE_REF)
            {
                const bool at_leaf = (int)ref < -1;
                const uint32_t prim = ref & ~RT_LEAF_BIT;
                float last = 0.0f;
                if (at_leaf) last = flag_base[((size_t)prim << 4) + 3u];
                const float4* rp = reinterpret_cast<const float4*>(at_leaf ? tri_base + ((size_t)prim << 7) : node_base + ((size_t)ref << 6));
                const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
                if (at_leaf)
                {
                    const float p1[3] = {q0.x, q0.y, q0.z}, p2[3] = {q1.x, q1.y, q1.z}, p3[3] = {q2.x, q2.y, q2.z};
                    const uint32_t cls = classify(planes, np, p1, p2, p3);
                    if (cls != RT_REGION_REJECTED)
                    {
                        ++count;
                        inside += cls & RT_REGION_MEMBER_INSIDE;
                        if (LIST) rg_list_insert(list, prim);
                    }
                    if (last != 0.0f) ref = stack.pop([](float) { return true; });
                    else ref = RT_LEAF_BIT | (prim + 1u);
                }
                else walk::region_box_step<WIDE>(q0, q1, q2, q3, planes, np, ref, stack);
            }
        }

        if (i < n)
        {
            if (LIST)
            {
                // place t holds member t - first (region.h: the list is kept right-aligned)
                const uint32_t stored = count < max_list ? count : max_list, first = rg_list_first(max_list);
#pragma unroll
                for (uint32_t t = 0; t < RT_REGION_LIST_MAX; ++t)
                    if (t >= first)
                    {
                        const uint32_t j = t - first;
                        uint2 o = make_uint2(RT_INVALID_ID, 0u);
                        if (j < stored)
                        {
                            const uint32_t prim = list.key[t] - 1u;
                            const float4* tp = sc.tris_sh + (size_t)prim * 8;
                            const float4 a = tp[0], b = tp[1], c = tp[2];
                            const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
                            o = make_uint2(prim, classify(planes, np, p1, p2, p3));
                        }
                        members[(size_t)i * max_list + j] = o;
                    }
            }
            store_record(out + i, region_record(count, inside, max_list, np != 0u));
        }
    }
    stack.report(status);
}

// region.h over every triangle, no tree.  members may be nullptr when max_list == 0.
__global__ __launch_bounds__(64) void k_region_brute(const rt_triangle* __restrict__ tris, uint32_t n_tris, const float4* __restrict__ regions, uint32_t n,
    uint32_t max_list, float4* __restrict__ out, uint2* __restrict__ members)
{
    __shared__ walk::RegionLds planes;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t np = load_region(regions + (size_t)i * 9u, planes);
    uint32_t count = 0u, inside = 0u;
    RgList list;
    rg_list_clear(list, max_list);
    float p1[3], p2[3], p3[3];
    if (np != 0u)
        for (uint32_t t = 0; t < n_tris; ++t)
        {
            walk::triangle_corners(tris[t], p1, p2, p3);
            const uint32_t cls = classify(planes, np, p1, p2, p3);
            if (cls == RT_REGION_REJECTED) continue;
            ++count;
            inside += cls & RT_REGION_MEMBER_INSIDE;
            rg_list_insert(list, t);
        }
    const uint32_t stored = count < max_list ? count : max_list, first = rg_list_first(max_list);
#pragma unroll
    for (uint32_t t = 0; t < RT_REGION_LIST_MAX; ++t)
        if (t >= first)
        {
            const uint32_t j = t - first;
            if (j >= max_list) continue;
            uint2 o = make_uint2(RT_INVALID_ID, 0u);
            if (j < stored)
            {
                const uint32_t prim = list.key[t] - 1u;
                walk::triangle_corners(tris[prim], p1, p2, p3);
                o = make_uint2(prim, classify(planes, np, p1, p2, p3));
            }
            members[(size_t)i * max_list + j] = o;
        }
    store_record(out + i, region_record(count, inside, max_list, np != 0u));
}

// the OR of v over the wave's active lanes, in every lane
RT_DEV uint32_t wave_or(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// One lane per triangle, every region against it: the regions are the same for all lanes, so their planes come through scalar loads.  corners: the shading
// records (stride 8 pieces) or an rt_triangle array (stride 10 pieces, positions at pieces 0, 3, 6).  The per-object words: object_touching ORs the touching
// bits; object_outside ORs the bits of the searched regions a triangle is NOT inside and object_has marks an object with a triangle -- k_select_finish
// makes object_inside of the two.  All three are zeroed before the launch.  A wave whose lanes all belong to one object ORs once.
__global__ __launch_bounds__(256) void k_select(const float4* __restrict__ corners, uint32_t stride, uint32_t second, uint32_t third, uint32_t n_tris,
    const uint32_t* __restrict__ object_of_triangle, const rt_region* __restrict__ regions, uint32_t n, uint32_t* __restrict__ touching, uint32_t* __restrict__ inside,
    uint32_t* __restrict__ object_touching, uint32_t* __restrict__ object_outside, uint32_t* __restrict__ object_has)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool live = t < n_tris;
    uint32_t touch = 0u, in = 0u;
    if (live)
    {
        const float4* tp = corners + (size_t)t * stride;
        const float4 a = tp[0], b = tp[second], c = tp[third];
        const float p1[3] = {a.x, a.y, a.z}, p2[3] = {b.x, b.y, b.z}, p3[3] = {c.x, c.y, c.z};
        for (uint32_t r = 0; r < n; ++r)
        {
            const uint32_t np = regions[r].num_planes;
            if (!region_searched(np, &regions[r].planes[0][0])) continue;
            const uint32_t cls = region_classify(np, &regions[r].planes[0][0], p1, p2, p3);
            if (cls == RT_REGION_REJECTED) continue;
            touch |= 1u << r;
            if (cls & RT_REGION_MEMBER_INSIDE) in |= 1u << r;
        }
        if (touching) touching[t] = touch;
        if (inside) inside[t] = in;
    }
    if (!object_of_triangle) return;
    const uint32_t object = live ? object_of_triangle[t] : RT_INVALID_ID;
    const uint32_t outside = ~in;
    const uint32_t leader = __builtin_amdgcn_readfirstlane(object);
    if (__ballot(object != leader) == 0ull)
    {
        // Every lane of the wave is live here, or none is.  The invariant this rests on: an object index is below n_objects <= 0xFFFFFFFE (rt_scene_set_objects
        // and rt_debug_select refuse an index that is not below num_objects, a uint32_t), so RT_INVALID_ID = 0xFFFFFFFF is no object's index, a dead lane
        // differs from a live leader, and a wave of dead lanes alone has the leader RT_INVALID_ID, which is tested below.  object_has is written with plain
        // stores of the one value 1 (here and in the other branch): whichever lane's store lands last, the word is 1.
        const uint32_t all_touch = wave_or(touch), all_out = wave_or(outside);
        if (leader != RT_INVALID_ID && (threadIdx.x & 63u) == 0u)
        {
            if (object_touching && all_touch != 0u) atomicOr(object_touching + leader, all_touch);
            if (object_outside) { atomicOr(object_outside + leader, all_out); object_has[leader] = 1u; }
        }
    }
    else if (live)
    {
        if (object_touching && touch != 0u) atomicOr(object_touching + object, touch);
        if (object_outside) { atomicOr(object_outside + object, outside); object_has[object] = 1u; }
    }
}

// object_inside[o] (in place of the gathered object_outside[o]): every triangle of the object inside, and at least one triangle
__global__ __launch_bounds__(256) void k_select_finish(uint32_t* __restrict__ object_inside, const uint32_t* __restrict__ object_has, uint32_t n_objects)
{
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= n_objects) return;
    object_inside[o] = object_has[o] != 0u ? ~object_inside[o] : 0u;
}
} // namespace region
