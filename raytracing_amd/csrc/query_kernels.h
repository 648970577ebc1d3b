// query_kernels.h -- the kernels of a ray query (rt_scene_trace / rt_scene_trace_buffer / rt_frame_pick): CALLER-supplied rays against the
// uploaded scene's trees.
//
//   k_query_trace<ANY_HIT>   one lane per ray, 64-thread blocks: rt_ray in (32 bytes, two dwordx4), rt_hit (16 bytes) or one dword out
//   k_query_surface<RECORDS> one lane per ray: rt_surface (64 bytes) from the hit and the triangle's 128-byte shading record (query.h's arithmetic)
//
// Why the frame's walks are not borrowed: v1_trace_ray, k_trace2 and w4_trace_body fix t_min = 0, take rays in the queues' layout (o4.w = t_max, d4.w = a path
// id) and live on the frame's persistent queues, radiance log and slow lists.  A caller's rt_ray carries its own t_min (trace_bvh.cl:148 honours it), so the
// loops below are this kernel's own; the tests they are made of -- box_test, box_test_fast, w4_test_slots, ray_triangle -- are trace_kernels.h's, which take a t_min.
//
// The walk.  A lane's ray is at a reference: a 4-wide record, a child-pair record, or a triangle of a leaf.  Every pass of the one loop fetches the lane's next
// 64-byte record -- the same four 16-byte loads whichever kind -- and takes its step (the shape of w4_trace_body's loop D: one memory round trip per step):
//   * a ray the wide walk can take walks the 4-wide records: w4_test_slots' conservative slab tests with the ray's t_min, slots in the record's order table
//     (closest) or in stored order (any-hit); the first passing slot is visited next, the later ones wait on the stack with their entry distances; a leaf is
//     re-tested with its exact BVH2 bounds and the current t_max when it is reached and its triangles are tested in array order; an accepted hit lowers t_max
//     (trace_bvh.cl:157-162).  Per ray that is w4_trace_body's sequence of nodes, leaves and t_max, which is the reference's (trace_kernels.h, "Exactness"):
//     t_min only enters the two max(..., t_min) and the accept rule, and the pop-time re-test t_max >= entry stays equivalent to the full box test.
//   * RT_SIGN_SLOW rays (a non-finite or huge 1/dir component), rays from beyond 2^29, and every ray when the scene has no 4-wide tree (RT_CTX_OPT_WIDE_BVH = 0,
//     a tree that does not qualify) walk the exact child-pair records: trace_bvh.cl's loop, both children box-tested at their parent (select-form box_test for
//     the slow rays), near child first by the split axis, the far child pushed with its entry distance.  A leaf reached this way has had its exact box tested
//     at its parent, so it arrives with RT_LEAF_CONT_BIT set and shares the leaf step.  Any-hit slow rays walk this (the reference's) tree: any tree over the
//     reference's leaves gives the reference's verdict.
//   * a ray with a non-finite component or an all-zero direction is not walked: a miss.
//
// Stack: RT_QUERY_STACK_LDS entries of (ref, entry distance) per lane in LDS, the rest in the lane's slice of a spill area, RT_W4_STACK_MAX entries in all -- the
// bound k_trace_w4 has with its argument (at most three pending slots per wide level, at most 33 levels: build_wide_bvh refuses deeper folds), which also covers
// the child-pair walk's RT_TRACE_STACK_MAX = 64 (one pending child per level; the reference's own nodesToVisit[64], trace_bvh.cl:142).  A push beyond it is not
// written; it raises *status, which rt_scene_trace and rt_finish report -- never a silent limit, never a store out of bounds.
//
// Grid: persistent-style, blocks = min(ceil(n / 64), what is resident); block b takes chunks b, b + blocks, ... of 64 consecutive rays and finishes a chunk
// before it takes the next (no refill of single lanes: a query has no queue counters or work heads to share).  So the spill area is sized by the grid, not by n.
#pragma once
#include "trace_kernels.h"
#include "query.h"

#define RT_QUERY_STACK_LDS 12
#define RT_QUERY_SPILL_PER_LANE (RT_W4_STACK_MAX - RT_QUERY_STACK_LDS)
static_assert(RT_W4_STACK_MAX >= RT_TRACE_STACK_MAX, "the one stack serves both walks");

namespace query
{
// a ray that is walked: every component finite and a direction that is not all zeros
RT_DEV bool ray_walkable(const float4 o, const float4 d)
{
    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) && __builtin_isfinite(o.w) &&
                        __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z) && __builtin_isfinite(d.w);
    return finite && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

template <bool ANY_HIT>
__global__ __launch_bounds__(64) void k_query_trace(DScene sc, const float4* __restrict__ rays, uint32_t n, float4* __restrict__ hits, uint32_t hit_stride /* in float4 */,
    uint32_t* __restrict__ occluded, uint2* __restrict__ spill, uint32_t use_wide, uint32_t* __restrict__ status)
{
    __shared__ uint2 stack[RT_QUERY_STACK_LDS][64];
    const uint32_t lane = threadIdx.x;
    uint2* const my_spill = spill + (size_t)(blockIdx.x * 64u + lane) * RT_QUERY_SPILL_PER_LANE;
    const char* const wide_base = reinterpret_cast<const char*>(ANY_HIT ? sc.wnodes_sh : sc.wnodes);
    const char* const pair_base = reinterpret_cast<const char*>(sc.nodes);
    const char* const tri_base = reinterpret_cast<const char*>(sc.tris_rt);
    const uint32_t wide_entry = ANY_HIT ? sc.w_sh_entry_ref : sc.w_entry_ref;
    const float INF = __builtin_inff();
    const uint32_t n_chunks = (n >> 6) + ((n & 63u) != 0u ? 1u : 0u);          // (n + 63 would wrap above 2^32 - 64)
    bool overflow = false;

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
    {
        const uint32_t i = chunk * 64u + lane;
        uint32_t ref = RT_IDLE_REF;
        f3 org = F3s(0.0f), dir = F3s(0.0f), inv = F3s(0.0f);
        float t_min = 0.0f, t_max = 0.0f, hit_u = 0.0f, hit_v = 0.0f;
        uint32_t sign_bits = 0, octant4 = 0, hit_prim = RT_INVALID_ID;
        bool pairs = false, walked = false;                   // pairs: this ray walks the child-pair records
        int sp = 0;
        if (i < n)
        {
            const float4 q0 = q_load(rays + 2 * (size_t)i), q1 = q_load(rays + 2 * (size_t)i + 1);
            walked = ray_walkable(q0, q1);
            if (walked)
            {
                org = F3(q0.x, q0.y, q0.z); t_min = q0.w;
                dir = F3(q1.x, q1.y, q1.z); t_max = q1.w;
                const float4 q2 = ray_inverse(dir);                          // trace_bvh.cl:125-129
                inv = F3(q2.x, q2.y, q2.z);
                sign_bits = __float_as_uint(q2.w) & 0xFFu;
                octant4 = 4u * (sign_bits & 7u);
                pairs = use_wide == 0u || (sign_bits & RT_SIGN_SLOW) != 0u ||
                        !(hw_max3(__builtin_fabsf(org.x), __builtin_fabsf(org.y), __builtin_fabsf(org.z)) < 0x1p29f);
                ref = pairs ? sc.entry_ref : wide_entry;
            }
        }

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
                if (t_max >= __uint_as_float(e.y)) { ref = e.x; break; }     // the box re-test at pop time (wide entries: conservative, a pre-cull)
            }
        };
        // a child-pair walk tests a leaf's exact box at its parent: the leaf step must not test it again
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
                        // the reference's RayBounds on the leaf node (trace_bvh.cl:146-148) with the current t_max
                        float entry;
                        inside = box_test_fast(q1.w, q2.w, q3.x, q3.y, q3.z, q3.w, org, inv, t_min, t_max, entry);
                    }
                    if (!inside) pop();
                    else
                    {
                        const bool last = q0.w != 0.0f;
                        float t = 0.0f;
                        const bool accepted = ray_triangle(org, dir, F3(q0.x, q0.y, q0.z), F3(q1.x, q1.y, q1.z), F3(q2.x, q2.y, q2.z), t_min, t_max, hit_u, hit_v, t);
                        if (accepted) { hit_prim = prim; t_max = t; }            // trace_bvh.cl:159-162
                        if (ANY_HIT && accepted) ref = RT_IDLE_REF;              // goto endtrace, :164-167
                        else if (last) pop();
                        else ref = (RT_LEAF_BIT | RT_LEAF_CONT_BIT) | (prim + 1u);
                    }
                }
                else if (pairs)
                {
                    // one interior node of the reference's tree: both children's exact boxes (trace_bvh.cl:146-148), near child first (:181-190)
                    const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y), axis = __float_as_uint(q3.z);
                    float a0, a1;
                    bool h0, h1;
                    if (sign_bits & RT_SIGN_SLOW)
                    {
                        h0 = box_test(RT_NODE_C0(q0, q1, q2), org, inv, t_min, t_max, a0);
                        h1 = box_test(RT_NODE_C1(q0, q1, q2), org, inv, t_min, t_max, a1);
                    }
                    else
                    {
                        h0 = box_test_fast(RT_NODE_C0(q0, q1, q2), org, inv, t_min, t_max, a0);
                        h1 = box_test_fast(RT_NODE_C1(q0, q1, q2), org, inv, t_min, t_max, a1);
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
                    w4_test_slots<ANY_HIT>(q0, q1, q2, q3, org, inv, sign_bits, octant4, t_min, t_max, r, e);
                    // the first passing position is visited next, the later ones wait on the stack (deepest first)
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
            }
        }

        if (i < n)
        {
            if (hits)
                q_store(hits + (size_t)i * hit_stride, walked ? make_float4(hit_u, hit_v, __uint_as_float(hit_prim), t_max)
                                                              : make_float4(0.0f, 0.0f, __uint_as_float(RT_INVALID_ID), 0.0f));
            if (occluded) occluded[i] = hit_prim != RT_INVALID_ID ? 1u : 0u;
        }
    }
    if (overflow) *status = 1u;                                  // pinned host memory: the host reads it after it has waited for the stream
}

// RECORDS: `tris` = the scene's 128-byte shading records (p1 uv1.x | p2 uv1.y | p3 uv2.x | n1 uv2.y | n2 uv3.x | n3 uv3.y | mtl_index ...); otherwise rt_triangle[]
// (rt_debug_query_surface: they stand in for the records).  hits[i * hit_stride] may be the first 16 bytes of out[i] itself (a query that returns surfaces only
// keeps its hits there): lane i reads it before it writes.
template <bool RECORDS>
__global__ __launch_bounds__(256) void k_query_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ rays, const float4* hits, uint32_t hit_stride, uint32_t n, float4* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 hit = hits[(size_t)i * hit_stride];
    const uint32_t prim = __float_as_uint(hit.z);
    rt_surface s = qs_miss();
    if (prim < n_tris)                                           // RT_INVALID_ID (a miss) is above every count
    {
        QsTriangle t;
        if (RECORDS)
        {
            const float4* tp = tris + (size_t)prim * 8;
            const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2], q3 = tp[3], q4 = tp[4], q5 = tp[5], q6 = tp[6];
            t.p1[0] = q0.x; t.p1[1] = q0.y; t.p1[2] = q0.z; t.p2[0] = q1.x; t.p2[1] = q1.y; t.p2[2] = q1.z; t.p3[0] = q2.x; t.p3[1] = q2.y; t.p3[2] = q2.z;
            t.n1[0] = q3.x; t.n1[1] = q3.y; t.n1[2] = q3.z; t.n2[0] = q4.x; t.n2[1] = q4.y; t.n2[2] = q4.z; t.n3[0] = q5.x; t.n3[1] = q5.y; t.n3[2] = q5.z;
            t.uv1[0] = q0.w; t.uv1[1] = q1.w; t.uv2[0] = q2.w; t.uv2[1] = q3.w; t.uv3[0] = q4.w; t.uv3[1] = q5.w;
            t.mtl_index = __float_as_uint(q6.x);
        }
        else
            t = qs_triangle(reinterpret_cast<const rt_triangle*>(tris)[prim]);
        const float4 rd = rays[2 * (size_t)i + 1];
        const float d[3] = {rd.x, rd.y, rd.z};
        s = query_surface(t, d, hit.x, hit.y, hit.w, prim, object_of_triangle ? object_of_triangle[prim] : RT_INVALID_ID);
    }
    float4* o = out + (size_t)i * 4;
    o[0] = make_float4(s.position[0], s.position[1], s.position[2], __uint_as_float(s.primitive_id));
    o[1] = make_float4(s.geometric_normal[0], s.geometric_normal[1], s.geometric_normal[2], __uint_as_float(s.mtl_index));
    o[2] = make_float4(s.shading_normal[0], s.shading_normal[1], s.shading_normal[2], __uint_as_float(s.object));
    o[3] = make_float4(s.texcoord[0], s.texcoord[1], s.t, __uint_as_float(s.flags));
}
} // namespace query
