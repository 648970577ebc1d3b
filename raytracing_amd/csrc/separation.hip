// separation.hip -- the nearest scene triangle to a caller's triangle, and a scene's clearances (rt_scene_separation / rt_scene_separation_buffer /
// rt_scene_separation_self / rt_scene_separation_self_buffer / rt_debug_separation / rt_debug_separation_walk / rt_debug_separation_self, DESIGN.md section
// 7o): the kernels (separation_kernels.h), their host driver, and the host's brute force and walk over the same rule (separation.h).  A translation unit and
// a code object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include "rt_hip.h"
#include "separation_kernels.h"
#include "separation_host.h"
#include "walk_host.h"

namespace separation
{
static_assert(sizeof(rt_probe) == 3 * sizeof(float4) && sizeof(rt_separation) == 3 * sizeof(float4) && sizeof(rt_triangle) == 10 * sizeof(float4),
    "records as 16-byte pieces");
// 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers (226 VGPRs) allow 2 waves per SIMD (DESIGN.md section 7o's table)
#define RT_SEPARATION_WAVES_PER_CU 8u

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_probe* d_probes, uint32_t n, float max_distance,
    rt_separation* d_out)
{
    if (n == 0u) return true;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, RT_SEPARATION_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
    if (use_wide)
        hipLaunchKernelGGL((k_separation<true, false>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_probes, (const uint32_t*)nullptr, 0u, n, max_distance,
            (float4*)d_out, q.spill, q.status);
    else
        hipLaunchKernelGGL((k_separation<false, false>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_probes, (const uint32_t*)nullptr, 0u, n, max_distance,
            (float4*)d_out, q.spill, q.status);
    return dev::clean();
}

bool launch_self(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const uint32_t* d_object_of_triangle, uint32_t first,
    uint32_t n, float max_distance, uint32_t options, rt_separation* d_out)
{
    if (n == 0u) return true;
    const uint32_t* const ids = (options & RT_SEPARATION_OTHER_OBJECTS) != 0u ? d_object_of_triangle : nullptr;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, RT_SEPARATION_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
    if (use_wide)
        hipLaunchKernelGGL((k_separation<true, true>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)nullptr, ids, first, n, max_distance, (float4*)d_out,
            q.spill, q.status);
    else
        hipLaunchKernelGGL((k_separation<false, true>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)nullptr, ids, first, n, max_distance, (float4*)d_out,
            q.spill, q.status);
    return dev::clean();
}

// probe i of a host form: a caller's, or (probes == nullptr) triangle first + i
static void host_probe(const rt_triangle* tris, const rt_probe* probes, uint32_t first, uint32_t i, CrossProbe& q)
{
    if (probes) { cross_probe_make(q, probes[i].p1, probes[i].p2, probes[i].p3); return; }
    float p1[3], p2[3], p3[3];
    walk::triangle_corners(tris[first + i], p1, p2, p3);
    cross_probe_make(q, p1, p2, p3);
}

// a probe's record from the triangle a pass kept of it
static rt_separation host_record(const rt_triangle* tris, const CrossProbe& q, bool searched, uint32_t best_prim)
{
    if (best_prim == RT_INVALID_ID) return sep_none(searched);
    float p1[3], p2[3], p3[3];
    walk::triangle_corners(tris[best_prim], p1, p2, p3);
    return sep_record(q, p1, p2, p3, best_prim);
}

void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, float max_distance, uint32_t options,
    rt_separation* out)
{
    const bool self = probes == nullptr;
    if (!(options & RT_SEPARATION_OTHER_OBJECTS)) ids = nullptr;
    walk::split_range(n, (uint64_t)n * n_tris, [&](uint32_t begin, uint32_t end)
    {
        for (uint32_t i = begin; i < end; ++i)
        {
            CrossProbe q;
            host_probe(tris, probes, first, i, q);
            const bool searched = sep_searched(q, max_distance);
            float best = max_distance * max_distance;
            uint32_t best_prim = RT_INVALID_ID;
            float p1[3], p2[3], p3[3];
            if (searched)
                for (uint32_t t = 0; t < n_tris; ++t)
                {
                    walk::triangle_corners(tris[t], p1, p2, p3);
                    if (self && (t == first + i || cross_shares_corner(q, p1, p2, p3) || (ids && ids[t] == ids[first + i]))) continue;
                    if (!sep_maybe_nearer(q, p1, p2, p3, best)) continue;
                    const float d2 = sep_pair(q, p1, p2, p3).d2;
                    if (nearest_accepts(d2, t, best, best_prim)) { best = d2; best_prim = t; }
                }
            out[i] = host_record(tris, q, searched, best_prim);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n,
    float max_distance, uint32_t options, rt_separation* out)
{
    if (!(options & RT_SEPARATION_OTHER_OBJECTS)) ids = nullptr;
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_probes = probes ? tmp.get(probes, (size_t)n * sizeof(rt_probe)) : nullptr;
    void* const d_ids = ids ? tmp.get(ids, (size_t)n_tris * sizeof(uint32_t)) : nullptr;
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_separation));
    bool ok = d_tris && (d_probes || !probes) && (d_ids || !ids) && d_out;
    if (ok)
        hipLaunchKernelGGL(k_separation_brute, dim3(dev::blocks_for(n, 64u)), dim3(64), 0, stream, (const rt_triangle*)d_tris, n_tris, (const float4*)d_probes,
            (const uint32_t*)d_ids, first, n, max_distance, (float4*)d_out);
    return tmp.finish(ok && dev::clean(), out, d_out, (size_t)n * sizeof(rt_separation));
}

const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_probe* probes, uint32_t n,
    float max_distance, rt_separation* out, uint32_t* tested)
{
    walk::HostTree tree;
    if (const char* why = tree.prepare(nodes, nn, n_tris, wide)) return why;
    const float INF = __builtin_inff();

    for (uint32_t i = 0; i < n; ++i)
    {
        CrossProbe q;
        host_probe(tris, probes, 0u, i, q);
        const bool searched = sep_searched(q, max_distance);
        float best = max_distance * max_distance;
        uint32_t best_prim = RT_INVALID_ID, visited = 0u;
        struct Entry { uint32_t ref; float d2; } stack[RT_W4_STACK_MAX];
        int sp = 0;
        uint32_t ref = RT_IDLE_REF;
        if (searched) ref = tree.entry([&](const float (&lo)[3], const float (&hi)[3]) { return !(sep_box_d2(q.lo, q.hi, lo, hi) > best); });
        auto pop = [&]()
        {
            ref = RT_IDLE_REF;
            while (sp > 0)
            {
                --sp;
                if (!(stack[sp].d2 > best)) { ref = stack[sp].ref; break; }
            }
        };
        float p1[3], p2[3], p3[3];
        while (ref != RT_IDLE_REF)
        {
            if ((int)ref < -1)
            {
                const uint32_t prim = ref & ~RT_LEAF_BIT;
                if (prim >= n_tris) return "a leaf reference lies outside the triangle array";
                walk::triangle_corners(tris[prim], p1, p2, p3);
                ++visited;
                if (sep_maybe_nearer(q, p1, p2, p3, best))
                {
                    const float d2 = sep_pair(q, p1, p2, p3).d2;
                    if (nearest_accepts(d2, prim, best, best_prim)) { best = d2; best_prim = prim; }
                }
                if (tree.last[prim]) pop();
                else ref = RT_LEAF_BIT | (prim + 1u);
                continue;
            }
            uint32_t r[4];
            float lo[4][3], hi[4][3], e[4];
            if (const char* why = tree.slots(ref, r, lo, hi)) return why;
            // walk::probe_box_step
            for (int k = 0; k < 4; ++k)
            {
                e[k] = r[k] != RT_EMPTY_REF ? sep_box_d2(q.lo, q.hi, lo[k], hi[k]) : INF;
                if (r[k] == RT_EMPTY_REF || e[k] > best) { r[k] = RT_EMPTY_REF; e[k] = INF; }
            }
            auto exchange = [&](int a, int b)
            {
                if (e[b] < e[a]) { const float te = e[a]; e[a] = e[b]; e[b] = te; const uint32_t tr = r[a]; r[a] = r[b]; r[b] = tr; }
            };
            exchange(0, 1); exchange(2, 3); exchange(0, 2); exchange(1, 3); exchange(1, 2);
            uint32_t next = RT_IDLE_REF;
            float next_e = 0.0f;
            for (int k = 3; k >= 0; --k)
                if (r[k] != RT_EMPTY_REF)
                {
                    if (next != RT_IDLE_REF)
                    {
                        if (sp >= RT_W4_STACK_MAX) return "the tree is deeper than the walk's stack";
                        stack[sp].ref = next; stack[sp].d2 = next_e; ++sp;
                    }
                    next = r[k]; next_e = e[k];
                }
            if (next != RT_IDLE_REF) ref = next;
            else pop();
        }
        if (tested) tested[i] = visited;
        out[i] = host_record(tris, q, searched, best_prim);
    }
    return nullptr;
}
} // namespace separation
