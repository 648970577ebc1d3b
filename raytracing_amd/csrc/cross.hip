// cross.hip -- every scene triangle a caller's triangle crosses, and a scene's self-crossings (rt_scene_cross / rt_scene_cross_buffer / rt_scene_cross_self /
// rt_scene_cross_self_buffer / rt_debug_cross / rt_debug_cross_walk / rt_debug_cross_self): the kernels (cross_kernels.h), their host
// driver, and the host's brute force and walk over the same rule (cross.h).  A translation unit and a code object of its own so that the hot path's code
// object (rt_hip.hip, codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "cross_kernels.h"
#include "cross_host.h"
#include "walk_host.h"

namespace cross
{
static_assert(sizeof(rt_probe) == 3 * sizeof(float4) && sizeof(rt_probe_hits) == sizeof(float4) && sizeof(rt_cross_member) == 2 * sizeof(float4) &&
    sizeof(rt_triangle) == 10 * sizeof(float4), "records as 16-byte pieces");
// 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow 4 waves per SIMD where no list is kept and 3 where one is (DESIGN.md section 7n's table)
#define RT_CROSS_COUNT_WAVES_PER_CU 16u
#define RT_CROSS_LIST_WAVES_PER_CU 12u

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_probe* d_probes, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* d_out, rt_cross_member* d_members)
{
    if (n == 0u) return true;
    const bool any = (options & RT_CROSS_ANY) != 0u, list = !any && max_list > 0u && d_members;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, list ? RT_CROSS_LIST_WAVES_PER_CU : RT_CROSS_COUNT_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
#define RT_CROSS_LAUNCH(WIDE, LIST, ANY) \
    hipLaunchKernelGGL((k_cross<WIDE, LIST, ANY>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_probes, n, max_list, (float4*)d_out, (float4*)d_members, q.spill, q.status)
    if (use_wide) { if (any) RT_CROSS_LAUNCH(true, false, true); else if (list) RT_CROSS_LAUNCH(true, true, false); else RT_CROSS_LAUNCH(true, false, false); }
    else { if (any) RT_CROSS_LAUNCH(false, false, true); else if (list) RT_CROSS_LAUNCH(false, true, false); else RT_CROSS_LAUNCH(false, false, false); }
#undef RT_CROSS_LAUNCH
    return dev::clean();
}

bool launch_self(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const uint32_t* d_object_of_triangle, uint32_t first,
    uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* d_out, rt_cross_member* d_members)
{
    if (n == 0u) return true;
    const uint32_t any = (options & RT_CROSS_ANY) != 0u ? 1u : 0u;
    const bool list = any == 0u && max_list > 0u && d_members;
    const uint32_t* const ids = (options & RT_CROSS_OTHER_OBJECTS) != 0u ? d_object_of_triangle : nullptr;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, list ? RT_CROSS_LIST_WAVES_PER_CU : RT_CROSS_COUNT_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
#define RT_CROSS_LAUNCH(WIDE, LIST) \
    hipLaunchKernelGGL((k_cross_self<WIDE, LIST>), dim3(blocks), dim3(64), 0, stream, sc, ids, first, n, max_list, any, (float4*)d_out, (float4*)d_members, q.spill, q.status)
    if (use_wide) { if (list) RT_CROSS_LAUNCH(true, true); else RT_CROSS_LAUNCH(true, false); }
    else { if (list) RT_CROSS_LAUNCH(false, true); else RT_CROSS_LAUNCH(false, false); }
#undef RT_CROSS_LAUNCH
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

// a probe's outputs from what a pass over triangles kept of it
static void write_probe(const rt_triangle* tris, const CrossProbe& q, uint32_t count, uint32_t lowest, const RgList& list, uint32_t max_list, bool any,
    rt_probe_hits* out, rt_cross_member* members)
{
    *out = cross_record(count, lowest, max_list, q.searched, any);
    const uint32_t place = rg_list_first(max_list);
    float p1[3], p2[3], p3[3];
    if (members)
        for (uint32_t j = 0; j < max_list; ++j)
        {
            rt_cross_member& m = members[j];
            m.primitive_id = RT_INVALID_ID; m.flags = 0u;
            for (int a = 0; a < 3; ++a) m.c0[a] = m.c1[a] = 0.0f;
            if (j >= out->stored) continue;
            const uint32_t prim = list.key[place + j] - 1u;
            walk::triangle_corners(tris[prim], p1, p2, p3);
            m.primitive_id = prim;
            m.flags = cross_pair(q, p1, p2, p3, m.c0, m.c1);
        }
}

void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options,
    rt_probe_hits* out, rt_cross_member* members)
{
    const bool any = (options & RT_CROSS_ANY) != 0u, self = probes == nullptr;
    if (!(options & RT_CROSS_OTHER_OBJECTS)) ids = nullptr;
    walk::split_range(n, (uint64_t)n * n_tris, [&](uint32_t begin, uint32_t end)
    {
        for (uint32_t i = begin; i < end; ++i)
        {
            CrossProbe q;
            host_probe(tris, probes, first, i, q);
            uint32_t count = 0u, lowest = RT_INVALID_ID;
            RgList list;
            rg_list_clear(list, max_list);
            float p1[3], p2[3], p3[3];
            if (q.searched)
                for (uint32_t t = 0; t < n_tris && !(any && count != 0u); ++t)
                {
                    walk::triangle_corners(tris[t], p1, p2, p3);
                    if (self && (t == first + i || cross_shares_corner(q, p1, p2, p3) || (ids && ids[t] == ids[first + i]))) continue;
                    if (!cross_test(q, p1, p2, p3)) continue;
                    ++count;
                    lowest = t < lowest ? t : lowest;
                    rg_list_insert(list, t);
                }
            write_probe(tris, q, count, lowest, list, max_list, any, out + i, members ? members + (size_t)i * max_list : nullptr);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (!(options & RT_CROSS_OTHER_OBJECTS)) ids = nullptr;
    // members == NULL happens only where nothing is listed (max_list == 0 or RT_CROSS_ANY: rt_debug_cross and rt_debug_cross_self refuse every other
    // NULL), and there `stored` is 0 whatever max_list says (cross_record), so the record does not change with this
    if (!members) max_list = 0u;
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_probes = probes ? tmp.get(probes, (size_t)n * sizeof(rt_probe)) : nullptr;
    void* const d_ids = ids ? tmp.get(ids, (size_t)n_tris * sizeof(uint32_t)) : nullptr;
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_probe_hits));
    void* const d_members = tmp.get(nullptr, (size_t)n * max_list * sizeof(rt_cross_member));
    bool ok = d_tris && (d_probes || !probes) && (d_ids || !ids) && d_out && d_members;
    if (ok)
        hipLaunchKernelGGL(k_cross_brute, dim3(dev::blocks_for(n, 64u)), dim3(64), 0, stream, (const rt_triangle*)d_tris, n_tris, (const float4*)d_probes,
            (const uint32_t*)d_ids, first, n, max_list, (options & RT_CROSS_ANY) != 0u ? 1u : 0u, (float4*)d_out, (float4*)d_members);
    ok = ok && dev::clean();
    if (ok && max_list > 0u) ok = hipMemcpyAsync(members, d_members, (size_t)n * max_list * sizeof(rt_cross_member), hipMemcpyDeviceToHost, stream) == hipSuccess;
    return tmp.finish(ok, out, d_out, (size_t)n * sizeof(rt_probe_hits));
}

const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_probe* probes, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* out, rt_cross_member* members, uint32_t* tested)
{
    walk::HostTree tree;
    if (const char* why = tree.prepare(nodes, nn, n_tris, wide)) return why;
    const bool any = (options & RT_CROSS_ANY) != 0u;

    for (uint32_t i = 0; i < n; ++i)
    {
        CrossProbe q;
        host_probe(tris, probes, 0u, i, q);
        uint32_t count = 0u, lowest = RT_INVALID_ID, visited = 0u;
        RgList list;
        rg_list_clear(list, max_list);
        // walk::cross_box_step's two tests
        auto box_passes = [&](const float (&lo)[3], const float (&hi)[3])
        {
            return cross_boxes_overlap(q.lo, q.hi, lo, hi) && !(q.plane && cross_planes_reject_box(q.pl, lo, hi));
        };
        uint32_t stack[RT_W4_STACK_MAX];
        int sp = 0;
        uint32_t ref = q.searched ? tree.entry(box_passes) : RT_IDLE_REF;
        float p1[3], p2[3], p3[3];
        while (ref != RT_IDLE_REF)
        {
            if ((int)ref < -1)
            {
                const uint32_t prim = ref & ~RT_LEAF_BIT;
                if (prim >= n_tris) return "a leaf reference lies outside the triangle array";
                walk::triangle_corners(tris[prim], p1, p2, p3);
                ++visited;
                if (cross_test(q, p1, p2, p3))
                {
                    ++count;
                    lowest = prim < lowest ? prim : lowest;
                    rg_list_insert(list, prim);
                }
                if (any && count != 0u) ref = RT_IDLE_REF;
                else if (tree.last[prim]) ref = sp > 0 ? stack[--sp] : RT_IDLE_REF;
                else ref = RT_LEAF_BIT | (prim + 1u);
                continue;
            }
            uint32_t r[4];
            float lo[4][3], hi[4][3];
            if (const char* why = tree.slots(ref, r, lo, hi)) return why;
            bool pass[4];
            for (int k = 0; k < 4; ++k) pass[k] = r[k] != RT_EMPTY_REF && box_passes(lo[k], hi[k]);
            // walk::cross_box_step: every passing slot but one is pushed, that one is visited next
            uint32_t next = RT_IDLE_REF;
            for (int k = 3; k >= 0; --k)
                if (pass[k])
                {
                    if (next != RT_IDLE_REF)
                    {
                        if (sp >= RT_W4_STACK_MAX) return "the tree is deeper than the walk's stack";
                        stack[sp++] = next;
                    }
                    next = r[k];
                }
            if (next != RT_IDLE_REF) ref = next;
            else ref = sp > 0 ? stack[--sp] : RT_IDLE_REF;
        }
        if (tested) tested[i] = visited;
        write_probe(tris, q, count, lowest, list, max_list, any, out + i, members ? members + (size_t)i * max_list : nullptr);
    }
    return nullptr;
}
} // namespace cross
