// region.hip -- every triangle a caller's convex region touches or encloses (rt_scene_overlap / rt_scene_overlap_buffer / rt_scene_select / rt_frame_pick_rect /
// rt_debug_overlap / rt_debug_overlap_walk / rt_debug_select): the kernels (region_kernels.h), their host driver, and the host's brute
// force and walk over the same rule (region.h).  A translation unit and a code object of its own so that the hot path's code object (rt_hip.hip,
// codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "region_kernels.h"
#include "region_host.h"
#include "walk_host.h"

namespace region
{
static_assert(sizeof(rt_region) == 9 * sizeof(float4) && sizeof(rt_region_hits) == sizeof(float4) && sizeof(rt_region_member) == sizeof(uint2) &&
    sizeof(rt_triangle) == 10 * sizeof(float4), "records as 16-byte pieces");
// 14 KiB of LDS per block (the stack's 6 and the planes' 8): 11 fit a CU's 160 KiB, fewer than the registers would allow (DESIGN.md section 7m's table)
#define RT_REGION_WAVES_PER_CU 11u

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_region* d_regions, uint32_t n, uint32_t max_list,
    rt_region_hits* d_out, rt_region_member* d_members)
{
    if (n == 0u) return true;
    const bool list = max_list > 0u && d_members;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, RT_REGION_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
#define RT_REGION_LAUNCH(WIDE, LIST) \
    hipLaunchKernelGGL((k_region<WIDE, LIST>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_regions, n, max_list, (float4*)d_out, (uint2*)d_members, q.spill, q.status)
    if (use_wide) { if (list) RT_REGION_LAUNCH(true, true); else RT_REGION_LAUNCH(true, false); }
    else { if (list) RT_REGION_LAUNCH(false, true); else RT_REGION_LAUNCH(false, false); }
#undef RT_REGION_LAUNCH
    return dev::clean();
}

// k_select and its finishing step over `corners`; d_has: a word per object
static bool select_launch(hipStream_t stream, const float4* corners, uint32_t stride, uint32_t second, uint32_t third, uint32_t n_tris, const uint32_t* d_ids,
    uint32_t n_objects, const rt_region* d_regions, uint32_t n, uint32_t* d_touching, uint32_t* d_inside, uint32_t* d_object_touching, uint32_t* d_object_inside,
    uint32_t* d_has)
{
    const bool objects = d_ids && (d_object_touching || d_object_inside);
    if (objects && d_object_touching && hipMemsetAsync(d_object_touching, 0, (size_t)n_objects * 4u, stream) != hipSuccess) return false;
    if (objects && d_object_inside &&
        (hipMemsetAsync(d_object_inside, 0, (size_t)n_objects * 4u, stream) != hipSuccess || hipMemsetAsync(d_has, 0, (size_t)n_objects * 4u, stream) != hipSuccess))
        return false;
    if (n_tris > 0u)
    {
        hipLaunchKernelGGL(k_select, dim3(dev::blocks_for(n_tris, 256u)), dim3(256), 0, stream, corners, stride, second, third, n_tris, objects ? d_ids : nullptr, d_regions, n,
            d_touching, d_inside, objects ? d_object_touching : nullptr, objects ? d_object_inside : nullptr, d_has);
        if (!dev::clean()) return false;
    }
    if (objects && d_object_inside)
    {
        hipLaunchKernelGGL(k_select_finish, dim3(dev::blocks_for(n_objects, 256u)), dim3(256), 0, stream, d_object_inside, (const uint32_t*)d_has, n_objects);
        if (!dev::clean()) return false;
    }
    return true;
}

bool select(hipStream_t stream, query::Scratch& q, const DScene& sc, uint32_t n_tris, const uint32_t* d_object_of_triangle, uint32_t n_objects,
    const rt_region* d_regions, uint32_t n, uint32_t* d_touching, uint32_t* d_inside, uint32_t* d_object_touching, uint32_t* d_object_inside)
{
    uint32_t* has = nullptr;
    if (d_object_of_triangle && d_object_inside)
    {
        if (!query::reserve(stream, q, 3, (size_t)n_objects * 4u)) return false;
        has = (uint32_t*)q.stage[3];
    }
    return select_launch(stream, sc.tris_sh, 8u, 1u, 2u, n_tris, d_object_of_triangle, n_objects, d_regions, n, d_touching, d_inside, d_object_touching, d_object_inside, has);
}

// a region's outputs from what a pass over triangles kept of it
static void write_region(const rt_triangle* tris, const rt_region& g, uint32_t count, uint32_t inside, const RgList& list, uint32_t max_list, bool searched,
    rt_region_hits* out, rt_region_member* members)
{
    const uint32_t stored = count < max_list ? count : max_list, first = rg_list_first(max_list);
    float p1[3], p2[3], p3[3];
    for (uint32_t j = 0; j < max_list; ++j)
    {
        members[j].primitive_id = RT_INVALID_ID; members[j].flags = 0u;
        if (j >= stored) continue;
        const uint32_t prim = list.key[first + j] - 1u;
        walk::triangle_corners(tris[prim], p1, p2, p3);
        members[j].primitive_id = prim;
        members[j].flags = region_classify(g.num_planes, &g.planes[0][0], p1, p2, p3);
    }
    *out = region_record(count, inside, max_list, searched);
}

void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members)
{
    walk::split_range(n, (uint64_t)n * n_tris, [&](uint32_t first, uint32_t end)
    {
        for (uint32_t i = first; i < end; ++i)
        {
            const rt_region& g = regions[i];
            const bool searched = region_searched(g.num_planes, &g.planes[0][0]);
            uint32_t count = 0u, inside = 0u;
            RgList list;
            rg_list_clear(list, max_list);
            float p1[3], p2[3], p3[3];
            if (searched)
                for (uint32_t t = 0; t < n_tris; ++t)
                {
                    walk::triangle_corners(tris[t], p1, p2, p3);
                    const uint32_t cls = region_classify(g.num_planes, &g.planes[0][0], p1, p2, p3);
                    if (cls == RT_REGION_REJECTED) continue;
                    ++count;
                    inside += cls & RT_REGION_MEMBER_INSIDE;
                    rg_list_insert(list, t);
                }
            write_region(tris, g, count, inside, list, max_list, searched, out + i, members + (size_t)i * max_list);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out,
    rt_region_member* members)
{
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_regions = tmp.get(regions, (size_t)n * sizeof(rt_region));
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_region_hits));
    void* const d_members = tmp.get(nullptr, (size_t)n * max_list * sizeof(rt_region_member));
    bool ok = d_tris && d_regions && d_out && d_members;
    if (ok)
        hipLaunchKernelGGL(k_region_brute, dim3(dev::blocks_for(n, 64u)), dim3(64), 0, stream, (const rt_triangle*)d_tris, n_tris, (const float4*)d_regions, n, max_list,
            (float4*)d_out, (uint2*)d_members);
    ok = ok && dev::clean();
    if (ok && max_list > 0u) ok = hipMemcpyAsync(members, d_members, (size_t)n * max_list * sizeof(rt_region_member), hipMemcpyDeviceToHost, stream) == hipSuccess;
    return tmp.finish(ok, out, d_out, (size_t)n * sizeof(rt_region_hits));
}

const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_region* regions, uint32_t n,
    uint32_t max_list, rt_region_hits* out, rt_region_member* members, uint32_t* tested)
{
    walk::HostTree tree;
    if (const char* why = tree.prepare(nodes, nn, n_tris, wide)) return why;

    for (uint32_t i = 0; i < n; ++i)
    {
        const rt_region& g = regions[i];
        const float* planes = &g.planes[0][0];
        const bool searched = region_searched(g.num_planes, planes);
        uint32_t count = 0u, inside = 0u, visited = 0u;
        RgList list;
        rg_list_clear(list, max_list);
        auto box_passes = [&](const float (&lo)[3], const float (&hi)[3])
        {
            for (uint32_t k = 0; k < g.num_planes; ++k) if (region_plane_rejects_box(planes + 4u * k, lo, hi)) return false;
            return true;
        };
        uint32_t stack[RT_W4_STACK_MAX];
        int sp = 0;
        uint32_t ref = searched ? tree.entry(box_passes) : RT_IDLE_REF;
        float p1[3], p2[3], p3[3];
        while (ref != RT_IDLE_REF)
        {
            if ((int)ref < -1)
            {
                const uint32_t prim = ref & ~RT_LEAF_BIT;
                if (prim >= n_tris) return "a leaf reference lies outside the triangle array";
                walk::triangle_corners(tris[prim], p1, p2, p3);
                const uint32_t cls = region_classify(g.num_planes, planes, p1, p2, p3);
                ++visited;
                if (cls != RT_REGION_REJECTED)
                {
                    ++count;
                    inside += cls & RT_REGION_MEMBER_INSIDE;
                    rg_list_insert(list, prim);
                }
                if (tree.last[prim]) ref = sp > 0 ? stack[--sp] : RT_IDLE_REF;
                else ref = RT_LEAF_BIT | (prim + 1u);
                continue;
            }
            uint32_t r[4];
            float lo[4][3], hi[4][3];
            if (const char* why = tree.slots(ref, r, lo, hi)) return why;
            bool pass[4];
            for (int k = 0; k < 4; ++k) pass[k] = r[k] != RT_EMPTY_REF && box_passes(lo[k], hi[k]);
            // walk::region_box_step: every passing slot but one is pushed, that one is visited next
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
        write_region(tris, g, count, inside, list, max_list, searched, out + i, members + (size_t)i * max_list);
    }
    return nullptr;
}

void select_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* ids, uint32_t n_objects, const rt_region* regions, uint32_t n, uint32_t* touching,
    uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    std::vector<uint32_t> outside(ids ? n_objects : 0u, 0u), has(ids ? n_objects : 0u, 0u);
    if (ids && object_touching) for (uint32_t o = 0; o < n_objects; ++o) object_touching[o] = 0u;
    float p1[3], p2[3], p3[3];
    for (uint32_t t = 0; t < n_tris; ++t)
    {
        walk::triangle_corners(tris[t], p1, p2, p3);
        uint32_t touch = 0u, in = 0u;
        for (uint32_t r = 0; r < n; ++r)
        {
            if (!region_searched(regions[r].num_planes, &regions[r].planes[0][0])) continue;
            const uint32_t cls = region_classify(regions[r].num_planes, &regions[r].planes[0][0], p1, p2, p3);
            if (cls == RT_REGION_REJECTED) continue;
            touch |= 1u << r;
            if (cls & RT_REGION_MEMBER_INSIDE) in |= 1u << r;
        }
        touching[t] = touch; inside[t] = in;
        if (!ids) continue;
        if (object_touching) object_touching[ids[t]] |= touch;
        outside[ids[t]] |= ~in; has[ids[t]] = 1u;
    }
    if (ids && object_inside) for (uint32_t o = 0; o < n_objects; ++o) object_inside[o] = has[o] ? ~outside[o] : 0u;
}

bool select_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* ids, uint32_t n_objects, const rt_region* regions, uint32_t n,
    uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_regions = tmp.get(regions, (size_t)n * sizeof(rt_region));
    uint32_t* const d_touching = (uint32_t*)tmp.get(nullptr, (size_t)n_tris * 4u);
    uint32_t* const d_inside = (uint32_t*)tmp.get(nullptr, (size_t)n_tris * 4u);
    bool ok = d_tris && d_regions && d_touching && d_inside;
    uint32_t *d_ids = nullptr, *d_ot = nullptr, *d_oi = nullptr, *d_has = nullptr;
    if (ok && ids)
    {
        d_ids = (uint32_t*)tmp.get(ids, (size_t)n_tris * 4u);
        d_ot = (uint32_t*)tmp.get(nullptr, (size_t)n_objects * 4u);
        d_oi = (uint32_t*)tmp.get(nullptr, (size_t)n_objects * 4u);
        d_has = (uint32_t*)tmp.get(nullptr, (size_t)n_objects * 4u);
        ok = d_ids && d_ot && d_oi && d_has;
    }
    ok = ok && select_launch(stream, (const float4*)d_tris, 10u, 3u, 6u, n_tris, d_ids, n_objects, (const rt_region*)d_regions, n, d_touching, d_inside, d_ot, d_oi, d_has);
    if (ok && n_tris > 0u) ok = hipMemcpyAsync(inside, d_inside, (size_t)n_tris * 4u, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (ok && ids && object_touching) ok = hipMemcpyAsync(object_touching, d_ot, (size_t)n_objects * 4u, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (ok && ids && object_inside) ok = hipMemcpyAsync(object_inside, d_oi, (size_t)n_objects * 4u, hipMemcpyDeviceToHost, stream) == hipSuccess;
    return tmp.finish(ok, touching, d_touching, (size_t)n_tris * 4u);
}

const char* rect_refused(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (x1 < x0 || y1 < y0) return "an empty rectangle (x1 < x0 or y1 < y0)";
    if (x1 >= width || y1 >= height) return "the rectangle is outside the image";
    return nullptr;
}

rt_region rect_region(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far)
{
    return region_of_rect(cam, width, height, x0, y0, x1, y1, t_near, t_far);
}
} // namespace region
