// within.hip -- every triangle within a radius of caller-supplied points (rt_scene_within / rt_scene_within_buffer / rt_debug_within / rt_debug_within_walk,
// DESIGN.md section 7l): the kernels (within_kernels.h), their host driver, and the host's brute force and walk over the same arithmetic (nearest.h, within.h).
// A translation unit and a code object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.
// -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "within_kernels.h"
#include "within_host.h"
#include "nearest_host.h"
#include "walk_host.h"

namespace within
{
static_assert(sizeof(rt_point) == sizeof(float4) && sizeof(rt_point_hits) == sizeof(float4) && sizeof(rt_nearest) == 2 * sizeof(float4) &&
    sizeof(rt_surface) == 4 * sizeof(float4), "records as 16-byte pieces");
// 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow fewer (DESIGN.md section 7l's table)
#define RT_WITHIN_LIST_WAVES_PER_CU 16u
#define RT_WITHIN_COUNT_WAVES_PER_CU 24u

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_point* d_points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* d_out, rt_nearest* d_near, rt_surface* d_surfaces)
{
    if (n == 0u) return true;
    // the records k_within_surface reads: the caller's, or the first 32 bytes of each surface record
    float4* near = (float4*)d_near;
    uint32_t near_stride = 2u;
    if (!near && d_surfaces) { near = (float4*)d_surfaces; near_stride = 4u; }
    // with nowhere to list members the counting walk answers both modes: stored = min(count, max_near), and a k-nearest count is its stored
    const bool list = max_near > 0u && near;
    const bool knn = list && (options & RT_WITHIN_K_NEAREST) != 0u;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, list ? RT_WITHIN_LIST_WAVES_PER_CU : RT_WITHIN_COUNT_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
#define RT_WITHIN_LAUNCH(WIDE, LIST, KNN) \
    hipLaunchKernelGGL((k_within<WIDE, LIST, KNN>), dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_points, n, max_near, options, (float4*)d_out, near, near_stride, \
        q.spill, q.status)
    if (use_wide)
    {
        if (knn) RT_WITHIN_LAUNCH(true, true, true);
        else if (list) RT_WITHIN_LAUNCH(true, true, false);
        else RT_WITHIN_LAUNCH(true, false, false);
    }
    else
    {
        if (knn) RT_WITHIN_LAUNCH(false, true, true);
        else if (list) RT_WITHIN_LAUNCH(false, true, false);
        else RT_WITHIN_LAUNCH(false, false, false);
    }
#undef RT_WITHIN_LAUNCH
    if (!dev::clean()) return false;
    if (d_surfaces && max_near > 0u)
    {
        const unsigned long long total = (unsigned long long)n * max_near;
        hipLaunchKernelGGL(k_within_surface, dim3(dev::blocks_for(total, 256u)), dim3(256), 0, stream, sc.tris_sh, n_tris, object_of_triangle,
            (const float4*)d_points, (const float4*)near, near_stride, max_near, total, (float4*)d_surfaces);
        if (!dev::clean()) return false;
    }
    return true;
}

// a point's outputs from what a pass over triangles kept of it
static void write_point(const rt_triangle* tris, const rt_point& pt, uint32_t count, const WnList& list, uint32_t max_near, uint32_t options, bool searched,
    rt_point_hits* out, rt_nearest* near)
{
    const uint32_t stored = count < max_near ? count : max_near, first = wn_list_first(max_near);
    float p1[3], p2[3], p3[3];
    for (uint32_t j = 0; j < max_near; ++j)
    {
        near[j] = nearest_none();
        if (j >= stored) continue;
        walk::triangle_corners(tris[list.prim[first + j]], p1, p2, p3);
        near[j] = nearest_record(pt.position, p1, p2, p3, list.prim[first + j]);
    }
    // the list keeps max(max_near, 1) members, so its first place names the nearest one also where none is listed
    *out = within_record(count, max_near, options, list.prim[first], searched);
}

void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near)
{
    walk::split_range(n, (uint64_t)n * n_tris, [&](uint32_t first, uint32_t end)
    {
        for (uint32_t i = first; i < end; ++i)
        {
            const float* p = points[i].position;
            const bool searched = nearest_searched(p, points[i].max_distance);
            uint32_t count = 0u;
            WnList list;
            wn_list_clear(list, max_near);
            if (searched)
            {
                const float r2 = points[i].max_distance * points[i].max_distance;
                float p1[3], p2[3], p3[3];
                for (uint32_t t = 0; t < n_tris; ++t)
                {
                    walk::triangle_corners(tris[t], p1, p2, p3);
                    const NpTriangle c = nearest_point_triangle(p, p1, p2, p3);
                    if (!within_member(c.d2, r2)) continue;
                    ++count;
                    wn_list_insert(list, c.d2, t);
                }
            }
            write_point(tris, points[i], count, list, max_near, options, searched, out + i, near + (size_t)i * max_near);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options,
    rt_point_hits* out, rt_nearest* near)
{
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_points = tmp.get(points, (size_t)n * sizeof(rt_point));
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_point_hits));
    void* const d_near = tmp.get(nullptr, (size_t)n * max_near * sizeof(rt_nearest));
    bool ok = d_tris && d_points && d_out && d_near;
    if (ok)
        hipLaunchKernelGGL(k_within_brute, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, (const rt_triangle*)d_tris, n_tris, (const float4*)d_points, n,
            max_near, options, (float4*)d_out, (float4*)d_near);
    ok = ok && dev::clean();
    if (ok && max_near > 0u) ok = hipMemcpyAsync(near, d_near, (size_t)n * max_near * sizeof(rt_nearest), hipMemcpyDeviceToHost, stream) == hipSuccess;
    return tmp.finish(ok, out, d_out, (size_t)n * sizeof(rt_point_hits));
}

const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, uint32_t* tested)
{
    // k_within<WIDE, true, KNN> on the host: the list is always kept here, so max_near == 0 answers nearest_primitive from its one place
    const bool knn = (options & RT_WITHIN_K_NEAREST) != 0u;
    std::vector<WnList> lists(n);
    std::vector<uint32_t> counts(n, 0u);
    for (uint32_t i = 0; i < n; ++i) wn_list_clear(lists[i], max_near);
    if (const char* why = nearest::walk_points(nodes, nn, tris, n_tris, wide, points, n, tested, [&](uint32_t i, uint32_t prim, const NpTriangle& t, float bound)
        {
            const float r2 = points[i].max_distance * points[i].max_distance;
            if (!within_member(t.d2, r2)) return bound;
            ++counts[i];
            wn_list_insert(lists[i], t.d2, prim);
            return knn ? within_knn_bound(lists[i], r2) : bound;
        }))
        return why;
    for (uint32_t i = 0; i < n; ++i)
        write_point(tris, points[i], counts[i], lists[i], max_near, options, nearest_searched(points[i].position, points[i].max_distance), out + i,
            near + (size_t)i * max_near);
    return nullptr;
}
} // namespace within
