// nearest.hip -- the nearest surface point to caller-supplied points (rt_scene_nearest / rt_scene_nearest_buffer / rt_debug_nearest / rt_debug_nearest_walk,
// DESIGN.md section 7j): the kernels (nearest_kernels.h), their host driver, and the host's brute force and walk over the same arithmetic (nearest.h).  A
// translation unit and a code object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.
// -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <functional>
#include "rt_hip.h"
#include "nearest_kernels.h"
#include "nearest_host.h"
#include "walk_host.h"

namespace nearest
{
static_assert(sizeof(rt_point) == sizeof(float4) && sizeof(rt_nearest) == 2 * sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4), "records as 16-byte pieces");
#define RT_NEAREST_WAVES_PER_CU 24u     // 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow 24

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_point* d_points, uint32_t n, rt_nearest* d_out, rt_surface* d_surfaces)
{
    if (n == 0u) return true;
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, RT_NEAREST_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
    // the records k_nearest_surface reads: the caller's, or the first 32 bytes of each surface record
    float4* found = (float4*)d_out;
    uint32_t found_stride = 2u;
    if (!found) { found = (float4*)d_surfaces; found_stride = 4u; }
    if (use_wide)
        hipLaunchKernelGGL(k_nearest<true>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_points, n, found, found_stride, q.spill, q.status);
    else
        hipLaunchKernelGGL(k_nearest<false>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_points, n, found, found_stride, q.spill, q.status);
    if (!dev::clean()) return false;
    if (d_surfaces)
    {
        hipLaunchKernelGGL(k_nearest_surface, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, sc.tris_sh, n_tris, object_of_triangle,
            (const float4*)d_points, (const float4*)found, found_stride, n, (float4*)d_surfaces);
        if (!dev::clean()) return false;
    }
    return true;
}

void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, rt_nearest* out)
{
    walk::split_range(n, (uint64_t)n * n_tris, [&](uint32_t first, uint32_t end)
    {
        for (uint32_t i = first; i < end; ++i)
        {
            const float* p = points[i].position;
            out[i] = nearest_none();
            if (!nearest_searched(p, points[i].max_distance)) continue;
            float best = points[i].max_distance * points[i].max_distance;
            uint32_t best_prim = RT_INVALID_ID;
            float p1[3], p2[3], p3[3];
            for (uint32_t t = 0; t < n_tris; ++t)
            {
                walk::triangle_corners(tris[t], p1, p2, p3);
                const NpTriangle c = nearest_point_triangle(p, p1, p2, p3);
                if (nearest_accepts(c.d2, t, best, best_prim)) { best = c.d2; best_prim = t; }
            }
            if (best_prim == RT_INVALID_ID) continue;
            walk::triangle_corners(tris[best_prim], p1, p2, p3);
            out[i] = nearest_record(p, p1, p2, p3, best_prim);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, rt_nearest* out)
{
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_points = tmp.get(points, (size_t)n * sizeof(rt_point));
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_nearest));
    const bool ok = d_tris && d_points && d_out;
    if (ok)
        hipLaunchKernelGGL(k_nearest_brute, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, (const rt_triangle*)d_tris, n_tris, (const float4*)d_points, n,
            (float4*)d_out);
    return tmp.finish(ok && dev::clean(), out, d_out, (size_t)n * sizeof(rt_nearest));
}

const char* walk_points(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    uint32_t* tested, const std::function<float(uint32_t, uint32_t, const NpTriangle&, float)>& triangle)
{
    walk::HostTree tree;
    if (const char* why = tree.prepare(nodes, nn, n_tris, wide)) return why;
    const float INF = __builtin_inff();

    for (uint32_t i = 0; i < n; ++i)
    {
        const float* p = points[i].position;
        if (tested) tested[i] = 0u;
        if (!nearest_searched(p, points[i].max_distance)) continue;
        float best = points[i].max_distance * points[i].max_distance;          // the bound that prunes
        uint32_t count = 0u;
        struct Entry { uint32_t ref; float d2; } stack[RT_W4_STACK_MAX];
        int sp = 0;
        uint32_t ref = tree.entry([&](const float (&lo)[3], const float (&hi)[3]) { return !(nearest_box_d2(p, lo, hi) > best); });
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
                const NpTriangle t = nearest_point_triangle(p, p1, p2, p3);
                ++count;
                best = triangle(i, prim, t, best);
                if (tree.last[prim]) pop();
                else ref = RT_LEAF_BIT | (prim + 1u);
                continue;
            }
            uint32_t r[4];
            float lo[4][3], hi[4][3], e[4];
            if (const char* why = tree.slots(ref, r, lo, hi)) return why;
            for (int k = 0; k < 4; ++k)
            {
                e[k] = r[k] != RT_EMPTY_REF ? nearest_box_d2(p, lo[k], hi[k]) : INF;
                if (e[k] > best) { r[k] = RT_EMPTY_REF; e[k] = INF; }
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
        if (tested) tested[i] = count;
    }
    return nullptr;
}

const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    rt_nearest* out, uint32_t* tested)
{
    std::vector<uint32_t> best_prim(n, RT_INVALID_ID);
    if (const char* why = walk_points(nodes, nn, tris, n_tris, wide, points, n, tested, [&](uint32_t i, uint32_t prim, const NpTriangle& t, float best)
        {
            if (!nearest_accepts(t.d2, prim, best, best_prim[i])) return best;
            best_prim[i] = prim;
            return t.d2;
        }))
        return why;
    float p1[3], p2[3], p3[3];
    for (uint32_t i = 0; i < n; ++i)
    {
        out[i] = nearest_none();
        if (best_prim[i] == RT_INVALID_ID) continue;
        walk::triangle_corners(tris[best_prim[i]], p1, p2, p3);
        out[i] = nearest_record(points[i].position, p1, p2, p3, best_prim[i]);
    }
    return nullptr;
}
} // namespace nearest
