// all_hits.hip -- every surface a caller's ray crosses (rt_scene_trace_all / rt_scene_trace_all_buffer / rt_frame_pick_all / rt_debug_trace_all, DESIGN.md
// section 7k): the kernels (all_hits_kernels.h), their host driver, and the host's brute force over the same arithmetic (all_hits.h).  A translation unit and a
// code object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "all_hits_kernels.h"
#include "all_hits_host.h"
#include "walk_host.h"

namespace all_hits
{
static_assert(sizeof(rt_ray) == 2 * sizeof(float4) && sizeof(rt_hit) == sizeof(float4) && sizeof(rt_ray_hits) == sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4),
    "records as 16-byte pieces");
// 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow 16 waves per CU with the list (109 VGPRs) and 24 of the 28 without (67)
#define RT_ALL_HITS_LIST_WAVES_PER_CU 16u
#define RT_ALL_HITS_COUNT_WAVES_PER_CU 24u

bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_ray* d_rays, uint32_t n, uint32_t max_hits, rt_ray_hits* d_out, rt_hit* d_hits, rt_surface* d_surfaces)
{
    if (n == 0u) return true;
    // the hits k_all_hits_surface reads: the caller's, or the first 16 bytes of each surface record
    float4* hits = (float4*)d_hits;
    uint32_t hit_stride = 1u;
    if (!hits && d_surfaces) { hits = (float4*)d_surfaces; hit_stride = 4u; }
    const uint32_t blocks = query::prepare(stream, q, &q.status, compute_units, max_hits > 0u && hits ? RT_ALL_HITS_LIST_WAVES_PER_CU : RT_ALL_HITS_COUNT_WAVES_PER_CU,
        dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
    if (max_hits > 0u && hits)
        hipLaunchKernelGGL(k_all_hits<true>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_rays, n, max_hits, (float4*)d_out, hits, hit_stride, q.spill,
            use_wide ? 1u : 0u, q.status);
    else
        hipLaunchKernelGGL(k_all_hits<false>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_rays, n, max_hits, (float4*)d_out, (float4*)nullptr, 1u, q.spill,
            use_wide ? 1u : 0u, q.status);
    if (!dev::clean()) return false;
    if (d_surfaces && max_hits > 0u)
    {
        const unsigned long long total = (unsigned long long)n * max_hits;
        hipLaunchKernelGGL(k_all_hits_surface, dim3(dev::blocks_for(total, 256u)), dim3(256), 0, stream, sc.tris_sh, n_tris, object_of_triangle,
            (const float4*)d_rays, (const float4*)hits, hit_stride, max_hits, total, (float4*)d_surfaces);
        if (!dev::clean()) return false;
    }
    return true;
}

const char* leaves_refused(const rt_bvh_node* nodes, uint32_t nn, uint32_t n_tris)
{
    for (uint32_t k = 0; k < nn; ++k)
    {
        const uint32_t np = nodes[k].num_primitives_axis >> 16;
        if (np > 0u && (uint64_t)nodes[k].offset + np > n_tris) return "a leaf's triangles lie outside the array";
    }
    return nullptr;
}

void brute_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits)
{
    auto corners = [&](uint32_t prim, float (&p1)[3], float (&e1)[3], float (&e2)[3])
    {
        float p2[3], p3[3];
        walk::triangle_corners(tris[prim], p1, p2, p3);
        for (int a = 0; a < 3; ++a) { e1[a] = p2[a] - p1[a]; e2[a] = p3[a] - p1[a]; }
    };
    // the work: (ray, node) pairs
    walk::split_range(n, (uint64_t)n * nn, [&](uint32_t first, uint32_t end)
    {
        for (uint32_t i = first; i < end; ++i)
        {
            const float o4[4] = {rays[i].origin.x, rays[i].origin.y, rays[i].origin.z, rays[i].origin.w};
            const float d4[4] = {rays[i].direction.x, rays[i].direction.y, rays[i].direction.z, rays[i].direction.w};
            const float t_min = o4[3], t_max = d4[3];
            const bool walked = ah_walkable(o4, d4);
            uint32_t count = 0u, entering = 0u, exits = 0u;
            AhList list;
            ah_list_clear(list);
            if (walked)
            {
                float inv[3];
                ah_inverse(d4, inv);
                for (uint32_t k = 0; k < nn; ++k)
                {
                    const rt_bvh_node& nd = nodes[k];
                    const uint32_t np = nd.num_primitives_axis >> 16;
                    if (np == 0u) continue;
                    const float lo[3] = {nd.bounds_min.x, nd.bounds_min.y, nd.bounds_min.z}, hi[3] = {nd.bounds_max.x, nd.bounds_max.y, nd.bounds_max.z};
                    if (!ah_box(lo, hi, o4, inv, t_min, t_max)) continue;
                    for (uint32_t prim = nd.offset; prim < nd.offset + np; ++prim)
                    {
                        float p1[3], e1[3], e2[3], u, v, t, det;
                        corners(prim, p1, e1, e2);
                        if (!ah_triangle(o4, d4, p1, e1, e2, t_min, t_max, &u, &v, &t, &det)) continue;
                        ++count;
                        if (det > 0.0f) ++entering;
                        ah_list_insert(list, t, prim);
                    }
                }
            }
            for (uint32_t j = 0; j < max_hits; ++j)
            {
                rt_hit h = {{0.0f, 0.0f}, RT_INVALID_ID, 0.0f};
                if (j < count)
                {
                    float p1[3], e1[3], e2[3], u = 0.0f, v = 0.0f, t = 0.0f, det = 0.0f;
                    corners(list.prim[j], p1, e1, e2);
                    (void)ah_triangle(o4, d4, p1, e1, e2, t_min, t_max, &u, &v, &t, &det);
                    if (det < 0.0f) exits |= 1u << j;
                    h.bc.x = u; h.bc.y = v; h.primitive_id = list.prim[j]; h.t = t;
                }
                hits[(size_t)i * max_hits + j] = h;
            }
            out[i] = ah_record(count, entering, max_hits, exits, walked);
        }
    });
}

bool brute_device(hipStream_t stream, const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, const rt_ray* rays, uint32_t n,
    uint32_t max_hits, rt_ray_hits* out, rt_hit* hits)
{
    dev::Temps tmp(stream);
    void* const d_nodes = tmp.get(nodes, (size_t)nn * sizeof(rt_bvh_node));
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_rays = tmp.get(rays, (size_t)n * sizeof(rt_ray));
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_ray_hits));
    void* const d_hits = tmp.get(nullptr, (size_t)n * max_hits * sizeof(rt_hit));
    bool ok = d_nodes && d_tris && d_rays && d_out && d_hits;
    if (ok)
        hipLaunchKernelGGL(k_all_hits_brute, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, (const rt_bvh_node*)d_nodes, nn, (const rt_triangle*)d_tris,
            (const float4*)d_rays, n, max_hits, (float4*)d_out, (float4*)d_hits);
    ok = ok && dev::clean();
    if (ok && max_hits > 0u) ok = hipMemcpyAsync(hits, d_hits, (size_t)n * max_hits * sizeof(rt_hit), hipMemcpyDeviceToHost, stream) == hipSuccess;
    return tmp.finish(ok, out, d_out, (size_t)n * sizeof(rt_ray_hits));
}
} // namespace all_hits
