// query.hip -- caller-supplied rays traced against the uploaded scene (rt_scene_trace / rt_scene_trace_buffer / rt_frame_pick): the kernels
// (query_kernels.h), their host driver, the pick ray and the host restatement of the surface record (query.h).  A translation unit and a code object of its own so
// that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "query_kernels.h"
#include "spatial_filter.h"       // sf_guide_dir: the guide pass's pixel-centre direction, shared with rt_frame_pick
#include "query_host.h"

namespace query
{
static_assert(sizeof(rt_ray) == 2 * sizeof(float4) && sizeof(rt_hit) == sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4), "records as 16-byte pieces");
#define RT_QUERY_WAVES_PER_CU 24u       // 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow 24

size_t Scratch::spill_bytes() const { return (size_t)spill_blocks * 64u * RT_QUERY_SPILL_PER_LANE * sizeof(uint2); }
size_t Scratch::bytes() const
{
    size_t b = spill_bytes();
    for (int k = 0; k < 4; ++k) b += stage_bytes[k];
    return b;
}

void release(Scratch& s)
{
    if (s.spill) (void)hipFree(s.spill);
    if (s.status) (void)hipHostFree(s.status);
    for (int k = 0; k < 4; ++k) if (s.stage[k]) (void)hipFree(s.stage[k]);
    s = Scratch();
}

bool reserve(hipStream_t stream, Scratch& s, int k, size_t bytes)
{
    if (bytes <= s.stage_bytes[k]) return true;
    if (s.stage[k])
    {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(s.stage[k]);
        s.stage[k] = nullptr; s.stage_bytes[k] = 0;
    }
    if (hipMalloc(&s.stage[k], bytes) != hipSuccess) { (void)hipGetLastError(); s.stage[k] = nullptr; return false; }
    s.stage_bytes[k] = bytes;
    return true;
}

uint32_t prepare(hipStream_t stream, Scratch& s, uint32_t** status, int compute_units, uint32_t waves_per_cu, uint32_t n_groups)
{
    const uint32_t resident = (((uint32_t)compute_units * waves_per_cu) + 7u) & ~7u;
    const uint32_t blocks = n_groups < resident ? n_groups : resident;
    if (!*status)
    {
        if (hipHostMalloc((void**)status, 4) != hipSuccess) { (void)hipGetLastError(); *status = nullptr; return 0u; }
        **status = 0u;
    }
    if (blocks > s.spill_blocks)
    {
        if (s.spill) { (void)hipStreamSynchronize(stream); (void)hipFree(s.spill); s.spill = nullptr; s.spill_blocks = 0; }
        if (hipMalloc((void**)&s.spill, (size_t)blocks * 64u * RT_QUERY_SPILL_PER_LANE * sizeof(uint2)) != hipSuccess) { (void)hipGetLastError(); s.spill = nullptr; return 0u; }
        s.spill_blocks = blocks;
    }
    return blocks;
}

bool launch(hipStream_t stream, Scratch& s, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_ray* d_rays, uint32_t n, uint32_t mode, rt_hit* d_hits, uint32_t* d_occluded, rt_surface* d_surfaces)
{
    if (n == 0u) return true;
    const uint32_t blocks = prepare(stream, s, &s.status, compute_units, RT_QUERY_WAVES_PER_CU, dev::blocks_for(n, 64u));
    if (blocks == 0u) return false;
    // the hits k_query_surface reads: the caller's, or the first 16 bytes of each surface record
    float4* hits = (float4*)d_hits;
    uint32_t hit_stride = 1u;
    if (!hits && d_surfaces) { hits = (float4*)d_surfaces; hit_stride = 4u; }
    if (mode == RT_QUERY_ANY_HIT)
        hipLaunchKernelGGL(k_query_trace<true>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_rays, n, (float4*)nullptr, 1u, d_occluded, s.spill,
            use_wide ? 1u : 0u, s.status);
    else
        hipLaunchKernelGGL(k_query_trace<false>, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_rays, n, hits, hit_stride, d_occluded, s.spill,
            use_wide ? 1u : 0u, s.status);
    if (!dev::clean()) return false;
    if (d_surfaces)
    {
        hipLaunchKernelGGL(k_query_surface<true>, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, sc.tris_sh, n_tris, object_of_triangle, (const float4*)d_rays,
            (const float4*)hits, hit_stride, n, (float4*)d_surfaces);
        if (!dev::clean()) return false;
    }
    return true;
}

rt_ray pick_ray(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y)
{
    float d[3];
    sf_guide_dir(cam, rt_tanf(0.5f * cam.fov), width, height, x, y, d);
    rt_ray r;
    r.origin = {cam.position.x, cam.position.y, cam.position.z, 0.0f};
    r.direction = {d[0], d[1], d[2], RT_MAX_RENDER_DIST};
    return r;
}

void debug_surface_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits, uint32_t n, rt_surface* out)
{
    for (uint32_t i = 0; i < n; ++i)
    {
        const uint32_t prim = hits[i].primitive_id;
        if (prim >= n_tris) { out[i] = qs_miss(); continue; }
        const float d[3] = {rays[i].direction.x, rays[i].direction.y, rays[i].direction.z};
        out[i] = query_surface(qs_triangle(tris[prim]), d, hits[i].bc.x, hits[i].bc.y, hits[i].t, prim, object_of_triangle ? object_of_triangle[prim] : RT_INVALID_ID);
    }
}

bool debug_surface_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits,
    uint32_t n, rt_surface* out)
{
    dev::Temps tmp(stream);
    void* const d_tris = tmp.get(tris, (size_t)n_tris * sizeof(rt_triangle));
    void* const d_ids = object_of_triangle ? tmp.get(object_of_triangle, (size_t)n_tris * 4) : nullptr;
    void* const d_rays = tmp.get(rays, (size_t)n * sizeof(rt_ray));
    void* const d_hits = tmp.get(hits, (size_t)n * sizeof(rt_hit));
    void* const d_out = tmp.get(nullptr, (size_t)n * sizeof(rt_surface));
    const bool ok = d_tris && (d_ids || !object_of_triangle) && d_rays && d_hits && d_out;
    if (ok)
        hipLaunchKernelGGL(k_query_surface<false>, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, (const float4*)d_tris, n_tris, (const uint32_t*)d_ids,
            (const float4*)d_rays, (const float4*)d_hits, 1u, n, (float4*)d_out);
    return tmp.finish(ok && dev::clean(), out, d_out, (size_t)n * sizeof(rt_surface));
}
} // namespace query
