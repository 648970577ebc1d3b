// atlas.hip -- the scene's triangles rasterised into a UV atlas and the surfaces its texels show (rt_scene_atlas* / rt_scene_atlas_surfaces* /
// rt_scene_atlas_bake / rt_debug_atlas): the kernels (atlas_kernels.h), their host driver and the host restatement of the rule (atlas.h).
// A translation unit and a code object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.
// -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "rt_hip.h"
#include "atlas_kernels.h"
#include "atlas_host.h"
#include "device_memory.h"

namespace atlas
{
static_assert(sizeof(rt_texel) == sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4) && sizeof(rt_atlas_stats) <= HEADER_BYTES, "records as 16-byte pieces");

static size_t texels_of(const rt_atlas_desc& d) { return (size_t)d.width * d.height; }

size_t work_bytes(const rt_atlas_desc& d)
{
    return (size_t)HEADER_BYTES + texels_of(d) * ((d.gutter ? sizeof(rt_texel) : 0u) + 2u * sizeof(uint32_t));
}

bool launch(hipStream_t stream, void* d_work, const rt_atlas_desc& d, const float* d_uv, const float4* tris_sh, uint32_t n_tris, const uint32_t* d_object_of_triangle,
    rt_texel* d_texels)
{
    const size_t n = texels_of(d);
    uint32_t* const stats = (uint32_t*)d_work;
    float4* const second = (float4*)((char*)d_work + HEADER_BYTES);
    uint32_t* const owner = (uint32_t*)((char*)d_work + HEADER_BYTES + (d.gutter ? n * sizeof(rt_texel) : 0u));
    uint32_t* const count = owner + n;
    if (hipMemsetAsync(stats, 0, HEADER_BYTES, stream) != hipSuccess || hipMemsetAsync(owner, 0xFF, n * 4u, stream) != hipSuccess ||
        hipMemsetAsync(count, 0, n * 4u, stream) != hipSuccess)
        return false;
    const dim3 per_texel(dev::blocks_for(n, 256u));
    // the ping-pong ends in d_texels: the resolve writes there when the passes are even in number
    float4* from = (d.gutter & 1u) ? second : (float4*)d_texels;
    float4* to = (d.gutter & 1u) ? (float4*)d_texels : second;
    if (n_tris > 0u)
    {
        if (d_uv)
            hipLaunchKernelGGL(k_atlas_cover<false>, dim3(dev::blocks_for(n_tris, 256u)), dim3(256), 0, stream, d_uv, tris_sh, n_tris, d_object_of_triangle, d.object, d.width,
                d.height, owner, count, stats);
        else
            hipLaunchKernelGGL(k_atlas_cover<true>, dim3(dev::blocks_for(n_tris, 256u)), dim3(256), 0, stream, d_uv, tris_sh, n_tris, d_object_of_triangle, d.object, d.width,
                d.height, owner, count, stats);
        if (!dev::clean()) return false;
    }
    if (d_uv) hipLaunchKernelGGL(k_atlas_resolve<false>, per_texel, dim3(256), 0, stream, d_uv, tris_sh, d.width, d.height, owner, count, from, stats);
    else hipLaunchKernelGGL(k_atlas_resolve<true>, per_texel, dim3(256), 0, stream, d_uv, tris_sh, d.width, d.height, owner, count, from, stats);
    if (!dev::clean()) return false;
    for (uint32_t pass = 0; pass < d.gutter; ++pass)
    {
        hipLaunchKernelGGL(k_atlas_gutter, per_texel, dim3(256), 0, stream, d.width, d.height, (const float4*)from, to, stats);
        if (!dev::clean()) return false;
        float4* const t = from; from = to; to = t;
    }
    return true;
}

bool launch_surfaces(hipStream_t stream, const float4* tris_sh, uint32_t n_tris, const uint32_t* d_object_of_triangle, const rt_texel* d_texels, uint32_t n,
    rt_surface* d_surfaces)
{
    if (n == 0u) return true;
    hipLaunchKernelGGL(k_atlas_surfaces, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, tris_sh, n_tris, d_object_of_triangle, (const float4*)d_texels, n,
        (float4*)d_surfaces);
    return dev::clean();
}

// six floats per triangle from the triangles' own texcoord.xy
static std::vector<float> own_uv(const rt_triangle* tris, uint32_t n_tris)
{
    std::vector<float> uv((size_t)n_tris * 6u);
    for (uint32_t i = 0; i < n_tris; ++i)
    {
        const rt_vertex* v[3] = {&tris[i].v1, &tris[i].v2, &tris[i].v3};
        for (int k = 0; k < 3; ++k) { uv[(size_t)i * 6u + 2 * k] = v[k]->texcoord.x; uv[(size_t)i * 6u + 2 * k + 1] = v[k]->texcoord.y; }
    }
    return uv;
}

void cover_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const float* uv, const rt_atlas_desc& d, rt_texel* texels, rt_atlas_stats* stats)
{
    std::vector<float> own;
    if (!uv) { own = own_uv(tris, n_tris); uv = own.data(); }
    const size_t n = texels_of(d);
    std::vector<uint32_t> owner(n, RT_INVALID_ID), count(n, 0u);
    rt_atlas_stats st;
    memset(&st, 0, sizeof st);
    for (uint32_t i = 0; i < n_tris; ++i)
    {
        if (d.object != RT_INVALID_ID && object_of_triangle[i] != d.object) { ++st.triangles_filtered; continue; }
        AtlasTri t;
        if (!atlas_setup(uv + (size_t)i * 6u, d.width, d.height, &t)) { ++st.triangles_skipped; continue; }
        uint32_t covered = 0u;
        for (int32_t y = t.y0; y <= t.y1; ++y)
            for (int32_t x = t.x0; x <= t.x1; ++x)
                if (atlas_covers(t, x, y))
                {
                    const size_t idx = (size_t)y * d.width + (size_t)x;
                    if (i < owner[idx]) owner[idx] = i;
                    ++count[idx];
                    ++covered;
                }
        if (covered == 0u) ++st.triangles_without_texel;
    }
    for (size_t idx = 0; idx < n; ++idx)
    {
        rt_texel r = atlas_uncovered();
        if (count[idx] != 0u)
        {
            AtlasTri t;
            (void)atlas_setup(uv + (size_t)owner[idx] * 6u, d.width, d.height, &t);
            atlas_bc(t, (int32_t)(idx % d.width), (int32_t)(idx / d.width), r.bc);
            r.primitive_id = owner[idx]; r.count = (uint16_t)(count[idx] < 65535u ? count[idx] : 65535u); r.flags = (uint16_t)RT_TEXEL_COVERED;
            ++st.covered;
            if (count[idx] > 1u) ++st.overlapped;
        }
        texels[idx] = r;
    }
    std::vector<rt_texel> next(d.gutter ? n : 0u);
    for (uint32_t pass = 0; pass < d.gutter; ++pass)
    {
        const int nb[8][2] = RT_ATLAS_NEIGHBOURS;
        for (size_t idx = 0; idx < n; ++idx)
        {
            rt_texel r = texels[idx];
            if (r.flags == 0u)
            {
                const int32_t x = (int32_t)(idx % d.width), y = (int32_t)(idx / d.width);
                for (int k = 0; k < 8; ++k)
                {
                    const int32_t nx = x + nb[k][0], ny = y + nb[k][1];
                    if (nx < 0 || ny < 0 || nx >= (int32_t)d.width || ny >= (int32_t)d.height) continue;
                    const rt_texel& q = texels[(size_t)ny * d.width + (size_t)nx];
                    if (q.flags == 0u) continue;
                    r = q; r.flags = (uint16_t)RT_TEXEL_GUTTER; r.count = 0u;
                    ++st.gutter;
                    break;
                }
            }
            next[idx] = r;
        }
        memcpy(texels, next.data(), n * sizeof(rt_texel));
    }
    if (stats) *stats = st;
}

bool cover_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const float* uv, const rt_atlas_desc& d, rt_texel* texels,
    rt_atlas_stats* stats)
{
    std::vector<float> own;
    if (!uv) { own = own_uv(tris, n_tris); uv = own.data(); }
    const size_t n = texels_of(d);
    dev::Temps tmp(stream);
    void* const d_uv = tmp.get(uv, (size_t)n_tris * 24u);
    void* const d_ids = d.object != RT_INVALID_ID ? tmp.get(object_of_triangle, (size_t)n_tris * 4u) : nullptr;
    void* const d_work = tmp.get(nullptr, work_bytes(d));
    void* const d_texels = tmp.get(nullptr, n * sizeof(rt_texel));
    bool ok = d_uv && (d_ids || d.object == RT_INVALID_ID) && d_work && d_texels;
    ok = ok && launch(stream, d_work, d, (const float*)d_uv, nullptr, n_tris, (const uint32_t*)d_ids, (rt_texel*)d_texels);
    ok = ok && (!stats || hipMemcpyAsync(stats, d_work, sizeof(rt_atlas_stats), hipMemcpyDeviceToHost, stream) == hipSuccess);
    return tmp.finish(ok, texels, d_texels, n * sizeof(rt_texel));
}
} // namespace atlas
