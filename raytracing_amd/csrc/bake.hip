// bake.hip -- ambient occlusion and bent normals at caller-supplied points (rt_scene_bake / rt_scene_bake_buffer / rt_debug_bake_rays / rt_debug_bake_reduce,
// DESIGN.md section 7i): the kernels (bake_kernels.h), their host driver and the host restatement of the arithmetic (bake.h).  A translation unit and a code
// object of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "bake_kernels.h"
#include "bake_host.h"

namespace bake
{
static_assert(sizeof(rt_bake_result) == sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4) && sizeof(rt_ray) == 2 * sizeof(float4), "records as 16-byte pieces");
#define RT_BAKE_WAVES_PER_CU 20u        // 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers (82 VGPRs) allow 5 waves per SIMD

const char* desc_refusal(const rt_bake_desc& d)
{
    if (d.samples < 16u || d.samples > 4096u || (d.samples & (d.samples - 1u)) != 0u) return "samples must be a power of two in 16 .. 4096";
    if (!__builtin_isfinite(d.bias)) return "bias is not finite";
    if (!__builtin_isfinite(d.radius) || !(d.radius > 0.0f)) return "radius must be finite and > 0";
    if ((d.flags & ~RT_BAKE_FLAGS_KNOWN) != 0u) return "unknown flag bits (RT_BAKE_FROM_SURFACES)";
    return nullptr;
}

bool launch(hipStream_t stream, query::Scratch& s, uint32_t** status, const DScene& sc, bool use_wide, int compute_units, const void* d_points, uint32_t n,
    uint32_t first_index, const rt_bake_desc& d, rt_bake_result* d_out)
{
    if (n == 0u) return true;
    const uint32_t per_wave = d.samples < 64u ? 64u / d.samples : 1u;
    const uint32_t blocks = query::prepare(stream, s, status, compute_units, RT_BAKE_WAVES_PER_CU, dev::blocks_for(n, per_wave));
    if (blocks == 0u) return false;
    hipLaunchKernelGGL(k_bake, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_points, (d.flags & RT_BAKE_FROM_SURFACES) ? 1u : 0u, n, first_index, d.samples,
        d.seed, d.bias, d.radius, (float4*)d_out, s.spill, use_wide ? 1u : 0u, *status);
    return dev::clean();
}

void debug_rays_host(const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc& d, rt_ray* out)
{
    const bool from_surfaces = (d.flags & RT_BAKE_FROM_SURFACES) != 0u;
    const size_t stride = point_bytes(d) / sizeof(float);
    for (uint32_t p = 0; p < n; ++p)
    {
        float pos[3], nrm[3];
        const bool record_ok = bake_point((const float*)points + (size_t)p * stride, from_surfaces, pos, nrm);
        const BakeFrame f = bake_frame(pos, nrm, record_ok, d.bias);
        float r1 = 0.0f, r2 = 0.0f;
        bake_rotations(first_index + p, d.seed, &r1, &r2);
        for (uint32_t k = 0; k < d.samples; ++k)
        {
            rt_ray& r = out[(size_t)p * d.samples + k];
            if (!f.walked) { r.origin = {0.0f, 0.0f, 0.0f, 0.0f}; r.direction = {0.0f, 0.0f, 0.0f, 0.0f}; continue; }
            float dd[3];
            bake_direction(f, r1, r2, k, d.samples, dd);
            r.origin = {f.origin[0], f.origin[1], f.origin[2], 0.0f};
            r.direction = {dd[0], dd[1], dd[2], d.radius};
        }
    }
}

bool debug_rays_device(hipStream_t stream, const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc& d, rt_ray* out)
{
    const size_t n_rays = (size_t)n * d.samples;
    dev::Temps tmp(stream);
    void* const d_points = tmp.get(points, (size_t)n * point_bytes(d));
    void* const d_rays = tmp.get(nullptr, n_rays * sizeof(rt_ray));
    const bool ok = d_points && d_rays;
    if (ok)
        hipLaunchKernelGGL(k_bake_rays, dim3(dev::blocks_for(n_rays, 256u)), dim3(256), 0, stream, (const float4*)d_points, (d.flags & RT_BAKE_FROM_SURFACES) ? 1u : 0u, n,
            first_index, d.samples, d.seed, d.bias, d.radius, (float4*)d_rays);
    return tmp.finish(ok && dev::clean(), out, d_rays, n_rays * sizeof(rt_ray));
}

void debug_reduce_host(const rt_ray* rays, const uint32_t* occluded, uint32_t n, uint32_t samples, rt_bake_result* out)
{
    const uint32_t L = samples < RT_BAKE_SLOTS_MAX ? samples : RT_BAKE_SLOTS_MAX;
    for (uint32_t p = 0; p < n; ++p)
    {
        const rt_ray* r = rays + (size_t)p * samples;
        const uint32_t* occ = occluded + (size_t)p * samples;
        rt_bake_result& o = out[p];
        o.bent_normal[0] = o.bent_normal[1] = o.bent_normal[2] = 0.0f;
        if (r[0].direction.x == 0.0f && r[0].direction.y == 0.0f && r[0].direction.z == 0.0f) { o.unoccluded = RT_INVALID_ID; continue; }
        float v[RT_BAKE_SLOTS_MAX][3];
        uint32_t count = 0u;
        for (uint32_t l = 0; l < L; ++l)
        {
            v[l][0] = v[l][1] = v[l][2] = 0.0f;
            for (uint32_t k = l; k < samples; k += L)
                if (!occ[k])
                {
                    v[l][0] = v[l][0] + r[k].direction.x; v[l][1] = v[l][1] + r[k].direction.y; v[l][2] = v[l][2] + r[k].direction.z;
                    ++count;
                }
        }
        for (uint32_t s = L >> 1; s > 0u; s >>= 1)
            for (uint32_t l = 0; l < s; ++l)
                for (int q = 0; q < 3; ++q) v[l][q] = v[l][q] + v[l + s][q];
        bake_bent(v[0], o.bent_normal);
        o.unoccluded = count;
    }
}
} // namespace bake
