// light_bake.hip -- the irradiance of the sky and of the scene's analytic lights at caller-supplied points (rt_scene_light_bake / rt_scene_light_bake_buffer /
// rt_scene_atlas_bake_light / rt_debug_light_bake_rays / rt_debug_light_bake_reduce): the kernels (light_bake_kernels.h), their host
// driver and the host restatement of the arithmetic (light_bake.h).  A translation unit and a code object of its own so that neither the hot path's code
// object (rt_hip.hip, codeobj.code_object_sha256) nor the occlusion bake's (bake.hip) changes.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "rt_hip.h"
#include "light_bake_kernels.h"
#include "light_bake_host.h"

namespace light_bake
{
static_assert(sizeof(rt_light_bake_result) == 2 * sizeof(float4) && sizeof(rt_surface) == 4 * sizeof(float4) && sizeof(rt_ray) == 2 * sizeof(float4) &&
              sizeof(rt_light) == 3 * sizeof(float4), "records as 16-byte pieces");
// (the figures: hipcc -Rpass-analysis=kernel-resource-usage on this unit with _build.py's HIP_FLAGS; k_bake_light must report ScratchSize 0)
#define RT_LIGHT_BAKE_WAVES_PER_CU 16u  // 6 KiB of LDS per block: 26 fit a CU's 160 KiB; the registers allow 4 waves per SIMD

const char* desc_refusal(const rt_light_bake_desc& d)
{
    if (d.samples < 16u || d.samples > 4096u || (d.samples & (d.samples - 1u)) != 0u) return "samples must be a power of two in 16 .. 4096";
    if (!__builtin_isfinite(d.bias)) return "bias is not finite";
    if (!__builtin_isfinite(d.sky_distance) || !(d.sky_distance > 0.0f)) return "sky_distance must be finite and > 0";
    if ((d.flags & ~RT_LIGHT_BAKE_FLAGS_KNOWN) != 0u) return "unknown flag bits (RT_BAKE_FROM_SURFACES, RT_LIGHT_BAKE_NO_SKY, RT_LIGHT_BAKE_NO_LIGHTS)";
    return nullptr;
}

bool launch(hipStream_t stream, query::Scratch& s, uint32_t** status, const DScene& sc, bool use_wide, int compute_units, const void* d_points, uint32_t n,
    uint32_t first_index, const rt_light_bake_desc& d, rt_light_bake_result* d_out)
{
    if (n == 0u) return true;
    const uint32_t per_wave = d.samples < 64u ? 64u / d.samples : 1u;
    const uint32_t blocks = query::prepare(stream, s, status, compute_units, RT_LIGHT_BAKE_WAVES_PER_CU, dev::blocks_for(n, per_wave));
    if (blocks == 0u) return false;
    hipLaunchKernelGGL(k_bake_light, dim3(blocks), dim3(64), 0, stream, sc, (const float4*)d_points, n, first_index, d.samples, d.seed, d.flags, d.bias, d.sky_distance,
        (float4*)d_out, s.spill, use_wide ? 1u : 0u, *status);
    return dev::clean();
}

// item r of a walked point
static LightBakeItem host_item(const BakeFrame& f, float r1, float r2, uint32_t r, const rt_light_bake_desc& d, const rt_light* lights)
{
    if (r < d.samples) return light_bake_sky_item(f, r1, r2, r, d.samples, d.flags, d.sky_distance);
    const rt_light& l = lights[r - d.samples];
    const float lo[3] = {l.origin.x, l.origin.y, l.origin.z}, lr[3] = {l.radiance.x, l.radiance.y, l.radiance.z};
    return light_bake_light_item(f, lo, lr, l.type, d.flags, d.sky_distance);
}

static BakeFrame host_frame(const void* points, uint32_t p, const rt_light_bake_desc& d)
{
    float pos[3], nrm[3];
    const bool record_ok = bake_point((const float*)points + (size_t)p * (point_bytes(d) / sizeof(float)), (d.flags & RT_BAKE_FROM_SURFACES) != 0u, pos, nrm);
    return bake_frame(pos, nrm, record_ok, d.bias);
}

void debug_rays_host(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights, uint32_t num_lights, rt_ray* out)
{
    const size_t items = (size_t)d.samples + num_lights;
    for (uint32_t p = 0; p < n; ++p)
    {
        const BakeFrame f = host_frame(points, p, d);
        float r1 = 0.0f, r2 = 0.0f;
        bake_rotations(first_index + p, d.seed, &r1, &r2);
        for (uint32_t r = 0; r < items; ++r)
        {
            rt_ray& ray = out[(size_t)p * items + r];
            ray.origin = {0.0f, 0.0f, 0.0f, 0.0f}; ray.direction = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!f.walked) continue;
            const LightBakeItem it = host_item(f, r1, r2, r, d, lights);
            if (!it.made) continue;
            ray.origin = {f.origin[0], f.origin[1], f.origin[2], 0.0f};
            ray.direction = {it.dir[0], it.dir[1], it.dir[2], it.t_max};
        }
    }
}

bool debug_rays_device(hipStream_t stream, const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights,
    uint32_t num_lights, rt_ray* out)
{
    const size_t n_rays = (size_t)n * ((size_t)d.samples + num_lights);
    dev::Temps tmp(stream);
    void* const d_points = tmp.get(points, (size_t)n * point_bytes(d));
    void* const d_lights = tmp.get(lights, (size_t)num_lights * sizeof(rt_light));
    void* const d_rays = tmp.get(nullptr, n_rays * sizeof(rt_ray));
    const bool ok = d_points && d_lights && d_rays;
    if (ok)
        hipLaunchKernelGGL(k_light_bake_rays, dim3(dev::blocks_for(n_rays, 256u)), dim3(256), 0, stream, (const float4*)d_points, n, first_index, d.samples, d.seed,
            d.flags, d.bias, d.sky_distance, (const float4*)d_lights, num_lights, (float4*)d_rays);
    return tmp.finish(ok && dev::clean(), out, d_rays, n_rays * sizeof(rt_ray));
}

void debug_reduce_host(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights, uint32_t num_lights,
    const float* env_rgba, uint32_t env_w, uint32_t env_h, const uint32_t* occluded, rt_light_bake_result* out)
{
    const uint32_t L = d.samples < RT_BAKE_SLOTS_MAX ? d.samples : RT_BAKE_SLOTS_MAX;
    const size_t items = (size_t)d.samples + num_lights;
    for (uint32_t p = 0; p < n; ++p)
    {
        rt_light_bake_result& o = out[p];
        for (int q = 0; q < 3; ++q) { o.sky[q] = 0.0f; o.lights[q] = 0.0f; }
        const BakeFrame f = host_frame(points, p, d);
        if (!f.walked) { o.sky_unoccluded = RT_INVALID_ID; o.lights_unshadowed = RT_INVALID_ID; continue; }
        float r1 = 0.0f, r2 = 0.0f;
        bake_rotations(first_index + p, d.seed, &r1, &r2);
        const uint32_t* occ = occluded + (size_t)p * items;
        float sky[RT_BAKE_SLOTS_MAX][3], lit[RT_BAKE_SLOTS_MAX][3];
        uint32_t n_sky = 0u, n_lit = 0u;
        for (uint32_t l = 0; l < L; ++l)
        {
            for (int q = 0; q < 3; ++q) { sky[l][q] = 0.0f; lit[l][q] = 0.0f; }
            for (size_t r = l; r < items; r += L)
            {
                const LightBakeItem it = host_item(f, r1, r2, (uint32_t)r, d, lights);
                if (!it.made || occ[r]) continue;
                if (r < d.samples)
                {
                    float rgb[3];
                    light_bake_sky((const rt_float4*)env_rgba, (int)env_w, (int)env_h, it.dir, rgb);
                    for (int q = 0; q < 3; ++q) sky[l][q] = sky[l][q] + rgb[q];
                    ++n_sky;
                }
                else
                {
                    for (int q = 0; q < 3; ++q) lit[l][q] = lit[l][q] + it.E[q];
                    ++n_lit;
                }
            }
        }
        for (uint32_t s = L >> 1; s > 0u; s >>= 1)
            for (uint32_t l = 0; l < s; ++l)
                for (int q = 0; q < 3; ++q) { sky[l][q] = sky[l][q] + sky[l + s][q]; lit[l][q] = lit[l][q] + lit[l + s][q]; }
        light_bake_finish(sky[0], d.samples, o.sky);
        for (int q = 0; q < 3; ++q) o.lights[q] = lit[0][q];
        o.sky_unoccluded = n_sky;
        o.lights_unshadowed = n_lit;
    }
}
} // namespace light_bake
