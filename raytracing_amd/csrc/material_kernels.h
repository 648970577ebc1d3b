// material_kernels.h -- the material record and its texture lookups (material.h:251-369, utils.h:123-190): what k_shade and the spatial filter's
// guide pass (filters.hip) both need.  Device functions only: including it compiles no kernel.
#pragma once
#include "kernels_common.h"

struct Material
{
    f3 diffuse_albedo; float roughness;
    f3 specular_albedo; float metalness;
    f3 emission; float ior; float transparency;
};

// material.h:251-264 + utils.h:123-131
RT_DEV f3 SampleTexture(const DScene& sc, uint32_t tex_idx, f2 uv)
{
    rt_texture tex = sc.textures[tex_idx];
    uv.x -= __builtin_floorf(uv.x);
    uv.y -= __builtin_floorf(uv.y);
    uv.y = 1.f - uv.y;
    int texel_x = cl_clampi((int)(uv.x * (float)tex.width), 0, tex.width - 1);
    int texel_y = cl_clampi((int)(uv.y * (float)tex.height), 0, tex.height - 1);
    int texel_addr = tex.data_start + texel_y * tex.width + texel_x;
    uint32_t data = sc.texture_data[texel_addr];
    float r = (float)(data & 0xFF) / 255.0f;
    float g = (float)((data >> 8) & 0xFF) / 255.0f;
    float b = (float)((data >> 16) & 0xFF) / 255.0f;
    return F3(cl_min(cl_max(r, 0.0f), 1.0f), cl_min(cl_max(g, 0.0f), 1.0f), cl_min(cl_max(b, 0.0f), 1.0f));
}

// pow(SampleTexture(...), 2.2f) (material.h:327,336,361).  A texel channel is one of 256 values,
// so the three rt_powf evaluations (~200 fp64 operations each, paid by the whole wave as soon as
// one lane has a textured material) are a table of the very same function, filled on the device
// by the very same code (k_fill_gamma_lut) -- identical bits by construction.
RT_DEV f3 SampleTextureGamma(const DScene& sc, uint32_t tex_idx, f2 uv)
{
    rt_texture tex = sc.textures[tex_idx];
    uv.x -= __builtin_floorf(uv.x);
    uv.y -= __builtin_floorf(uv.y);
    uv.y = 1.f - uv.y;
    int texel_x = cl_clampi((int)(uv.x * (float)tex.width), 0, tex.width - 1);
    int texel_y = cl_clampi((int)(uv.y * (float)tex.height), 0, tex.height - 1);
    uint32_t data = sc.texture_data[tex.data_start + texel_y * tex.width + texel_x];
    return F3(sc.gamma_lut[data & 0xFF], sc.gamma_lut[(data >> 8) & 0xFF], sc.gamma_lut[(data >> 16) & 0xFF]);
}

RT_DEV f3 UnpackRGBTex(uint32_t data, uint32_t& idx)                    // utils.h:133-147
{
    float r = (float)(data & 0xFF), g = (float)((data >> 8) & 0xFF), b = (float)((data >> 16) & 0xFF);
    idx = (data >> 24) & 0xFF;
    return F3(r / 255.0f, g / 255.0f, b / 255.0f);
}

// mtl: the material's index (for the wide texture indices of rt_scene_desc::material_texture_indices, when given)
RT_DEV void ApplyTextures(const DScene& sc, uint32_t mtl, Material& out, f2 uv)   // material.h:319-369
{
    const rt_packed_material in = sc.materials[mtl];
    // texture index of slot k: the packed 8-bit field (0xFF = none), or the 16-bit side table (0xFFFF = none)
    const uint16_t* wide = sc.mat_tex16 ? sc.mat_tex16 + (size_t)mtl * 6u : nullptr;
    const uint32_t none = wide ? 0xFFFFu : RT_INVALID_TEXTURE_IDX;
    uint32_t idx;
    out.diffuse_albedo = UnpackRGBTex(in.diffuse_albedo, idx);
    if (wide) idx = wide[0];
    if (idx != none) out.diffuse_albedo = SampleTextureGamma(sc, idx, uv);
    out.specular_albedo = UnpackRGBTex(in.specular_albedo, idx);
    if (wide) idx = wide[1];
    if (idx != none) out.specular_albedo = SampleTextureGamma(sc, idx, uv);
    {
        uint32_t rgbe = in.emission;                                     // utils.h:149-158
        int r = (int)(rgbe & 0xFF), g = (int)((rgbe >> 8) & 0xFF), b = (int)((rgbe >> 16) & 0xFF);
        int e = (int)(rgbe >> 24);
        float f = rt_ldexpf(1.0f, e - (128 + 8));
        out.emission = F3((float)r * f, (float)g * f, (float)b * f);
    }
    uint32_t d = in.roughness_metalness;                                 // utils.h:160-174
    out.roughness = (float)(d & 0xFF) / 255.0f;
    uint32_t roughness_idx = wide ? wide[2] : (d >> 8) & 0xFF;
    out.metalness = (float)((d >> 16) & 0xFF) / 255.0f;
    uint32_t metalness_idx = wide ? wide[3] : (d >> 24) & 0xFF;
    if (roughness_idx != none) out.roughness = SampleTexture(sc, roughness_idx, uv).x;
    if (metalness_idx != none) out.metalness = SampleTexture(sc, metalness_idx, uv).x;
    d = in.ior_emission_idx_transparency;                                // utils.h:176-190
    out.ior = (float)(d & 0xFF) / 25.5f;
    uint32_t emission_idx = wide ? wide[4] : (d >> 8) & 0xFF;
    out.transparency = (float)((d >> 16) & 0xFF) / 255.0f;
    uint32_t transparency_idx = wide ? wide[5] : (d >> 24) & 0xFF;
    if (emission_idx != none)
        out.emission = out.emission * SampleTextureGamma(sc, emission_idx, uv);
    if (transparency_idx != none)
        out.transparency *= SampleTexture(sc, transparency_idx, uv).x;
}
