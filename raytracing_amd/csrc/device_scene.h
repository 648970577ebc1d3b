// device_scene.h -- DScene, the kernels' view of an uploaded scene: the record every launch receives by value.  Apart from kernels_common.h (which
// includes it) so that host translation units that hold one (context.h: Scene::d) need no device code and compile as plain C++.
#pragma once
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include "rt_types.h"

struct DScene
{
    const float4* nodes;          // 4 x float4 per interior node
    const float4* tris_rt;        // 4 x float4 per triangle
    const float4* tris_sh;        // 8 x float4 per triangle
    const rt_packed_material* materials;
    const rt_texture* textures;
    const uint32_t* texture_data;
    const float4* lights;         // 3 x float4 per light: origin, radiance, (type bits,0,0,0)
    const float4* env;
    const float* gamma_lut;       // pow(byte / 255, 2.2f) for the 256 texel values (k_fill_gamma_lut)
    int env_w, env_h;
    uint32_t light_count;
    uint32_t root_ref;            // RT_LEAF_BIT | first triangle, or interior node 0
    uint32_t entry_ref;           // "super-root" record: child 0 = (root box, root_ref), child 1 empty
    const float4* wnodes;         // 4-wide quantized nodes (k_trace_w4), 4 x float4 each; nullptr = not built
    uint32_t w_entry_ref;         // wide node 0, or RT_LEAF_BIT | first triangle when the root is a leaf
    const float4* wnodes_sh;      // the tree the SHADOW rays walk: the backend's own over the reference's leaves (own_bvh.h), or wnodes
    uint32_t w_sh_entry_ref;
    float root_min[3];
    float root_max[3];
    // opt-in extensions (rt_scene_desc): nullptr / 0 = the reference's behaviour
    const uint16_t* mat_tex16;    // 6 texture indices per material (0xFFFF = none) replacing the packed 8-bit ones
    const uint32_t* emissive;     // emissive triangle indices (Scene::GetEmissiveIndices)
    uint32_t emissive_count;
    uint32_t emissive_nee;        // RT_SCENE_EMISSIVE_NEE
};
