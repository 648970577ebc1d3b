// atlas_host.h -- the interface of atlas.hip: the scene's triangles rasterised into a UV atlas, and the surfaces its texels show (rt_scene_atlas* /
// rt_scene_atlas_surfaces* / rt_scene_atlas_bake / rt_debug_atlas).  The rule itself is atlas.h's.  A translation unit and a device code
// object of its own, like bake.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"

namespace atlas
{
enum { HEADER_BYTES = 256 };        // the work area starts with the rt_atlas_stats the kernels add to

// The work area of one cover, device memory of the caller's: HEADER_BYTES | with a gutter the second rt_texel array of the ping-pong | the owner plane | the
// count plane.
size_t work_bytes(const rt_atlas_desc& d);

// The cover's launches on `stream`, nothing waited for: the planes and the statistics cleared, k_atlas_cover, k_atlas_resolve, d.gutter passes of
// k_atlas_gutter ordered so that the last one writes d_texels.  d_uv: six floats per triangle, or nullptr for tris_sh's own (the scene's 128-byte shading
// records).  d_object_of_triangle: read when d.object is set.  Afterwards the first sizeof(rt_atlas_stats) bytes of d_work are the statistics.
// false: a launch failed.
bool launch(hipStream_t stream, void* d_work, const rt_atlas_desc& d, const float* d_uv, const float4* tris_sh, uint32_t n_tris, const uint32_t* d_object_of_triangle,
    rt_texel* d_texels);

// k_atlas_surfaces over d_texels[n] on `stream`, nothing waited for
bool launch_surfaces(hipStream_t stream, const float4* tris_sh, uint32_t n_tris, const uint32_t* d_object_of_triangle, const rt_texel* d_texels, uint32_t n,
    rt_surface* d_surfaces);

// rt_debug_atlas: atlas.h over caller triangles on the host, or the kernels on uploaded copies (uv nullptr: the triangles' own texcoord.xy)
void cover_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const float* uv, const rt_atlas_desc& d, rt_texel* texels, rt_atlas_stats* stats);
bool cover_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const float* uv, const rt_atlas_desc& d, rt_texel* texels,
    rt_atlas_stats* stats);
} // namespace atlas
