// light_bake_host.h -- the interface of light_bake.hip: the irradiance of the sky and of the scene's analytic lights at caller-supplied points
// (rt_scene_light_bake / rt_scene_light_bake_buffer / rt_scene_atlas_bake_light / rt_debug_light_bake_rays / rt_debug_light_bake_reduce).
// The arithmetic itself is light_bake.h's.  A translation unit and a device code object of its own, like bake.hip: neither the hot path's code object
// (rt_hip.hip) nor the occlusion bake's is rebuilt or re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace light_bake
{
// why a description is refused (nullptr: it is fine): samples a power of two in 16 .. 4096, finite bias, finite sky_distance > 0, known flags
const char* desc_refusal(const rt_light_bake_desc& d);
inline size_t point_bytes(const rt_light_bake_desc& d) { return (d.flags & RT_BAKE_FROM_SURFACES) ? sizeof(rt_surface) : 32u; }

// k_bake_light over d_points[n] on `stream`, nothing waited for.  first_index: the index of d_points[0] within the caller's array (a chunk of the host form).
// s: the bakes' query::Scratch (its spill area).  *status: the query's status word, allocated here if it is not yet.  false: an allocation or the launch failed.
bool launch(hipStream_t stream, query::Scratch& s, uint32_t** status, const DScene& sc, bool use_wide, int compute_units, const void* d_points, uint32_t n,
    uint32_t first_index, const rt_light_bake_desc& d, rt_light_bake_result* d_out);

// rt_debug_light_bake_rays: n * (samples + num_lights) rays, point-major, on the host or by k_light_bake_rays on uploaded copies
void debug_rays_host(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights, uint32_t num_lights, rt_ray* out);
bool debug_rays_device(hipStream_t stream, const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights,
    uint32_t num_lights, rt_ray* out);
// rt_debug_light_bake_reduce: light_bake.h's items and reduction over the points and the verdicts of their n * (samples + num_lights) items
void debug_reduce_host(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& d, const rt_light* lights, uint32_t num_lights,
    const float* env_rgba, uint32_t env_w, uint32_t env_h, const uint32_t* occluded, rt_light_bake_result* out);
} // namespace light_bake
