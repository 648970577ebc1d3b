// bake_host.h -- the interface of bake.hip: ambient occlusion and bent normals at caller-supplied points (rt_scene_bake / rt_scene_bake_buffer /
// rt_debug_bake_rays / rt_debug_bake_reduce).  The arithmetic itself is bake.h's.  A translation unit and a device code object of its
// own, like query.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace bake
{
enum { CHUNK_POINTS = 1u << 20 };        // rt_scene_bake stages at most this many points at a time (RT_CTX_OPT_BAKE_CHUNK_POINTS: fewer)

// why a description is refused (nullptr: it is fine): samples a power of two in 16 .. 4096, finite bias, finite radius > 0, known flags
const char* desc_refusal(const rt_bake_desc& d);
inline size_t point_bytes(const rt_bake_desc& d) { return (d.flags & RT_BAKE_FROM_SURFACES) ? sizeof(rt_surface) : 32u; }

// k_bake over d_points[n] on `stream`, nothing waited for.  first_index: the index of d_points[0] within the caller's array (a chunk of the host form).
// s: the context's second query::Scratch, the bakes' own (its spill area; stages 0 and 1 hold the host form's points and results).
// *status: the query's status word (pinned host memory), allocated here if it is not yet.  false: an allocation or the launch failed.
bool launch(hipStream_t stream, query::Scratch& s, uint32_t** status, const DScene& sc, bool use_wide, int compute_units, const void* d_points, uint32_t n,
    uint32_t first_index, const rt_bake_desc& d, rt_bake_result* d_out);

// rt_debug_bake_rays: n * samples rays, point-major, on the host or by k_bake_rays on an uploaded copy of the points
void debug_rays_host(const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc& d, rt_ray* out);
bool debug_rays_device(hipStream_t stream, const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc& d, rt_ray* out);
// rt_debug_bake_reduce: bake.h's reduction over n * samples rays and their verdicts; a point whose first ray has an all-zero direction is a skipped one
void debug_reduce_host(const rt_ray* rays, const uint32_t* occluded, uint32_t n, uint32_t samples, rt_bake_result* out);
} // namespace bake
