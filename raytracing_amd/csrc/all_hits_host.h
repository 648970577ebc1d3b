// all_hits_host.h -- the interface of all_hits.hip: every surface a caller's ray crosses (rt_scene_trace_all / rt_scene_trace_all_buffer / rt_frame_pick_all /
// rt_debug_trace_all).  The arithmetic itself is all_hits.h's.  A translation unit and a device code object of its own, like query.hip:
// the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace all_hits
{
// The query's launches on `stream`, nothing waited for: k_all_hits over d_rays[n] (the shadow rays' 4-wide records when use_wide, the child-pair records
// otherwise), then k_all_hits_surface when d_surfaces is given.  d_hits may be nullptr when d_surfaces is given (the hits then pass through the surfaces' own
// memory); both are nullptr when max_hits is 0.  The stack spill area and the status word are the ray queries' (q).  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_ray* d_rays, uint32_t n, uint32_t max_hits, rt_ray_hits* d_out, rt_hit* d_hits, rt_surface* d_surfaces);

// rt_debug_trace_all: brute force over the leaves of `nodes`, on the host or by k_all_hits_brute on uploaded copies.  leaves_refused: nullptr, or why the
// nodes cannot be gone through (checked before either).
const char* leaves_refused(const rt_bvh_node* nodes, uint32_t nn, uint32_t n_tris);
void brute_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits);
bool brute_device(hipStream_t stream, const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, const rt_ray* rays, uint32_t n,
    uint32_t max_hits, rt_ray_hits* out, rt_hit* hits);
} // namespace all_hits
