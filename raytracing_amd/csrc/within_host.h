// within_host.h -- the interface of within.hip: every triangle within a radius of caller-supplied points (rt_scene_within / rt_scene_within_buffer /
// rt_debug_within / rt_debug_within_walk).  The arithmetic is nearest.h's, the membership rule and the list within.h's.  A translation
// unit and a device code object of its own, like nearest.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace within
{
// The query's launches on `stream`, nothing waited for: k_within over d_points[n] (the 4-wide records when use_wide, the child-pair records otherwise), then
// k_within_surface when d_surfaces is given.  d_near may be nullptr when d_surfaces is given (the records then pass through the surfaces' own memory), and
// both may be nullptr (only d_out is written).  The stack spill area and the status word are the ray queries' (q), grown or allocated here as query::launch
// does.  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_point* d_points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* d_out, rt_nearest* d_near, rt_surface* d_surfaces);

// rt_debug_within: brute force over all triangles, on the host or by k_within_brute on uploaded copies.  near may be nullptr when max_near == 0.
void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near);
bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options,
    rt_point_hits* out, rt_nearest* near);

// rt_debug_within_walk: k_within's walk on the host (nearest::walk_points with within.h's bound).  nullptr, or why the walk was refused.
const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, uint32_t* tested);
} // namespace within
