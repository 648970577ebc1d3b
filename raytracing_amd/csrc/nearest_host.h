// nearest_host.h -- the interface of nearest.hip: the nearest surface point to caller-supplied points (rt_scene_nearest / rt_scene_nearest_buffer /
// rt_debug_nearest / rt_debug_nearest_walk).  The arithmetic itself is nearest.h's.  A translation unit and a device code object of its
// own, like query.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include <functional>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;
struct NpTriangle;          // nearest.h

namespace nearest
{
// The query's launches on `stream`, nothing waited for: k_nearest over d_points[n] (the 4-wide records when use_wide, the child-pair records otherwise), then
// k_nearest_surface when d_surfaces is given.  d_out may be nullptr when d_surfaces is given (the records then pass through the surfaces' own memory).  The
// stack spill area and the status word are the ray queries' (q), grown or allocated here as query::launch does.  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_point* d_points, uint32_t n, rt_nearest* d_out, rt_surface* d_surfaces);

// rt_debug_nearest: brute force over all triangles, on the host or by k_nearest_brute on uploaded copies
void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, rt_nearest* out);
bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_point* points, uint32_t n, rt_nearest* out);

// k_nearest's and k_within's walk on the host over `nodes` (wide: over build_wide_bvh's records of them).  Every searched point starts with the bound
// max_distance^2; triangle(i, prim, t, bound) is called for each triangle point i reaches (t = nearest_point_triangle's answer) and returns the bound from
// then on.  tested[i] (optional) = how many triangles point i reached.  nullptr, or why the walk was refused.
const char* walk_points(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    uint32_t* tested, const std::function<float(uint32_t, uint32_t, const NpTriangle&, float)>& triangle);

// rt_debug_nearest_walk: k_nearest's walk on the host over `nodes` (wide: over build_wide_bvh's records of them).  nullptr, or why the walk was refused.
const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_point* points, uint32_t n,
    rt_nearest* out, uint32_t* tested);
} // namespace nearest
