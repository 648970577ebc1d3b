// separation_host.h -- the interface of separation.hip: the nearest scene triangle to a caller's triangle, and a scene's clearances (rt_scene_separation /
// rt_scene_separation_buffer / rt_scene_separation_self / rt_scene_separation_self_buffer / rt_debug_separation / rt_debug_separation_walk /
// rt_debug_separation_self).  The rule is separation.h's.  A translation unit and a device code object of its own, like cross.hip: the
// hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace separation
{
// The walk's launch on `stream`, nothing waited for: k_separation over d_probes[n] (the 4-wide records when use_wide, the child-pair records otherwise).
// The stack spill area and the status word are the ray queries' (q), grown or allocated here as query::launch does.  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_probe* d_probes, uint32_t n, float max_distance,
    rt_separation* d_out);

// The same where probe i is scene triangle first + i.  d_object_of_triangle: the device table of rt_scene_set_objects when options has
// RT_SEPARATION_OTHER_OBJECTS, else nullptr.
bool launch_self(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const uint32_t* d_object_of_triangle, uint32_t first,
    uint32_t n, float max_distance, uint32_t options, rt_separation* d_out);

// rt_debug_separation / rt_debug_separation_self: brute force over all triangles, on the host or by k_separation_brute on uploaded copies.  probes == nullptr:
// the self form (probe i is tris[first + i]; ids: the objects' table when options has RT_SEPARATION_OTHER_OBJECTS).
void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, float max_distance, uint32_t options,
    rt_separation* out);
bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n,
    float max_distance, uint32_t options, rt_separation* out);

// rt_debug_separation_walk: k_separation's walk on the host.  nullptr, or why the walk was refused.
const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_probe* probes, uint32_t n,
    float max_distance, rt_separation* out, uint32_t* tested);
} // namespace separation
