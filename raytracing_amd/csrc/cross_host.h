// cross_host.h -- the interface of cross.hip: every scene triangle a caller's triangle crosses, and a scene's self-crossings (rt_scene_cross /
// rt_scene_cross_buffer / rt_scene_cross_self / rt_scene_cross_self_buffer / rt_debug_cross / rt_debug_cross_walk / rt_debug_cross_self, DESIGN.md section
// 7n).  The rule is cross.h's.  A translation unit and a device code object of its own, like region.hip: the hot path's code object (rt_hip.hip) is neither
// rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace cross
{
// The walk's launch on `stream`, nothing waited for: k_cross over d_probes[n] (the 4-wide records when use_wide, the child-pair records otherwise).
// d_members may be nullptr (only d_out is written).  options: RT_CROSS_ANY or 0.  The stack spill area and the status word are the ray queries' (q), grown
// or allocated here as query::launch does.  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_probe* d_probes, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* d_out, rt_cross_member* d_members);

// The same for k_cross_self: probe i is scene triangle first + i.  d_object_of_triangle: the device table of rt_scene_set_objects when options has
// RT_CROSS_OTHER_OBJECTS, else nullptr.
bool launch_self(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const uint32_t* d_object_of_triangle, uint32_t first,
    uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* d_out, rt_cross_member* d_members);

// rt_debug_cross / rt_debug_cross_self: brute force over all triangles, on the host or by k_cross_brute on uploaded copies.  probes == nullptr: the self form
// (probe i is tris[first + i]; ids: the objects' table when options has RT_CROSS_OTHER_OBJECTS).  members may be nullptr when max_list == 0.
void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options,
    rt_probe_hits* out, rt_cross_member* members);
bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_probe* probes, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* out, rt_cross_member* members);

// rt_debug_cross_walk: k_cross's walk on the host.  nullptr, or why the walk was refused.
const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_probe* probes, uint32_t n, uint32_t max_list,
    uint32_t options, rt_probe_hits* out, rt_cross_member* members, uint32_t* tested);
} // namespace cross
