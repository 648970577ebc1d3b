// region_host.h -- the interface of region.hip: every triangle a caller's convex region touches or encloses (rt_scene_overlap / rt_scene_overlap_buffer /
// rt_scene_select / rt_scene_select_buffer / rt_frame_pick_rect / rt_debug_overlap / rt_debug_overlap_walk / rt_debug_select / rt_debug_rect_region, DESIGN.md
// section 7m).  The rule is region.h's.  A translation unit and a device code object of its own, like within.hip: the hot path's code object (rt_hip.hip) is
// neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "query_host.h"

struct DScene;

namespace region
{
// The walk's launch on `stream`, nothing waited for: k_region over d_regions[n] (the 4-wide records when use_wide, the child-pair records otherwise).
// d_members may be nullptr (only d_out is written).  The stack spill area and the status word are the ray queries' (q), grown or allocated here as
// query::launch does.  false: an allocation or a launch failed.
bool launch(hipStream_t stream, query::Scratch& q, const DScene& sc, bool use_wide, int compute_units, const rt_region* d_regions, uint32_t n, uint32_t max_list,
    rt_region_hits* d_out, rt_region_member* d_members);

// The select's launches on `stream`, nothing waited for: the per-object words zeroed, k_select over the scene's shading records, k_select_finish.  Any output may
// be nullptr; the per-object ones need d_object_of_triangle.  The finishing step's word per object lives in q's staging array 3, grown here.
bool select(hipStream_t stream, query::Scratch& q, const DScene& sc, uint32_t n_tris, const uint32_t* d_object_of_triangle, uint32_t n_objects,
    const rt_region* d_regions, uint32_t n, uint32_t* d_touching, uint32_t* d_inside, uint32_t* d_object_touching, uint32_t* d_object_inside);

// rt_debug_overlap: brute force over all triangles, on the host or by k_region_brute on uploaded copies.  members may be nullptr when max_list == 0.
void brute_host(const rt_triangle* tris, uint32_t n_tris, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members);
bool brute_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out,
    rt_region_member* members);

// rt_debug_overlap_walk: k_region's walk on the host.  nullptr, or why the walk was refused.
const char* walk_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t n_tris, bool wide, const rt_region* regions, uint32_t n,
    uint32_t max_list, rt_region_hits* out, rt_region_member* members, uint32_t* tested);

// rt_debug_select: region.h per triangle on the host, or k_select on uploaded copies.  ids may be nullptr (the per-object outputs are then not written).
void select_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* ids, uint32_t n_objects, const rt_region* regions, uint32_t n, uint32_t* touching,
    uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside);
bool select_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* ids, uint32_t n_objects, const rt_region* regions, uint32_t n,
    uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside);

// why the inclusive pixel rectangle (x0, y0) .. (x1, y1) of a width x height image is refused (nullptr: it is fine), for rt_frame_pick_rect and rt_debug_rect_region
const char* rect_refused(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
// ... and its region: region.h's region_of_rect
rt_region rect_region(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far);
} // namespace region
