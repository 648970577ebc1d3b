// query_host.h -- the interface of query.hip: caller-supplied rays traced against the uploaded scene (rt_scene_trace / rt_scene_trace_buffer / rt_frame_pick /
// rt_debug_query_surface).  The surface arithmetic itself is query.h's.  A translation unit and a device code object of its own, like
// pose.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"
#include "device_memory.h"

struct DScene;

namespace query
{
enum { CHUNK_RAYS = 4u << 20 };          // rt_scene_trace stages at most this many rays at a time

// what a context keeps for its queries: the walk's stack spill area (sized by the grid), a status word, and the host forms' staging arrays (grown on demand).
// A context has two: one for its ray and nearest-point queries, which owns the status word, and one for its bakes (stages 0 and 1, no status word of its own).
struct Scratch
{
    uint2* spill = nullptr; uint32_t spill_blocks = 0;
    uint32_t* status = nullptr;                         // pinned host memory the kernel can write; bit 0: a traversal stack ran over its bound (walk_kernels.h)
    void* stage[4] = {nullptr, nullptr, nullptr, nullptr};   // rays | points, hits | records | results, occluded, surfaces
    size_t stage_bytes[4] = {0, 0, 0, 0};
    size_t bytes() const;          // the device memory above
    size_t spill_bytes() const;
};
void release(Scratch& s);
// stage[k] holds at least `bytes` (the stream is waited for before a smaller array is freed); false: out of device memory
bool reserve(hipStream_t stream, Scratch& s, int k, size_t bytes);

// Before a walk's launch: *status is allocated if it is not yet, s's spill area is grown to the grid (the stream is waited for before a smaller one is freed).
// The grid: n_groups blocks of one wave, at most what waves_per_cu keeps resident (rounded up to 8).  0: out of memory.
uint32_t prepare(hipStream_t stream, Scratch& s, uint32_t** status, int compute_units, uint32_t waves_per_cu, uint32_t n_groups);

// The query's launches on `stream`, nothing waited for: k_query_trace over d_rays[n], then k_query_surface when d_surfaces is given.  mode: RT_QUERY_*; use_wide:
// the scene's 4-wide trees are usable; object_of_triangle: the device table of rt_scene_set_objects or nullptr.  In closest mode d_hits may be nullptr when
// d_surfaces is given (the hits then pass through the surfaces' own memory).  compute_units sizes the grid.  false: the spill area could not be allocated or a launch failed.
bool launch(hipStream_t stream, Scratch& s, const DScene& sc, bool use_wide, uint32_t n_tris, const uint32_t* object_of_triangle, int compute_units,
    const rt_ray* d_rays, uint32_t n, uint32_t mode, rt_hit* d_hits, uint32_t* d_occluded, rt_surface* d_surfaces);

// rt_frame_pick's ray: from cam.position through the centre of pixel (x, y) of a width x height image -- sf_guide_dir, the guide pass's direction -- t_min 0,
// t_max RT_MAX_RENDER_DIST
rt_ray pick_ray(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y);

// rt_debug_query_surface: query.h's arithmetic over caller triangles, on the host or by k_query_surface on uploaded copies
void debug_surface_host(const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits, uint32_t n, rt_surface* out);
bool debug_surface_device(hipStream_t stream, const rt_triangle* tris, uint32_t n_tris, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits,
    uint32_t n, rt_surface* out);
} // namespace query
