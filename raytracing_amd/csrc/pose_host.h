// pose_host.h -- the interface of pose.hip: the scene's objects posed on the device from one 3x4 matrix per object (rt_scene_set_objects / rt_scene_pose,
// DESIGN.md section 7g), and the host restatement of the same rule (rt_debug_pose's oracle side).  The arithmetic itself is pose.h's.  A translation unit and a
// device code object of its own, like refit.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_types.h"
#include "moved.h"           // moved::Stage

namespace pose
{
// what rt_scene_set_objects keeps beside the scene, per triangle: the rest pose in rt_triangle layout (160 bytes), its object (4) and the staging area a pose
// is written to before the refit reads it (160)
enum { REST_BYTES = moved::REST_BYTES, ID_BYTES = 4, STAGED_BYTES = moved::STAGED_BYTES, BYTES_PER_TRIANGLE = REST_BYTES + ID_BYTES + STAGED_BYTES };

struct State
{
    uint32_t n_objects = 0;
    moved::Stage stage;                  // the pose rt_scene_set_objects saw; k_pose_triangles' output, refit_device's input
    uint32_t* ids = nullptr;             // object of every triangle
    void* objects = nullptr;             // pose::Object[n_objects] on the device ...
    void* host_objects = nullptr;        // ... and in pinned host memory, filled by every pose
    size_t bytes = 0;
};

bool ids_in_range(const uint32_t* ids, uint32_t nt, uint32_t n_objects);
bool matrices_finite(const float* matrices3x4, uint32_t n_objects);

// everything a pose needs, allocated here so that a pose allocates nothing; the rest pose is moved::Stage::arm's.  Waits for the stream.
// false: an allocation, a copy or the launch failed, and st is released
bool arm(hipStream_t stream, State& st, const float4* tris_sh, const uint32_t* ids, uint32_t nt, uint32_t n_objects);
void release(State& st);
// the per-object terms on the host, uploaded, then k_pose_triangles: rest -> staged.  Nothing is waited for.
bool run(hipStream_t stream, State& st, const float* matrices3x4);

// rt_debug_pose: out[nt] = rest[nt] posed, on the host (the restatement) or by k_pose_triangles on uploaded copies
void debug_host(const rt_triangle* rest, const uint32_t* ids, uint32_t nt, const float* matrices3x4, uint32_t n_objects, rt_triangle* out);
bool debug_device(hipStream_t stream, const rt_triangle* rest, const uint32_t* ids, uint32_t nt, const float* matrices3x4, uint32_t n_objects, rt_triangle* out);
} // namespace pose
