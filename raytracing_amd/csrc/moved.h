// moved.h -- the interface of moved.hip: the rest pose and the staging area that every producer of moved triangles (pose.hip, skin.hip, morph.hip) keeps beside
// the scene, and the one kernel that makes a rest pose.  A translation unit and a small device code object of its own.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include "rt_types.h"

namespace moved
{
enum { REST_BYTES = 160, STAGED_BYTES = 160 };   // per triangle: both are rt_triangle arrays

// One producer's own: its rest pose is the scene as it stood at ITS rt_scene_set_*.
struct Stage
{
    uint32_t n_tris = 0;
    rt_triangle* rest = nullptr;         // the pose rt_scene_set_* saw
    rt_triangle* staged = nullptr;       // the producer's kernel writes it, refit_device reads it
    // both allocated and k_rest_pose launched on `stream`; the caller waits for the stream with its own copies.  false: an allocation or the launch failed, no
    // HIP error is left pending and the Stage holds nothing
    bool arm(hipStream_t stream, const float4* tris_sh, uint32_t nt);
    void release();
};
} // namespace moved
