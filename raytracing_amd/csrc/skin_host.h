// skin_host.h -- the interface of skin.hip: the scene's triangles skinned on the device from a palette of bone matrices (rt_scene_set_skin / rt_scene_skin,
// DESIGN.md section 7p), and the host restatement of the same rule (rt_debug_skin's oracle side).  The arithmetic itself is skin.h's.  A translation unit and a
// device code object of its own, like pose.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include "rt_hip.h"          // rt_skin_influence
#include "rt_types.h"
#include "moved.h"           // moved::Stage

namespace skin
{
// what rt_scene_set_skin keeps beside the scene, per triangle: the rest pose in rt_triangle layout (160 bytes), the three corners' influences (72) and the
// staging area a skin is written to before the refit reads it (160)
enum { REST_BYTES = moved::REST_BYTES, INFLUENCE_BYTES = 72, STAGED_BYTES = moved::STAGED_BYTES, BYTES_PER_TRIANGLE = REST_BYTES + INFLUENCE_BYTES + STAGED_BYTES };
// a palette of up to LDS_BONES matrices is staged in LDS once per block (48 bytes each); a larger one is gathered through the vector L1 / L2
enum { MAX_BONES = 65536, LDS_BONES = 128, MATRIX_BYTES = 48 };

struct State
{
    uint32_t n_bones = 0;
    moved::Stage stage;                  // the pose rt_scene_set_skin saw; k_skin_triangles' output, refit_device's input
    rt_skin_influence* influences = nullptr;   // three per triangle
    float* palette = nullptr;            // n_bones 3x4 matrices on the device ...
    float* host_palette = nullptr;       // ... and in pinned host memory, filled by every skin
    size_t bytes = 0;
};

// 0: every bone index is below n_bones and every weight finite; 1: a bone index is not; 2: a weight is not (the first offence in array order decides)
int influences_fault(const rt_skin_influence* per_corner, uint32_t nt, uint32_t n_bones);
bool matrices_finite(const float* matrices3x4, uint32_t n_bones);

// everything a skin needs, allocated here so that a skin allocates nothing; the rest pose is moved::Stage::arm's.  Waits for the stream.
// false: an allocation, a copy or the launch failed, and st is released
bool arm(hipStream_t stream, State& st, const float4* tris_sh, const rt_skin_influence* per_corner, uint32_t nt, uint32_t n_bones);
void release(State& st);
// the palette into its pinned host copy and from there to the device, and no launch (rt_scene_morph_skin's kernel reads it: morph.hip).  Nothing is waited for.
bool upload_palette(hipStream_t stream, State& st, const float* matrices3x4);
// the palette uploaded, then k_skin_triangles: rest -> staged.  Nothing is waited for.
bool run(hipStream_t stream, State& st, const float* matrices3x4);

// rt_debug_skin: out[nt] = rest[nt] skinned, on the host (the restatement) or by k_skin_triangles on uploaded copies
void debug_host(const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t nt, const float* matrices3x4, uint32_t n_bones, rt_triangle* out);
bool debug_device(hipStream_t stream, const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t nt, const float* matrices3x4, uint32_t n_bones, rt_triangle* out);
} // namespace skin
