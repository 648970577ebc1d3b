// morph_host.h -- the interface of morph.hip: the scene's triangles morphed on the device from one weight per morph target, alone or fused with the skin
// (rt_scene_set_morph / rt_scene_morph / rt_scene_morph_skin), and the host restatement of the same rule (rt_debug_morph's oracle side).
// The arithmetic itself is morph.h's.  A translation unit and a device code object of its own, like skin.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "rt_hip.h"          // rt_morph_delta, rt_skin_influence
#include "rt_types.h"
#include "moved.h"           // moved::Stage

namespace morph
{
struct Record;               // morph.h: one delta of one target at one corner, 32 bytes
// what rt_scene_set_morph keeps beside the scene: per triangle the rest pose in rt_triangle layout (160 bytes), the staging area a morph is written to before
// the refit reads it (160) and one word of the row table (4); per delta one record (32); per target one weight (4)
enum { REST_BYTES = moved::REST_BYTES, STAGED_BYTES = moved::STAGED_BYTES, ROW_BYTES = 4, RECORD_BYTES = 32, WEIGHT_BYTES = 4 };
// up to LDS_TARGETS weights are staged in LDS once per block by k_morph_triangles (4 KB: with the 40 KB tile, three blocks per CU); more are gathered through
// the vector L1 / L2
enum { MAX_TARGETS = 65536, LDS_TARGETS = 1024 };
// a corner index 3 * triangle + c is 32 bits
enum : uint32_t { MAX_TRIANGLES = 0xFFFFFFFFu / 3u };

struct State
{
    uint32_t n_targets = 0, n_deltas = 0;
    moved::Stage stage;                  // the pose rt_scene_set_morph saw; the kernels' output, refit_device's input
    uint32_t* row = nullptr;             // stage.n_tris + 1: triangle i owns records[row[i] .. row[i + 1])
    Record* records = nullptr;           // n_deltas, by triangle, then target, then corner
    float* weights = nullptr;            // n_targets on the device ...
    float* host_weights = nullptr;       // ... and in pinned host memory, filled by every morph
    size_t bytes = 0;
};

// what is wrong with a table of targets, the first offence in array order (the offsets first, then the deltas target by target)
// (NO_MEMORY: the check's own table of 3 * nt words could not be allocated on the host)
enum Fault { TABLE_OK = 0, FIRST_OFFSET, DECREASING_OFFSET, BAD_CORNER, NOT_FINITE, BAD_PAD, TWICE, NO_MEMORY };
Fault table_fault(const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt);
bool weights_finite(const float* weights, uint32_t n_targets);
// a checked table by triangle: row[nt + 1] and the records sorted by triangle, then target, then corner.  false: no host memory for them
bool transpose(const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt, std::vector<uint32_t>& row, std::vector<Record>& records);

// everything a morph needs, allocated here so that a morph allocates nothing; the rest pose is moved::Stage::arm's.  Waits for the stream.
// false: an allocation, a copy or the launch failed, and st is released
bool arm(hipStream_t stream, State& st, const float4* tris_sh, const std::vector<uint32_t>& row, const std::vector<Record>& records, uint32_t nt, uint32_t n_targets);
void release(State& st);
// the weights uploaded, then k_morph_triangles: rest -> staged.  Nothing is waited for.
bool run(hipStream_t stream, State& st, const float* weights);
// the weights uploaded, then k_morph_skin_triangles with the skin's influences and its palette as skin::upload_palette left it: rest -> staged
bool run_skin(hipStream_t stream, State& st, const float* weights, const rt_skin_influence* d_influences, const float* d_palette, uint32_t n_bones);

// rt_debug_morph: out[nt] = rest[nt] morphed, on the host (the restatement; false: no host memory for the rows) or by k_morph_triangles on uploaded copies.
// The table has been checked.
bool debug_host(const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt, const float* weights, rt_triangle* out);
bool debug_device(hipStream_t stream, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt,
    const float* weights, rt_triangle* out);
// rt_debug_morph_skin's device side: k_morph_skin_triangles on uploaded copies (the host side is debug_host, then skin::debug_host)
bool debug_skin_device(hipStream_t stream, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt,
    const float* weights, const rt_skin_influence* per_corner, const float* matrices3x4, uint32_t n_bones, rt_triangle* out);
} // namespace morph
