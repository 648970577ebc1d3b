// refit.h -- the interface of refit.hip: the scene's trees refitted on the device when its triangles move (rt_scene_refit), and the host
// restatement of the same rule (rt_debug_refit's oracle side).  A translation unit and a device code object of its own, like device_fold.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <string>
#include "rt_types.h"
#include "wide_node.h"

namespace refit
{
enum { OK = 0, BAD_POSITION = 1, BAD_MATERIAL = 2, NOT_A_TREE = 3 };

// one 4-wide tree of the scene and what a refit keeps for it: the record that holds each record (parent << 2 | slot), the exact box of every record
// (8 floats: min.xyz, -, max.xyz, -), arrival counters
struct Tree
{
    WideNode* records = nullptr; uint32_t n = 0, entry = 0;
    uint32_t* parent = nullptr; float* boxes = nullptr; uint32_t* arrived = nullptr;
    const void* linked_for = nullptr; uint32_t linked_n = 0;        // the records the links were made for (an adopted or imported fold replaces them)
};

// what RT_CTX_OPT_REFITTABLE keeps beside the scene
struct State
{
    uint32_t n_pairs = 0;                                           // child-pair records, the super-root included
    uint32_t* pair_parent = nullptr; uint32_t* pair_arrived = nullptr;
    Tree trees[2];                                                  // wnodes, wnodes_sh
    int* d_status = nullptr;                                        // [0] validation, [1] the climb's guard, [2], [3] a record of tree 0 / 1 that does not qualify
    size_t bytes = 0;
};

struct Result { int error = OK; bool wide_bad[2] = {false, false}; float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0}; };

// what a refit asks of the node array at upload: the leaves are consecutive ranges that cover the triangle array (a leaf is found again as a run of records)
bool leaves_partition(const rt_bvh_node* nodes, uint32_t nn, uint32_t nt);
// links of the child-pair records (made once: a refit never moves them); false: an allocation or a launch failed
bool prepare(hipStream_t stream, State& st, const float4* pairs, uint32_t n_pairs);
// links of one 4-wide tree, made again when the scene holds other records than last time; records == nullptr releases them
bool link_tree(hipStream_t stream, State& st, int which, WideNode* records, uint32_t n, uint32_t entry);
void release(State& st);

// read-only: a non-finite position or mtl_index >= num_materials -> BAD_POSITION / BAD_MATERIAL (the stream is waited for)
int validate(hipStream_t stream, State& st, const rt_triangle* d_tris, uint32_t nt, uint32_t num_materials);
// the refit: triangle records and leaf boxes, child-pair records bottom-up, every linked 4-wide tree; waits for the stream.  false: a launch or a copy failed
bool run(hipStream_t stream, State& st, const rt_triangle* d_tris, uint32_t nt, float4* tris_rt, float4* tris_sh, float4* pairs, uint32_t super_root, Result& out);

// rt_debug_refit: a reference-layout node array and any fold of it, refitted to `tris` -- on the host (the restatement) or through the kernels above.
// out_nodes[nn], out_records[n_records] (either may be NULL); *wide_bad = a record no longer qualifies (its bytes are then left as they were).
bool debug_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t nt, const WideNode* records, uint32_t n_records, uint32_t entry,
    rt_bvh_node* out_nodes, WideNode* out_records, bool* wide_bad, std::string& error);
bool debug_device(hipStream_t stream, const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t nt, const WideNode* records, uint32_t n_records, uint32_t entry,
    rt_bvh_node* out_nodes, WideNode* out_records, bool* wide_bad, std::string& error);
} // namespace refit
