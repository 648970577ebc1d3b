// wide_bvh.h -- the host side of the backend's tree work (wide_bvh.cpp; no device code, no HIP runtime): the fold of a binary BVH into the 4-wide
// records of k_trace_w4 (build_wide_bvh: the specification of device_fold.hip's kernels, their fallback and the tests' oracle), the pair layout of the
// records, the shadow rays' metric, and the host walks of a fold adaptation (crossing counts, nearest occluders, slot order).  Split out of rt_hip.hip
// in round 6 (one 3 600-line translation unit): a change here re-links the library without touching the hot path's code object.
#pragma once
#include <stdint.h>
#include <atomic>
#include <utility>
#include <vector>
#include <hip/hip_vector_types.h>      // float4 (the probe rays travel as the kernels' own queues)
#include "rt_types.h"
#include "wide_node.h"
#include "own_bvh.h"

namespace rtw
{
enum { RT_WIDE_TWO_LEVELS = 0, RT_WIDE_SAH = 1 };
// record levels a fold may have (the entry's record is level 1): three pending slots per level must fit RT_W4_STACK_MAX (trace_kernels.h)
enum : uint32_t { RT_WIDE_MAX_LEVELS = 33u };

// false: the tree does not qualify (non-finite or non-nested bounds, child order, too deep for the kernel's stack): k_trace2 is used
bool build_wide_bvh(const rt_bvh_node* nodes, uint32_t nn, int collapse, std::vector<WideNode>& out, uint32_t& entry_ref,
    std::vector<uint32_t>* roots = nullptr /* the BVH2 node each record folds (tests) */,
    const ownbvh::Metric* metric = nullptr /* what "area" means for the SAH collapse (own_bvh.h); nullptr = surface area */,
    const double* weights = nullptr /* per BVH2 node: replaces the area altogether (a MEASURED visit frequency: FoldAdapt) */,
    const std::atomic<bool>* cancel = nullptr /* set by another thread: give up (false) at the next check -- a scene uploaded again does not wait */,
    unsigned threads = 0 /* 0 = the host's (at most 32; 16 with weights); the records do not depend on it */);

// RT_CTX_OPT_WIDE_LAYOUT = 1: the records permuted into (parent, likeliest child) pairs, one pair per 128-byte line; weight[record] = the visit weight of
// the box the record tests (by OLD record index); roots (optional) is permuted along
void pair_layout(std::vector<WideNode>& wide, std::vector<uint32_t>* roots, const std::vector<double>& weight);
// ... by the area (the own trees: their metric) of the records' boxes, or by per-NODE weights (an adaptation's measured crossings)
void pair_layout_by_area(std::vector<WideNode>& wide, std::vector<uint32_t>& roots, const rt_bvh_node* nodes, uint32_t nn, const ownbvh::Metric* metric);
void pair_layout_by_node_weights(std::vector<WideNode>& wide, std::vector<uint32_t>& roots, const double* node_weights, uint32_t nn);

// ---- records that come from outside (rt_scene_import_folds, rt_debug_check_folds): are they a tree over the scene's leaves that the walks can take? ----
// The first triangles of a scene's leaves: one bit per triangle, and -- for a node array in which several leaf nodes begin at the same triangle, which the
// reference's builder never makes but an upload does not refuse -- how many leaves begin there.
struct LeafStarts
{
    std::vector<uint64_t> bits;                                   // bit t: a leaf begins at triangle t
    std::vector<std::pair<uint32_t, uint32_t>> shared;            // (triangle, leaves that begin there) where that is more than one, sorted by triangle
    uint32_t n_tris = 0, distinct = 0;                            // distinct: bits set
    bool is_start(uint32_t t) const { return t < n_tris && ((bits[t >> 6] >> (t & 63u)) & 1u) != 0u; }
};
// from the binary tree's leaf nodes (a leaf that begins at or beyond n_tris is left out: nothing can refer to it)
LeafStarts leaf_starts(const rt_bvh_node* nodes, uint32_t nn, uint32_t n_tris);

// What is wrong with a record array, in the order the classes are looked for: the first class in this order that applies to the array is its defect, whichever
// record shows it, so the answer does not depend on the order of a walk.
enum class FoldDefect
{
    NONE = 0,
    ENTRY,            // the entry is not a record of the array; without records: not a leaf ref
    REF_RANGE,        // some record's ref, reached or not, lies outside the records / the triangles
    REACHED_TWICE,    // a record is reached through two slots: a cycle, a self-reference, a shared record
    TOO_DEEP,         // more record levels than build_wide_bvh allows (RT_W4_STACK_MAX is sized from them)
    SLOT_COUNT,       // meta >> 24 of a reached record is not the number of its non-empty refs, or not in 2 .. 4
    FRAME,            // a reached record's origin is not finite or beyond 2^28, a cell exponent outside wide_frame's range
    LEAF_NOT_A_START, // a reached leaf ref is not the first triangle of a leaf of the scene
    LEAF_TWICE,       // a leaf of the scene is reached more often than the scene has it
    LEAF_MISSING      // ... or less often
};
const char* fold_defect_text(FoldDefect d);
// Iterative (a chain or a cycle of any length costs heap, not stack); records that the entry does not reach are tolerated, their refs are still range-checked.
FoldDefect check_fold(const WideNode* recs, uint32_t n, uint32_t entry, const LeafStarts& leaves);

ownbvh::Metric shadow_metric(const rt_light* lights, uint32_t n, double iso_share);

// host threads one side of an adaptation may use beside the render loop
unsigned adapt_threads(size_t work_items, size_t per_thread);
// host walks (weights only) that met a binary tree deeper than their stack since the last call (read-and-clear) / add to it
uint64_t truncated_walks_exchange();
void truncated_walks_add(uint64_t n);

void count_box_passes(const rt_bvh_node* nodes, uint32_t nn, const float4* o, const float4* d, size_t n_rays, std::vector<uint32_t>& counts, const std::atomic<bool>& cancel,
    std::atomic<uint64_t>* truncated = nullptr /* walks cut short (RT_COUNT_STACK, wide_node.h) are counted here; NULL: in truncated_walks_exchange()'s counter */);
void nearest_occluders(const std::vector<rt_bvh_node>& tree, const std::vector<float>& tri9, const std::vector<float4>& o, const std::vector<float4>& d,
    std::vector<uint32_t>& prim, const std::atomic<bool>& cancel);
uint32_t occluder_first(std::vector<WideNode>& wide, const std::vector<uint32_t>& roots, const std::vector<rt_bvh_node>& tree, const std::vector<uint32_t>& prim);
} // namespace rtw
