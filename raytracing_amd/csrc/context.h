// context.h -- what a context is, for the translation units that implement entry points on it (context.cpp, scene_upload.cpp, scene_moved.cpp, scene_queries.cpp,
// and through frame.h the frames' units and rt_hip.hip): the uploaded scene and its trees, the context and the buffer records behind the C-ABI's opaque handles,
// how an entry point fails, and the device copies an upload makes.  Internal: never installed, never included by include/.  A feature unit gets the scene
// (ctx->scene: the kernels' view `d`, the trees, the objects' table), the queries' scratch areas, the stream, the device and its properties.  It may ask for
// everything in flight to drain before it frees or rewrites what a launch could still read (quiesce).  It cannot see a frame through this header: what a frame
// is, for the units that implement entry points on one, is frame.h's (quiesce is context.cpp's, on frame.h's ahead_discard and sync_frame_streams) -- nor the
// fold adaptation's state, which is a name only here (fold_adapt.h, for the units that work on it).  context.cpp owns the records' life, the thread's message,
// the context's options and the buffers; the two launches a context needs of the hot path's code object (relayout_records, fill_gamma_lut) are rt_hip.hip's.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <utility>
#include <vector>
#include "rt_hip.h"
#include "device_scene.h"    // DScene, the kernels' view of a scene (a Scene holds one by value)
#include "refit.h"           // refit::State
#include "pose_host.h"       // pose::State
#include "skin_host.h"       // skin::State
#include "morph_host.h"      // morph::State
#include "query_host.h"      // query::Scratch
#include "bake_host.h"       // bake::CHUNK_POINTS
#include "device_memory.h"   // dev::Mem

namespace rtw { struct LeafStarts; }        // the first triangles of a scene's leaves (wide_bvh.h)

namespace context
{
struct FoldAdapt;                          // RT_CTX_OPT_ADAPTIVE_FOLD: the state of a scene's fold adaptation (fold_adapt.h)

// One 4-wide quantized tree on the device: its records (whoever holds the value owns them), how many (0 with a leaf root), the record a walk enters at.
struct WideTree { void* recs = nullptr; uint32_t n = 0, entry = 0; };
// The trees a scene can hold: the fold of the reference's tree (build_wide_bvh / devfold::fold; no records when the tree does not qualify), the shadow rays'
// own (own_bvh.h over the reference's leaves) and, RT_CTX_OPT_CLOSEST_TREE != 0 (tolerance mode), the closest-hit rays' own.
enum TreeSlot { TREE_REF = 0, TREE_SHADOW = 1, TREE_CLOSEST = 2 };

struct Scene
{
    void* nodes = nullptr; void* tris_rt = nullptr; void* tris_sh = nullptr; void* materials = nullptr;
    void* textures = nullptr; void* texture_data = nullptr; void* lights = nullptr; void* env = nullptr;
    void* emissive = nullptr;
    void* mat_tex16 = nullptr;
    WideTree trees[3];                                           // by TreeSlot
    TreeSlot closest = TREE_REF, shadow = TREE_REF;              // which of them each ray population walks; an own tree is held exactly while its population walks it
    const WideTree &closest_tree() const { return trees[closest]; }
    const WideTree &shadow_tree() const { return trees[shadow]; }
    bool shadow_shares_closest() const { return shadow == closest; }     // the shadow rays walk the closest-hit rays' records
    // The only writer of the kernels' view of the trees (d.wnodes, d.w_entry_ref, d.wnodes_sh, d.w_sh_entry_ref): the two operations below end with it.
    void publish_trees()
    {
        d.wnodes = (const float4*)closest_tree().recs; d.w_entry_ref = closest_tree().entry;
        d.wnodes_sh = (const float4*)shadow_tree().recs; d.w_sh_entry_ref = shadow_tree().entry;
    }
    // `slot` holds `tree` from now on; what it held goes back to the caller, who frees it or keeps it until nothing in flight reads it (FoldAdapt::retired)
    WideTree replace_tree(TreeSlot slot, WideTree tree) { std::swap(trees[slot], tree); publish_trees(); return tree; }
    void walk_trees(TreeSlot closest_rays, TreeSlot shadow_rays) { closest = closest_rays; shadow = shadow_rays; publish_trees(); }
    uint32_t n_tris = 0;         // triangles of the uploaded scene (rt_scene_import_folds checks leaf refs against it)
    // the first triangles of the scene's leaves, one bit per triangle (wide_bvh.h; filled at upload from the nodes, freed by free_scene, left alone by a refit:
    // the topology does not change): what rt_scene_import_folds checks the leaf refs of imported records against
    rtw::LeafStarts* leaf_starts = nullptr;
    std::string tree_report;     // what rt_scene_upload measured when it chose the trees (rt_scene_tree_report)
    FoldAdapt* adapt = nullptr;  // RT_CTX_OPT_ADAPTIVE_FOLD: armed at upload, run by the first rt_integrate (fold_adapt_hook)
    DScene d = {};
    bool valid = false;
    bool wide_ok = false;     // build_wide_bvh succeeded (k_trace_w4 usable)
    bool offsets32 = false;   // node and trace-triangle arrays below 4 GiB: k_trace2 addresses them with 32-bit byte offsets
    // a quarter or more of the shadow rays will have a non-finite 1/dir component (directional lights along a coordinate
    // axis, e.g. an overhead light (0, -1, 0)): k_trace_w4 would hand every one of them to its small follow-up launch,
    // so the automatic choice traces the shadow queue with k_trace2 (select-form slab test inline, full residency)
    bool slow_shadow = false;
    // RT_CTX_OPT_REFITTABLE (scene_upload.cpp): what rt_scene_refit keeps beside the scene; nullptr = the option was off at upload (or refit_refusal says why not)
    refit::State* refit = nullptr;
    std::string refit_refusal;
    bool refit_wide_built = false;   // wide_ok as upload left it (a refit that meets a record that no longer qualifies clears wide_ok until one qualifies again)
    bool adapt_retired = false;      // a refit has retired the fold adaptation
    uint32_t n_materials = 0;
    uint64_t refits = 0;
    // RT_CTX_OPT_REFIT_MOTION: the pose before the last refit, 6 float4 per triangle (filt::snapshot_pose); nullptr = the option was off at upload (or the
    // allocation failed: treated as off).  pose_valid: a refit has filled it.
    void* pose_snap = nullptr;
    bool pose_valid = false;
    // rt_scene_set_objects (scene_moved.cpp): the rest pose, every triangle's object and the staging area of rt_scene_pose; nullptr = no objects set
    pose::State* pose = nullptr;
    // rt_scene_set_skin (scene_moved.cpp): the rest pose, every corner's influences, the palette and the staging area of rt_scene_skin; nullptr = no skin set
    skin::State* skin = nullptr;
    // rt_scene_set_morph (scene_moved.cpp): the rest pose, the targets' records by triangle, the weights and the staging area of rt_scene_morph / _morph_skin; nullptr = no morph set
    morph::State* morph = nullptr;
};
} // namespace context

struct rt_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
    std::string error;
    context::Scene scene;
    uint32_t treelet_nodes = 7;   // RT_CTX_OPT_TREELET_NODES
    uint32_t build_wide = 1;      // RT_CTX_OPT_WIDE_BVH
    uint32_t shadow_tree = 1;     // RT_CTX_OPT_SHADOW_TREE: 1 = shadow rays walk the backend's own tree where it measures cheaper (exact either way),
                                  // 2 = own unconditionally, 3 = own with the surface-area metric (A/B), 0 = they share the closest-hit tree
    uint32_t closest_tree = 0;    // RT_CTX_OPT_CLOSEST_TREE: 1 / 2 as above; != 0 is the tolerance mode (NOT bit-exact)
    uint32_t adaptive_fold = 25;  // RT_CTX_OPT_ADAPTIVE_FOLD (default bits 0 + 3 + 4 since round 5): bit 0 = re-fold the 4-wide trees for the rays rt_integrate actually traces (exact: a fold
                                  // decides which boxes are tested, never a result), bit 1 = rt_integrate waits for the new fold instead of
                                  // adopting it when it is ready, bit 2 = also for scenes too small to profit (tests), bit 3 = the shadow rays'
                                  // binary tree is rotated for the probe rays' crossings before it is folded (tree_rotate.h), bit 4 = the slots of
                                  // every shadow record are stored likeliest occluder first (measured on the device in round 5, profiles/r05_call01_*:
                                  // shadow trace 0.314 -> 0.258 ms per sample on the headline scene, bit-identical on all five configs)
    uint32_t adapt_min_interval_ms = 500;   // RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS
    uint32_t wide_layout = 0;               // RT_CTX_OPT_WIDE_LAYOUT: 1 = the 4-wide records stored in (parent, likeliest child) pairs, one pair per 128-byte line (pair_layout)
    uint32_t tree_builder = 2;              // RT_CTX_OPT_TREE_BUILDER: the shadow rays' own binary tree -- 0 = own_bvh.h's full-sweep SAH on host threads, 1 = PLOC on the device (ploc_kernels.h),
                                            // 2 (default) = both start, the device's is measured first and the host's build is abandoned if it wins its measurement
    uint32_t refittable = 0;                // RT_CTX_OPT_REFITTABLE: rt_scene_upload keeps what rt_scene_refit needs (refit.h)
    uint32_t device_fold = 1;               // RT_CTX_OPT_DEVICE_FOLD: the SAH collapse into 4-wide records runs on the device (fold_kernels.h); 0 = on host threads
    uint32_t refit_motion = 0;              // RT_CTX_OPT_REFIT_MOTION: a refit keeps the pose it replaces, for the temporal filter (needs refittable)
    uint64_t scene_uploads = 0;             // rt_scene_upload calls so far (what a frame's measured choices were made for)
    uint64_t upload_epoch = 0;              // changes on rt_scene_upload only; refit_index: the successful refits within it.  A temporal history made for
    uint64_t refit_index = 0;               // (epoch, index - 1) can follow the geometry through the one pose the scene keeps (Scene::pose_snap)
    std::vector<rt_frame*> frames;   // the frames alive on this context (rt_finish waits for their side streams too)
    uint8_t* blue_noise = nullptr;   // sobol[65536] | scramblingTile[131072] | rankingTile[131072]
    float* gamma_lut = nullptr;      // pow(byte / 255, 2.2f), 256 entries (k_fill_gamma_lut)
    query::Scratch query;            // rt_scene_trace*: the walk's stack spill area and the host form's staging arrays (query_host.h)
    query::Scratch bake;             // rt_scene_bake*: the same of its own (stages 0 and 1; the status word stays query.status), reported apart by rt_scene_tree_report
    uint32_t bake_chunk_points = bake::CHUNK_POINTS;   // RT_CTX_OPT_BAKE_CHUNK_POINTS
    std::string report_out;          // rt_scene_tree_report's answer when it has a "ray queries" line to add to the scene's report
};

struct rt_buffer
{
    rt_ctx* ctx;
    void* ptr;
    size_t bytes;
};

namespace context
{
// msg becomes the context's last error (no context: the calling thread's) and the call's result is RT_ERROR.  One definition, context.cpp's, beside
// rt_last_error and the thread's message.
int fail(rt_ctx* ctx, const std::string& msg);
// the calling thread's message (context.cpp); rt_group_last_error answers with it too (group_impl.h)
extern thread_local std::string g_thread_error;

#define HIPCHK(ctx, expr)                                                                         \
    do                                                                                            \
    {                                                                                             \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return context::fail(ctx, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

// m = `bytes` of device memory with src's bytes on their way into it on ctx's stream (no src: nothing is copied); a failure is `who`'s error
int dev_fill(rt_ctx* ctx, const char* who, dev::Mem& m, const void* src, size_t bytes);

// the same for a raw field of the Scene (free_scene's to free): it is set only when the allocation and the copy both worked
int scene_array(rt_ctx* ctx, void** field, const void* src, size_t bytes);

// Ray queries: the walk's status word (pinned host memory; bit 0: a traversal stack ran over its bound, query_kernels.h), read and cleared wherever the
// context's stream has just been waited for -- rt_scene_trace, rt_finish, rt_buffer_read -- so that the buffer form's queries report it too.
int query_check_status(rt_ctx* ctx, const char* who);

// Nothing in flight may still read what is about to be freed or rewritten: batches traced ahead are dropped (RT_OPT_SAMPLES_AHEAD), and every stream a frame
// launches on -- side streams, pipes, banks -- has drained.  context.cpp's, on what frame.h declares for it.
int quiesce(rt_ctx* ctx);

// Everything a scene holds on the device and beside it (its adaptation, refit, pose, skin and morph states) is freed and `s` is an empty scene again.  scene_upload.cpp's:
// rt_scene_upload and an upload that ends early call it there, rt_ctx_destroy from context.cpp.
void free_scene(Scene& s);

// The refit (scene_upload.cpp's, with rt_scene_refit*), for scene_moved.cpp's pose, skin and morph too.  refit_refused: why `who` cannot refit this scene now,
// as the context's error, or RT_OK.  Then refit_device: d_tris (device memory, written on ctx's stream) are validated read-only and become the scene's triangles.
int refit_refused(rt_ctx* ctx, const char* who, uint64_t count_or_bytes, bool bytes);
int refit_device(rt_ctx* ctx, const rt_triangle* d_tris, const char* who);

// The re-layout kernels' four launches on ctx's stream (relayout_kernels.h; they are of the hot path's code object, so rt_hip.hip launches them for
// Upload::relayout_on_device): the reference's node and triangle arrays on the device -> the child-pair records `nodes` in the order `index` gives, the 64-byte
// and 128-byte triangle records; `last` (nt bytes) and `err` (one int, an RL_* code of device_scene.h: the first one wins) are the caller's, cleared on the
// stream before this.  RT_OK: all four were launched.
int relayout_records(rt_ctx* ctx, const rt_bvh_node* raw_nodes, uint32_t nn, const rt_triangle* raw_tris, uint32_t nt, uint32_t num_materials, const uint32_t* index,
    uint8_t* last, int* err, float4* nodes, float4* tris_rt, float4* tris_sh);
} // namespace context
