// device_scene.h -- DScene, the kernels' view of an uploaded scene: the record every launch receives by value.  Apart from kernels_common.h (which
// includes it) so that host translation units that hold one (context.h: Scene::d) need no device code and compile as plain C++.  With it, for the same
// reason, the two other things of the kernels' that the scene's host unit reads -- DCounters and the re-layout kernels' error codes -- and the plain records
// a frame holds (DTile, DLog, DAov) with the sizes its buffers are made by, for frame.h.
#pragma once
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include "rt_types.h"

struct DScene
{
    const float4* nodes;          // 4 x float4 per interior node
    const float4* tris_rt;        // 4 x float4 per triangle
    const float4* tris_sh;        // 8 x float4 per triangle
    const rt_packed_material* materials;
    const rt_texture* textures;
    const uint32_t* texture_data;
    const float4* lights;         // 3 x float4 per light: origin, radiance, (type bits,0,0,0)
    const float4* env;
    const float* gamma_lut;       // pow(byte / 255, 2.2f) for the 256 texel values (k_fill_gamma_lut)
    int env_w, env_h;
    uint32_t light_count;
    uint32_t root_ref;            // RT_LEAF_BIT | first triangle, or interior node 0
    uint32_t entry_ref;           // "super-root" record: child 0 = (root box, root_ref), child 1 empty
    const float4* wnodes;         // 4-wide quantized nodes (k_trace_w4), 4 x float4 each; nullptr = not built
    uint32_t w_entry_ref;         // wide node 0, or RT_LEAF_BIT | first triangle when the root is a leaf
    const float4* wnodes_sh;      // the tree the SHADOW rays walk: the backend's own over the reference's leaves (own_bvh.h), or wnodes
    uint32_t w_sh_entry_ref;
    float root_min[3];
    float root_max[3];
    // opt-in extensions (rt_scene_desc): nullptr / 0 = the reference's behaviour
    const uint16_t* mat_tex16;    // 6 texture indices per material (0xFFFF = none) replacing the packed 8-bit ones
    const uint32_t* emissive;     // emissive triangle indices (Scene::GetEmissiveIndices)
    uint32_t emissive_count;
    uint32_t emissive_nee;        // RT_SCENE_EMISSIVE_NEE
};

// The frame's counters, here for the same reason: the fold adaptation's probe copies one per sample to the host (FoldAdapt::probe_counters, fold_adapt.h) and its
// worker reads the queue lengths out of it (scene_upload.cpp).
#define RT_LOG_SUBPOOLS 64u        // the overflow pool of the compact log is handed out from this many bump counters (k_shade)
struct DCounters                  // one per frame, device memory
{
    uint32_t queue[64];           // queue[b]  = rays in the incoming queue of bounce b
    uint32_t shadow[64];          // shadow[b] = shadow rays emitted at bounce b
    unsigned long long total_closest, total_shadow, samples;
    uint32_t last_queue[64], last_shadow[64];
    // work-distribution heads of the persistent trace kernels: one per XCD and per
    // kernel flavour (0 = closest, 1 / 2 = shadow rays of an even / odd bounce: the shadow trace of bounce b may
    // still be running while k_shade of bounce b + 1 prepares the next one), offsets inside the XCD's region
    uint32_t head[3][8];
    // rays k_trace_w4 hands to the BVH2 kernel (non-finite 1/dir): list length and that launch's work heads
    uint32_t slow_count[4];       // per flavour ([3] unused)
    uint32_t slow_head[3][8];
    uint32_t stack_spills;        // lane-steps with stack entries in the HBM spill area (k_trace2 / k_trace_w4), since the last reset
    uint32_t slow_rays;           // rays k_trace_w4 handed to k_trace2, since the last reset
    // launch timeline of k_trace_w4<closest> per bounce (rt_frame_debug_timeline), 100 MHz wall clock:
    // first wave started, first wave found the queue dry, last wave left
    unsigned long long tl_start[64], tl_dry[64], tl_end[64];
    // ... of its slowest ray: most traversal steps (wide nodes + triangles) any ray took, and the ticks from hand-out to
    // retirement (high bits) and steps (low 24 bits) of the ray that took longest ...
    unsigned long long tl_ray_steps[64], tl_ray_ticks[64];
    // ... and when its waves left, in 25 us bins after the first wave found the queue dry (all recorded launches together)
    unsigned long long tl_exit_hist[64];
    // compact radiance log (DLog): next free overflow block of the batch in flight, and "the pool ran dry"
    uint32_t log_ovf_next[RT_LOG_SUBPOOLS], log_ovf_flag;
};

// The plain records a frame holds or hands to its launches, and the four sizes its buffers are made by: here so that frame.h -- what a frame is, for the host
// units that implement entry points on one (frame_filters.cpp, frame_readers.cpp) -- needs no device code either.  What the kernels do with them stays with
// the kernels: log_index and log_put, tile_global_row (kernels_common.h).
#define RT_TRACE_STACK_LDS 24     // per-lane stack entries kept in LDS
#define RT_TRACE_STACK_MAX 64     // the reference's nodesToVisit[64] (trace_bvh.cl:142)
#define RT_W4_STACK_MAX 104               // <= 3 pending slots per wide level, <= 33 wide levels + slack
#define RT_FRAME_COUNT_STRIDE 136u       // per-wave row: [0..63] closest rays per bounce, [64..127] shadow rays per bounce, [128] spills, [129] slow rays, [130] scratch,
                                         // [131..134] the wave's 100 MHz ticks in the closest walks / shading / shadow walks / in all (rt_frame_debug_frame_rows)

// Where the entries of a path's radiance log live (the two layouts: kernels_common.h, above log_index)
struct DLog
{
    float* rlog;                  // 3 floats per entry
    uint32_t* cnt;                // entries of path id (k_flush replays that many)
    uint32_t* ovf_slot;           // compact: the overflow block of path id (RT_EMPTY_REF: none); nullptr in the full layout
    uint32_t stride;              // paths per row
    uint32_t inline_entries;
    uint32_t ovf_blocks;
};

struct DTile                      // which pixels of the full image this frame owns
{
    uint32_t width, height;       // full image
    uint32_t band_h, rank, nranks;
    uint32_t local_rows;
};

// the four AOV images (aov_kernels.h)
struct DAov
{
    float4* diffuse_albedo;   // float3 in the reference (16 B)
    float* depth;
    float4* normal;
    float2* velocity;
};

// What the re-layout kernels (relayout_kernels.h) report of the caller's arrays, the first one wins; decoded by the host (Upload::relayout_on_device, scene_upload.cpp).
enum { RL_OK = 0, RL_CHILD_RANGE = 1, RL_LEAF_RANGE = 2, RL_AXIS = 3, RL_MATERIAL = 4 };
