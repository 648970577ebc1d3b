// fold_adapt.h -- the state of RT_CTX_OPT_ADAPTIVE_FOLD (FoldAdapt; Scene::adapt points at one) for the two units that work on it: scene_upload.cpp arms it at
// upload, owns its worker (crossing counts, re-fold, tree rotations, occluder-first slots, the upload of the adapted records) and drops it; the
// render thread's side (frame_fold_hooks.cpp) probes, hands over to the worker and adopts.  Internal, like context.h -- which keeps the name only, so the
// queries' unit sees no more than that.
#pragma once
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "context.h"
#include "wide_node.h"       // WideNode

// ---- Fold adaptation (RT_CTX_OPT_ADAPTIVE_FOLD) ---------------------------------------------------------------------------------
// build_wide_bvh's dynamic programme is optimal for whatever visit probability it is given, and the surface area is only the
// probability of a ray population nobody traces: uniformly distributed lines.  The rays of a frame are not that (they start at
// the camera or on surfaces and stop at the first hit), and what they do can be measured: the first rt_integrate of a scene
// traces a small probe frame, the host counts how often its rays pass each box of the binary tree (closest-hit rays clipped at
// their hit), and the trees are folded again for those frequencies -- tools/fold_weight_study.py: - 8 % closest-hit and - 10 %
// shadow record visits on the benchmark scene, out of sample, and 14 000 probe rays are as good as 220 000.
// Exact by construction: every fold of the same binary tree tests the same leaves in the same order (build_wide_bvh).
namespace context
{
struct FoldAdapt
{
    enum { ARMED = 1, COMPUTING = 2, IDLE = 3, OFF = 4, PROBING = 5 };   // IDLE: adapted to `camera`; a frame whose camera has moved away arms it again;
                                                                         // PROBING: the probe frame's launches and copies are on the stream
    int state = ARMED;
    std::atomic<uint32_t> mode{1};                     // ctx->adaptive_fold at upload (atomic: RT_CTX_OPT_ADAPT_WAIT changes bit 1 on the render thread while the worker reads bits 3 / 4)
    uint32_t adaptations = 0;                          // folds adopted so far
    rt_camera camera;                                  // the probe's camera
    double scene_diagonal = 0.0;
    std::vector<rt_bvh_node> bvh2, bvh2_sh;            // the reference's tree; the shadow rays' own binary tree (empty: they walk the reference's)
    std::vector<uint32_t> roots, roots_sh;             // the binary-tree node each record of the CURRENT folds tests
    std::vector<uint32_t> roots_new, roots_sh_new;     // ... of the adapted folds
    std::vector<float> tri9;                           // mode bit 4: the triangles' corner positions (9 floats each), for the host's occluder search
    uint32_t reordered = 0;                            // ... shadow records whose slots changed places (0: placed as build_wide_bvh places them)
    std::vector<rt_bvh_node> bvh2_sh_new;              // mode bit 3: the shadow rays' binary tree after tree_rotate.h's rotations (when that is what was folded)
    uint32_t rotations = 0;                            // ... how many (0: the fold is of the tree as it was)
    std::vector<float4> o, d, sh_o, sh_d;              // the probe's rays (o.w = t_max: the hit distance where there was one)
    std::vector<WideNode> wide, wide_sh;               // the adapted folds
    uint32_t entry = 0, entry_sh = 0;
    bool ok = false, ok_sh = false;                    // ... exist and are cheaper for the probe rays
    double cost[2][2] = {{0.0, 0.0}, {0.0, 0.0}};      // [closest, shadow][current, adapted]: record visits per probe ray (an upper bound: box passes)
    double seconds = 0.0;
    double rotate_s[4] = {0, 0, 0, 0};                     // ... and tree_rotate.h's phases
    double stage_s[7] = {0, 0, 0, 0, 0, 0, 0};             // the worker's stages: unpacking the probe, closest-hit re-fold, shadow: plain re-fold, rotations, rotated re-fold, occluder order; upload
    std::atomic<bool> finished{false}, cancel{false};
    std::thread worker;
    // The probe (round 5: nothing on the render thread waits for it): a frame of its own, kept for the scene's life; its queues come back through
    // pinned memory with asynchronous copies behind each stage, `probe_done` marks the last one; the worker unpacks them (probe_unpack).
    rt_frame* probe = nullptr;
    uint32_t probe_paths = 0, probe_samples = 0, probe_bounces = 0;      // capacity of a queue, samples traced, bounces + 1
    char* staging = nullptr; size_t staging_bytes = 0;                   // pinned; layout: probe_block / probe_counters below
    hipEvent_t probe_done = nullptr;
    // The device side of an adoption is the WORKER's too: it uploads the adapted records on a stream of its own, and frees the ones an
    // earlier adoption replaced after a device synchronisation of ITS thread (every launch that could still read them was enqueued before
    // that adoption).  The render thread only exchanges pointers: no hipDeviceSynchronize, no hipMalloc / hipFree between two frames.
    int device = -1;                                                     // -1: host only (rt_debug_fold_abandon)
    bool device_fold = false;                                            // RT_CTX_OPT_DEVICE_FOLD: crossing counts and re-folds on `device` ...
    // ... when the device has nothing better to do: with bit 1 (rt_integrate waits for the adaptation) it is idle and the folds on it shorten the wait
    // (1.33 -> 1.09 s to the adapted fold on the headline scene, 8.5 -> 7.1 s on the 10 M-triangle one: profiles/r06/call03.log); asynchronously -- the library's
    // default -- the frames keep it busy and the host's threads are what is free: the same folds on the device took an orbiting camera's frames from
    // + 2 .. 4 % to + 23 % (per_frame.moving_camera, profiles/r06/call04.log), so there the worker folds on host threads as it did before.
    // Measured again in round 6's call 24, with the worker's other stages short: the folds on the device beside an orbiting camera's frames take 0.36 - 0.60 s instead of the
    // host's 0.22 - 0.25 (their kernels queue behind the frames') and the frames 3.6 - 3.8 ms instead of 2.68 (+ 40 %): the policy stands.
    int worker_fold_device() const { return device_fold && (mode.load() & 2u) ? device : -1; }
    bool pairs = false;                                                  // RT_CTX_OPT_WIDE_LAYOUT
    void *new_cl = nullptr, *new_sh = nullptr;
    bool upload_failed = false;
    std::vector<void*> retired;
    std::chrono::steady_clock::time_point last_armed{};                  // re-arming is rate-limited (RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS)
    std::atomic<uint32_t> min_interval_ms{500};
    size_t probe_block(uint32_t sample, uint32_t bounce, uint32_t which /* 0 o, 1 d, 2 hits, 3 shadow o, 4 shadow d */) const
    {
        return ((((size_t)sample * probe_bounces + bounce) * 5u + which) * probe_paths) * sizeof(float4);
    }
    size_t probe_counters(uint32_t sample) const { return (size_t)probe_samples * probe_bounces * 5u * probe_paths * sizeof(float4) + (size_t)sample * sizeof(DCounters); }
    ~FoldAdapt();
};

// What the context's and the frames' units call on one; all of it is scene_upload.cpp's.
void drop_fold_adapt(FoldAdapt* a);        // waits for its worker thread
void fold_adapt_set_interval(FoldAdapt* a, uint32_t ms);
void fold_adapt_set_wait(FoldAdapt* a, bool wait);
void fold_adapt_worker(FoldAdapt* a);      // the worker thread's body: fold_adapt_hook starts it once the probe's queues are on the host
// Has camera `c` left the view the folds were adapted to?  (fold_adapt_hook's trigger, rt_debug_fold_view_left)
bool fold_view_left(const FoldAdapt& a, const rt_camera& c);
// The tree report keeps one entry of a kind, the latest: what begins at the first `prefix` goes, `line` is appended.  (The upload's side writes the refit's
// and the imported folds' entries with it, the render thread's side the adaptation's.)
void replace_report_line(std::string& report, const char* prefix, const std::string& line);
} // namespace context
