// rt_hip.hip -- every launch of the hot path's code object (kernels.h: k_trace_w4, k_trace2, k_shade, k_frame, k_flush, k_raygen and the small kernels beside
// them), each with the grid, the stream and the arguments it takes.  What the units that schedule a frame's samples call here is frame_launch.h's namespace
// launch; what a context needs, context::relayout_records and context::fill_gamma_lut; what a filter needs, frame::trace_guides.  The entries whose body is
// essentially one launch stay as entries: rt_compute_aovs, rt_denoise, rt_copy_history, rt_frame_resolve, rt_frame_present(_wait), rt_frame_get_stats,
// rt_debug_eval, and the device groups (group_impl.h).  Everything else of the C-ABI in include/rt_hip.h is host code in units of its own: the context and
// the buffers (context.cpp), what a frame is made of and how it is laid out (frame_layout.cpp), when its samples run (frame_schedule.cpp), the fold
// adaptation's render-thread side (frame_fold_hooks.cpp), the scene (scene_upload.cpp, scene_moved.cpp, scene_queries.cpp), the filters and the readers
// (frame_filters.cpp, frame_readers.cpp).  The launches keep the order they have in this file: it decides where clang places the kernels' template
// instantiations in the code object, and codeobj.code_object_sha256 identifies that code object.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <assert.h>
#include <math.h>
#include <cmath>
#include <algorithm>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "kernels.h"
#include "device_memory.h"   // who owns a device allocation: dev::Mem
#include "context.h"         // Scene, rt_ctx, fail / HIPCHK
#include "frame.h"           // rt_frame, its pipes, banks and buffer lists; what the frames' feature units call on a frame: namespace frame
#include "frame_launch.h"    // what this unit offers the scheduling units (namespace launch), and what it calls on the layout (wait_shadow, side_on, ensure_slots, bytes_per_path)
using namespace rtw;
using namespace context;
using namespace frame;
using namespace launch;

// ---- context ---------------------------------------------------------------
// the gamma table of a new context, filled on its stream: the one launch rt_ctx_create (context.cpp) makes
void context::fill_gamma_lut(rt_ctx* ctx)
{
    hipLaunchKernelGGL(k_fill_gamma_lut, dim3(1), dim3(256), 0, ctx->stream, ctx->gamma_lut);
}

// ---- scene -----------------------------------------------------------------
// The scene's upload, trees, adaptation worker, refit and pose are scene_upload.cpp's.  What stays here of an upload are the launches of the re-layout
// kernels, which belong to this unit's code object: Upload::relayout_on_device clears `last` and `err` on the stream, calls this, and reads `err` back.
int context::relayout_records(rt_ctx* ctx, const rt_bvh_node* raw_nodes, uint32_t nn, const rt_triangle* raw_tris, uint32_t nt, uint32_t num_materials, const uint32_t* index,
    uint8_t* last, int* err, float4* nodes, float4* tris_rt, float4* tris_sh)
{
    hipLaunchKernelGGL(k_relayout_mark_leaves, dim3((nn + 255u) / 256u), dim3(256), 0, ctx->stream,
        raw_nodes, nn, nt, last, err);
    hipLaunchKernelGGL(k_relayout_nodes, dim3((nn + 255u) / 256u), dim3(256), 0, ctx->stream,
        raw_nodes, nn, index, nodes, err);
    hipLaunchKernelGGL(k_relayout_triangles, dim3((nt + 255u) / 256u), dim3(256), 0, ctx->stream,
        raw_tris, nt, num_materials, (const uint8_t*)last, tris_rt,
        tris_sh, err);
    hipLaunchKernelGGL(k_relayout_leaf_bounds, dim3((nn + 255u) / 256u), dim3(256), 0, ctx->stream,
        raw_nodes, nn, nt, tris_rt);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERROR;
}

// ---- frame -----------------------------------------------------------------
// the radiance log of a pipe as the kernels see it
DLog launch::dlog(const rt_frame* f, const PathPipe& p)
{
    DLog L;
    L.rlog = p.rlog; L.cnt = p.cnt; L.ovf_slot = f->log_ovf_blocks ? p.ovf_slot : nullptr;
    L.stride = f->log_stride; L.inline_entries = f->log_inline; L.ovf_blocks = f->log_ovf_blocks;
    return L;
}

// Adds the logged contributions of the batch in flight on pipe `p` to the running sum.
int launch::flush_log(rt_frame* f, PathPipe& p, bool keep_open)
{
    rt_ctx* ctx = f->ctx;
    if (p.cur_slots == 0 || f->n_local == 0 || p.chunk_count == 0) { p.cur_slots = 0; return RT_OK; }
    if (p.shadow_pending)
        return fail(ctx, "radiance requested between rt_shade and rt_intersect_shadow (direct samples still tentative)");
    if (wait_shadow(f, p, 0) != RT_OK || wait_shadow(f, p, 1) != RT_OK) return RT_ERROR;   // their verdicts are in the log
    uint32_t blocks = (p.chunk_count + 255u) / 256u;
    hipLaunchKernelGGL(k_flush, dim3(blocks), dim3(256), 0, p.stream, f->radiance + p.chunk_base, dlog(f, p),
        p.chunk_count, p.cur_slots, f->chunk_pixels, keep_open && f->log_ovf_blocks != 0u ? 1u : 0u, 0u);
    if (hipGetLastError() != hipSuccess) return fail(ctx, "k_flush launch failed");
    p.cur_slots = 0;
    return RT_OK;
}

// Mid-sample read (stage API / debugging): apply what has been logged so far but
// keep the sample open -- later contributions append again from entry 0.
int launch::flush_log_keep(rt_frame* f, PathPipe& p)
{
    uint32_t keep = p.cur_slots;
    int rc = flush_log(f, p, true);
    p.cur_slots = keep;
    return rc;
}

// ---- stages ----------------------------------------------------------------
namespace
{
// RAII bracket: records a start event now and a stop event at scope exit
struct KernelSpan
{
    rt_frame* f; int cls; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    KernelSpan(rt_frame* f_, int cls_, hipStream_t stream) : f(f_), cls(cls_), st(stream)
    {
        if (!f->profile) return;
        auto get = [&]() { hipEvent_t e = nullptr; if (!f->event_pool.empty()) { e = f->event_pool.back(); f->event_pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
        a = get(); b = get();
        (void)hipEventRecord(a, st);
    }
    ~KernelSpan()
    {
        if (!a) return;
        (void)hipEventRecord(b, st);
        f->spans.push_back({a, b, cls});
    }
};
} // namespace

namespace
{
#define RT_TRACE2_DEFAULT_TUNE (32u | (8u << 8))     // profiles/r02_ktrace2_tune_sweep.log, r02_w4_tune_sweep.log
#define RT_W4_DEFAULT_RAYS_PER_LANE 0u               // k_trace_w4's live-counter grid (trace_kernels.h); 0 = every wave

// What a trace launch needs besides its rays: where it goes and what it writes.  The stage that launches builds one from its pipe (the guide pass: from
// the filter's own buffers) and hands it down by value.
struct TraceTarget
{
    hipStream_t stream;
    uint2* spill; uint32_t* slow_list;     // the launch's stack spill area; the queue indices k_trace_w4 leaves to k_trace2
    uint32_t flavour;                      // which work heads and slow-ray count of `counters`: 0 = closest hit, 1 + q = shadow queue q
    float4* hits;                          // nullptr: a shadow trace
    DLog log; DCounters* counters;
    uint64_t paths;                        // paths of the batch the rays belong to (a launch's size class; its live count is on the device)
    uint32_t timeline_slot;                // rt_frame_debug_timeline: the bounce whose slot the instrumented closest-hit instance records into
    uint32_t variant, waves_per_cu;        // RT_OPT_TRACE_VARIANT, RT_OPT_TRACE_WAVES_PER_CU as this launch takes them
    const PrimaryGen* primary = nullptr;   // RT_OPT_FUSED_RAYGEN: the launch makes its rays itself (bounce 0 of a batch for which primary_fusable held)
};

// the persistent grid of one-wave blocks for an LDS stack of `stack_entries` entries: 160 KiB / (entries * 512 B) waves per CU, at most 32 and at most
// waves_per_cu (0 = no cap), rounded up to a multiple of 8 blocks (one per XCD)
uint32_t persistent_blocks(const rt_ctx* ctx, uint32_t stack_entries, uint32_t waves_per_cu)
{
    uint32_t per_cu = (160u * 1024u) / (stack_entries * 512u);
    if (per_cu > 32u) per_cu = 32u;
    if (waves_per_cu && waves_per_cu < per_cu) per_cu = waves_per_cu;
    return ((uint32_t)ctx->prop.multiProcessorCount * per_cu + 7u) & ~7u;
}

// RT_OPT_TRACE_TUNE's node and leaf thresholds, field by field (0 = that field's default), as node | leaf << 8
uint32_t tune_thresholds(uint32_t t)
{
    const uint32_t node_q = (t & 0xFFu) ? (t & 0xFFu) : (RT_TRACE2_DEFAULT_TUNE & 0xFFu);
    const uint32_t leaf_q = ((t >> 8) & 0xFFu) ? ((t >> 8) & 0xFFu) : ((RT_TRACE2_DEFAULT_TUNE >> 8) & 0xFFu);
    return node_q | leaf_q << 8;
}

// k_trace2: separate wave-uniform loops (trace_kernels.h).  One-wave blocks on the persistent grid of the LDS-limited residency.
template <bool SHADOW, int STACK>
void launch_trace2(rt_frame* f, const TraceTarget& t, const float4* o4, const float4* d4, const uint32_t* aux, const uint32_t* count)
{
    rt_ctx* ctx = f->ctx;
    const uint32_t blocks = persistent_blocks(ctx, STACK, t.waves_per_cu);
    uint32_t tune = f->trace_tune ? f->trace_tune : RT_TRACE2_DEFAULT_TUNE;
    if ((tune & 0xFFu) > 64u) tune = (tune & ~0xFFu) | 64u;
    if ((tune & 0xFFu) == 0u) tune |= 1u;
    hipLaunchKernelGGL((k_trace2<SHADOW, STACK>), dim3(blocks), dim3(64), 0, t.stream, ctx->scene.d, o4, d4, aux, count,
        &t.counters->head[t.flavour][0], t.hits,
        t.log, f->select_form_box, t.spill, tune, (const uint32_t*)nullptr,
        &t.counters->stack_spills);
}

// RT_OPT_FUSED_RAYGEN: the bounce-0 closest-hit launch that makes its primary rays itself, in place of the plain or the loop-D instance of the 12-entry stack
void launch_trace_w4_primary(rt_frame* f, const TraceTarget& t, uint32_t blocks, uint32_t tune, uint32_t chunk_below, bool tail_instance, const uint32_t* count)
{
    DCounters* const c = t.counters;
    if (tail_instance)
        hipLaunchKernelGGL((k_trace_w4_primary<true>), dim3(blocks), dim3(64), 0, t.stream, f->ctx->scene.d, *t.primary, count, &c->head[0][0], t.hits,
            t.spill, tune, t.slow_list, &c->slow_count[0], &c->stack_spills, chunk_below, f->trace_tail_lanes, f->chunk_refill);
    else
        hipLaunchKernelGGL((k_trace_w4_primary<false>), dim3(blocks), dim3(64), 0, t.stream, f->ctx->scene.d, *t.primary, count, &c->head[0][0], t.hits,
            t.spill, tune, t.slow_list, &c->slow_count[0], &c->stack_spills, chunk_below, 0u, f->chunk_refill);
}

// k_trace_w4 over the 4-wide quantized tree, then k_trace2 over the (normally empty) list of rays it left out
template <bool SHADOW, int STACK>
void launch_trace_w4(rt_frame* f, const TraceTarget& t, const float4* o4, const float4* d4, const uint32_t* aux, const uint32_t* count)
{
    rt_ctx* ctx = f->ctx;
    const uint32_t blocks = persistent_blocks(ctx, STACK, t.waves_per_cu);
    // RT_OPT_TRACE_TUNE, field by field (0 = that field's default)
    const uint32_t thresholds = tune_thresholds(f->trace_tune);
    const uint32_t node_q = (thresholds & 0xFFu) > 64u ? 64u : (thresholds & 0xFFu);
    uint32_t rays_per_lane = (f->trace_tune >> 24) ? (f->trace_tune >> 24) : RT_W4_DEFAULT_RAYS_PER_LANE;
    if (rays_per_lane == 255u) rays_per_lane = 0u;                          // 255 = every wave of the residency-sized grid
    const uint32_t tune = node_q | (thresholds & 0xFF00u) | (f->trace_tune & 0xFF0000u) | rays_per_lane << 24;
    const uint32_t s = t.flavour;
    DCounters* const c = t.counters;
    // the instance with loop D and refilled chunks (below): static assignment stays ahead of the shared work heads up to larger launches
    // there -- 8 M rays instead of 3 M (4 / 8 / 16 samples of a 1080p frame in flight: +2.7 / +8.4 / +4.8 %, profiles/r04_call20.log)
    const bool tail_instance = STACK == 12 && f->trace_tail_lanes != 0u && t.paths < f->trace_tail_paths && !(!SHADOW && f->timeline);
    const uint64_t small = f->small_launch_set || !tail_instance ? f->small_launch_paths : 8000000ull;
    const uint32_t chunk_below = small > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)small;
    // (Camera-ray launches refilled instead of chunked -- coherent rays, short tails? -- measured: 2477 instead of 2876 Mrays/s per frame,
    // profiles/r04_call14.log: a refilling launch of any size pays its ~0.6 ms drain.)
    unsigned long long* const no_timeline = nullptr;
    if (!SHADOW && STACK == 12 && t.primary)            // RT_OPT_FUSED_RAYGEN (primary_fusable: no timeline, this variant)
        launch_trace_w4_primary(f, t, blocks, tune, chunk_below, tail_instance, count);
    else if (!SHADOW && STACK == 12 && f->timeline)          // tools/launch_timeline.py: the instrumented instance
        hipLaunchKernelGGL((k_trace_w4<false, 12, true, false>), dim3(blocks), dim3(64), 0, t.stream, ctx->scene.d, o4, d4, aux, count,
            &c->head[s][0], t.hits, t.log, t.spill, tune, t.slow_list,
            &c->slow_count[s], &c->stack_spills, &c->tl_start[t.timeline_slot & 63u],
            t.timeline_slot & 63u, chunk_below, 0u, f->chunk_refill);
    else if (tail_instance)       // loop D (the fused tail pass) where the whole batch is a small launch: chunk mode whatever the live counter says (count <= paths < chunk_below)
        hipLaunchKernelGGL((k_trace_w4<SHADOW, 12, false, true>), dim3(blocks), dim3(64), 0, t.stream, ctx->scene.d, o4, d4, aux, count,
            &c->head[s][0], t.hits, t.log,
            t.spill, tune, t.slow_list, &c->slow_count[s], &c->stack_spills, no_timeline, 0u, chunk_below, f->trace_tail_lanes, f->chunk_refill);
    else
        hipLaunchKernelGGL((k_trace_w4<SHADOW, STACK, false, false>), dim3(blocks), dim3(64), 0, t.stream, ctx->scene.d, o4, d4, aux, count,
            &c->head[s][0], t.hits, t.log,
            t.spill, tune, t.slow_list, &c->slow_count[s], &c->stack_spills, no_timeline, 0u, chunk_below, 0u, f->chunk_refill);
    // The follow-up over the (normally empty) slow list: waves with a two-entry LDS stack (the rest of the stack
    // lives in the spill area) -- 1 KiB of LDS and a few registers, so it finds room beside the resident waves of the
    // OTHER stream's persistent launch (RT_OPT_OVERLAP_SHADOW) instead of waiting for that launch to end: with the
    // 6 KiB blocks of the ordinary k_trace2 the closest-hit follow-up sat 2.8 ms on average behind the shadow trace
    // (profiles/r02_final_rocprofv3_kernel_stats_overlap.csv) with k_shade queued behind it.
    // Four such waves per CU (4 KiB of LDS beside the other launch's 26 x 6 KiB): with an empty list they leave at once;
    // with a long one (every shadow ray towards an axis-aligned point-light arrangement, say) the list is not serialised
    // onto one wave per CU.  Scenes whose directional lights make MOST shadow rays slow never get here (Scene::slow_shadow).
    uint32_t blocks2 = ((uint32_t)ctx->prop.multiProcessorCount * 4u + 7u) & ~7u;
    hipLaunchKernelGGL((k_trace2<SHADOW, 2>), dim3(blocks2), dim3(64), 0, t.stream, ctx->scene.d, o4, d4, aux,
        (const uint32_t*)&c->slow_count[s], &c->slow_head[s][0], t.hits,
        t.log, f->select_form_box, t.spill, tune & 0xFFFFu, (const uint32_t*)t.slow_list,
        &c->stack_spills);
}

template <bool SHADOW>
void launch_trace(rt_frame* f, const TraceTarget& t, const float4* o4, const float4* d4, const uint32_t* aux, const uint32_t* count)
{
    rt_ctx* ctx = f->ctx;
    uint32_t variant = t.variant;
    if (variant == 5)
    {
        // auto: the 4-wide quantized tree wherever it was built -- 4214 (round 1's k_trace) / 4400 (k_trace2) / 5042
        // (k_trace_w4) Mrays/s on the headline workload when it was introduced (profiles/r02_w4_tune_sweep.log).
        // Scenes whose directional lights make most shadow rays "slow" (Scene::slow_shadow) trace the shadow queue with
        // k_trace2, which handles such rays inline.
        variant = (SHADOW && ctx->scene.slow_shadow) ? 8u : 10u;
        // k_trace_w4 switches to its chunk mode by itself when a launch is small (RT_OPT_SMALL_LAUNCH_PATHS, decided in the
        // kernel from the live queue counter).  Without the wide tree, small batches take the per-ray loop of v1, which
        // beats the refilling BVH2 kernel there (1511 vs 737 Mrays/s at one 1080p sample in flight, profiles/r03_call02_*)
        if ((variant == 8u || !ctx->scene.wide_ok) && t.paths < 2000000ull) variant = 0u;
    }
    if ((variant == 10u || variant == 11u) && !ctx->scene.wide_ok) variant = 8u;
    if ((variant == 8u || variant == 9u) && !ctx->scene.offsets32) variant = 0u;
    switch (variant)
    {
    case 0:
        hipLaunchKernelGGL(k_trace_v1<SHADOW>, dim3(t.waves_per_cu ? (((uint32_t)ctx->prop.multiProcessorCount *
            (t.waves_per_cu < 13u ? t.waves_per_cu : 13u) + 7u) & ~7u) : f->trace_blocks), dim3(64), 0, t.stream, ctx->scene.d, o4, d4,
            aux, count, t.hits, t.log, f->select_form_box, t.spill);
        break;
    case 8:
        if (!SHADOW && ctx->scene.d.entry_ref < 4000000u) launch_trace2<SHADOW, 10>(f, t, o4, d4, aux, count);
        else launch_trace2<SHADOW, 12>(f, t, o4, d4, aux, count);
        break;
    case 9: launch_trace2<SHADOW, 12>(f, t, o4, d4, aux, count); break;
    case 11: launch_trace_w4<SHADOW, 16>(f, t, o4, d4, aux, count); break;
    default: launch_trace_w4<SHADOW, 12>(f, t, o4, d4, aux, count); break;
    }
}
} // namespace

// Primary rays for `n_slots` consecutive samples (sample indices sample_count ..
// sample_count + n_slots - 1) in one launch on pipe `p`; they then travel through that pipe's queues.
// RT_OPT_FUSED_RAYGEN: may a batch of rt_integrate leave its bounce-0 queue unwritten?  Its bounce-0 closest-hit launch must be one of the k_trace_w4
// instances that have a primary form (the 12-entry stack, plain or loop D: what launch_trace picks under these conditions), and nothing else may read that
// queue: the instrumented instance (rt_frame_debug_timeline) does, and so does k_aov (per_frame: the caller rules it out).  The rays k_trace_w4 hands to
// k_trace2's list are written out by the primary instance itself.
bool launch::primary_fusable(const rt_frame* f)
{
    return f->fused_raygen != 0u && !f->timeline && f->ctx->scene.wide_ok && (f->trace_variant == 5u || f->trace_variant == 10u);
}

// fused: only the prologue runs (one block); the pipe's bounce-0 launches make the rays (intersect_pipe, shade_pipe)
int launch::generate_rays(rt_frame* f, PathPipe& p, uint32_t n_slots, uint32_t chunk_base, bool later_chunk_on_this_pipe, bool fused)
{
    rt_ctx* ctx = f->ctx;
    if (p.cur_slots != 0) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
    if (chunk_base == 0 && ensure_slots(f, n_slots) != RT_OK) return RT_ERROR;
    if (n_slots > f->slots) return fail(ctx, "rt_generate_rays: more samples than the frame can keep in flight");
    if (chunk_base >= tile_pixels(f)) return fail(ctx, "rt_generate_rays: chunk outside the tile");
    p.chunk_base = chunk_base;
    p.chunk_count = f->n_local - chunk_base < f->chunk_pixels ? f->n_local - chunk_base : f->chunk_pixels;
    float tan_half_fov = rt_tanf(0.5f * f->camera.fov);  // raygeneration.cl:108, uniform -> host
    uint32_t blocks = (p.chunk_count * n_slots + 255u) / 256u;
    if (blocks == 0 || fused) blocks = 1;
    p.primary_fused = fused;
    if (fused) ++f->fused_launches;
    KernelSpan span(f, 0, p.stream);
    hipLaunchKernelGGL(k_raygen, dim3(blocks), dim3(256), 0, p.stream, f->tile, f->camera, f->sample_count, n_slots,
        tan_half_fov, p.prev_bounces, p.o4[0], p.d4[0], p.thr[0], p.counters, p.chunk_base, p.chunk_count,
        f->chunk_pixels, p.fold_accumulates, fused ? 1u : 0u);
    p.fold_accumulates = later_chunk_on_this_pipe ? 1u : 0u;     // what the NEXT fold does with this sequence's counters
    p.prev_bounces = f->max_bounces;
    p.cur_slots = n_slots;
    HIPCHK(ctx, hipGetLastError());
    return RT_OK;
}

namespace
{
// the blue-noise sampler's three tables as k_shade and k_frame read them (one allocation; nullptr: not uploaded)
void set_blue_noise(ShadeArgs& a, const rt_ctx* ctx)
{
    a.bn_sobol = ctx->blue_noise; a.bn_scramble = ctx->blue_noise ? ctx->blue_noise + 65536 : nullptr;
    a.bn_rank = ctx->blue_noise ? ctx->blue_noise + 65536 + 131072 : nullptr;
}

template <bool FURNACE, bool BLUE>
int launch_frame_kernel_t(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    PathPipe& q = f->ps[0];
    if (f->kf.blocks == 0u)
    {
        // RT_OPT_FRAME_KERNEL = 1: as many one-wave blocks as the device keeps resident (the kernel's registers decide), every wave with the same
        // number of chunks; = k >= 2: k chunks per wave, i.e. MORE blocks than are resident -- the hardware starts the next block where one has
        // finished, which is a dynamic schedule of the frame's chunks in units of k
        int per_cu = 0;
        HIPCHK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_frame<FURNACE, BLUE>, 64, 0));
        if (per_cu < 1) return fail(ctx, "rt_advance_sample: k_frame does not fit the device");
        const uint32_t n_chunks = (f->n_local + 63u) >> 6;
        const uint32_t resident = std::max(8u, (uint32_t)ctx->prop.multiProcessorCount * (uint32_t)per_cu);
        const uint32_t cpw = f->frame_kernel >= 2u && f->frame_kernel != 255u ? f->frame_kernel : (n_chunks + resident - 1u) / resident;     // chunks per wave
        //  all three or none: the grid's size is committed only with its buffers, so a failed allocation cannot leave a later
        // launch with kf.blocks != 0 and a NULL buffer
        const uint32_t n_blocks = (((n_chunks + cpw - 1u) / cpw) + 7u) & ~7u;
        rt_frame::KFrame k;
        bool ok = f->debug_alloc_limit != 0xFFFFFFFFu;                               // (RT_OPT_DEBUG_ALLOC_LIMIT = 0xFFFFFFFF: the test hook for this path)
        for (const DevBuf& b : k.buffers(n_blocks, cpw)) ok = ok && hipMalloc(b.p, b.bytes) == hipSuccess;
        if (!ok)
        {
            (void)hipGetLastError();
            k.release();
            return fail(ctx, "rt_advance_sample: out of device memory for k_frame's per-wave buffers");
        }
        k.blocks = n_blocks;
        f->kf = k;
        f->frame_chunks_per_wave = cpw;
    }
    // the previous sample's per-bounce counters go to the totals first (k_raygen does this for the stage kernels)
    hipLaunchKernelGGL(k_fold_counters, dim3(1), dim3(64), 0, q.stream, q.counters, q.prev_bounces, q.fold_accumulates);
    q.fold_accumulates = 0;
    q.prev_bounces = f->max_bounces;
    FrameArgs fa;
    memset(&fa, 0, sizeof(fa));
    ShadeArgs& a = fa.shade;
    a.log = dlog(f, q); a.counters = q.counters;
    set_blue_noise(a, ctx);
    a.sample_base = f->sample_count;
    a.n_local = f->chunk_pixels ? f->chunk_pixels : 1;
    a.pix_base = 0;
    a.count_in_ray = 1u;
    a.partition = 0;
    for (int i = 0; i < 2; ++i) { fa.o4[i] = q.o4[i]; fa.d4[i] = q.d4[i]; fa.thr[i] = q.thr[i]; }
    fa.hits = q.hits;
    fa.sh_o4 = q.sh_o4[0]; fa.sh_d4 = q.sh_d4[0]; fa.sh_aux = q.sh_aux[0];
    fa.radiance = f->radiance;
    fa.spill = f->kf.spill;
    fa.slow_list = f->kf.slow;
    fa.wave_counts = f->kf.counts;
    fa.cam = f->camera;
    fa.tan_half_fov = rt_tanf(0.5f * f->camera.fov);
    fa.max_bounces = f->max_bounces;
    fa.drop_last = f->drop_last;
    fa.tune = tune_thresholds(f->trace_tune);
    fa.tail_q = f->trace_tail_lanes;
    fa.chunks_per_wave = f->frame_chunks_per_wave;
    hipLaunchKernelGGL((k_frame<FURNACE, BLUE>), dim3(f->kf.blocks), dim3(64), 0, q.stream, ctx->scene.d, f->tile, fa);
    hipLaunchKernelGGL(k_frame_sum, dim3(130), dim3(256), 0, q.stream, (const uint32_t*)f->kf.counts, f->kf.blocks, f->max_bounces, q.counters);
    HIPCHK(ctx, hipGetLastError());
    q.chunk_base = 0;
    q.chunk_count = f->n_local;
    ++f->frame_launches;
    return RT_OK;
}
} // namespace

int launch::launch_frame_kernel(rt_frame* f)
{
    const bool blue = f->sampler == 1;
    if (f->white_furnace) return blue ? launch_frame_kernel_t<true, true>(f) : launch_frame_kernel_t<true, false>(f);
    return blue ? launch_frame_kernel_t<false, true>(f) : launch_frame_kernel_t<false, false>(f);
}

// ---- the three stages, one pipe's work each: the C entry points run them over the pipes that hold the stage API's sample, rt_integrate and the banks
// (trace_bounces) over the pipe of each chunk ------------------------------------------------------------------------------------------
// IntersectRays: the closest-hit trace of pipe p's ray queue of `bounce`
int launch::intersect_pipe(rt_frame* f, PathPipe& p, uint32_t bounce)
{
    rt_ctx* ctx = f->ctx;
    const uint32_t in = bounce & 1u;
    PrimaryGen g;
    const bool primary = bounce == 0u && p.primary_fused;
    if (primary) g = PrimaryGen{f->tile, f->camera, rt_tanf(0.5f * f->camera.fov), f->sample_count, p.cur_slots, p.chunk_base, f->chunk_pixels, p.o4[0], p.d4[0]};
    const TraceTarget t = {p.stream, p.spill, p.slow_list, 0u, p.hits, dlog(f, p), p.counters, p.batch_paths(), bounce, f->trace_variant, f->trace_waves_per_cu,
                           primary ? &g : nullptr};
    KernelSpan span(f, 1, p.stream);
    launch_trace<false>(f, t, p.o4[in], p.d4[in], (const uint32_t*)nullptr, &p.counters->queue[bounce]);
    HIPCHK(ctx, hipGetLastError());
    return RT_OK;
}

// ShadeMissedRays + ShadeSurfaceHits.  count_in_ray: whole samples (rt_integrate, the banks) -- nothing reads the radiance between their stages
int launch::shade_pipe(rt_frame* f, PathPipe& p, uint32_t bounce, bool count_in_ray)
{
    rt_ctx* ctx = f->ctx;
    uint32_t in = bounce & 1u, out = (bounce + 1u) & 1u;
    ShadeArgs a;
    a.in_o4 = p.o4[in]; a.in_d4 = p.d4[in]; a.in_thr = p.thr[in]; a.hits = p.hits;
    a.out_o4 = p.o4[out]; a.out_d4 = p.d4[out]; a.out_thr = p.thr[out];
    a.sh_o4 = p.sh_o4[bounce & 1u]; a.sh_d4 = p.sh_d4[bounce & 1u]; a.sh_aux = p.sh_aux[bounce & 1u];
    a.log = dlog(f, p); a.counters = p.counters;
    set_blue_noise(a, ctx);
    a.bounce = bounce; a.sample_base = f->sample_count;
    a.emit_outgoing = (f->drop_last && bounce >= f->max_bounces) ? 0u : 1u;
    a.n_local = f->chunk_pixels ? f->chunk_pixels : 1;
    a.pix_base = p.chunk_base;
    a.count_in_ray = count_in_ray ? 1u : 0u;
    a.partition = f->shade_partition;
    a.final_bounce = bounce >= f->max_bounces ? 1u : 0u;
    const bool primary = bounce == 0u && p.primary_fused;        // (rt_integrate's batches: count_in_ray)
    uint32_t blocks = ((uint32_t)p.batch_paths() + RT_SHADE_BLOCK - 1u) / RT_SHADE_BLOCK;
    if (blocks == 0) blocks = 1;
    p.shadow_pending = true;
    // this bounce refills shadow queue [bounce & 1] and rewinds its work heads: the shadow trace of bounce - 2 is done with them
    if (wait_shadow(f, p, bounce & 1u) != RT_OK) return RT_ERROR;
    KernelSpan span(f, 2, p.stream);
    const bool blue = f->sampler == 1;   // kernel variants are AOT (the reference rebuilds with -D..., :267-285)
    const bool nee = ctx->scene.d.emissive_nee != 0;     // opt-in extension (rt_scene_desc::flags)
#define RT_LAUNCH_SHADE(FURNACE, BLUE, NEE) \
    do { if (primary && f->log_ovf_blocks) hipLaunchKernelGGL((k_shade<FURNACE, BLUE, NEE, true, true>), dim3(blocks), dim3(RT_SHADE_BLOCK), 0, p.stream, ctx->scene.d, f->tile, a); \
         else if (primary) hipLaunchKernelGGL((k_shade<FURNACE, BLUE, NEE, false, true>), dim3(blocks), dim3(RT_SHADE_BLOCK), 0, p.stream, ctx->scene.d, f->tile, a); \
         else if (f->log_ovf_blocks) hipLaunchKernelGGL((k_shade<FURNACE, BLUE, NEE, true>), dim3(blocks), dim3(RT_SHADE_BLOCK), 0, p.stream, ctx->scene.d, f->tile, a); \
         else hipLaunchKernelGGL((k_shade<FURNACE, BLUE, NEE, false>), dim3(blocks), dim3(RT_SHADE_BLOCK), 0, p.stream, ctx->scene.d, f->tile, a); } while (0)
    if (nee)
    {
        if (f->white_furnace && blue) RT_LAUNCH_SHADE(true, true, true);
        else if (f->white_furnace) RT_LAUNCH_SHADE(true, false, true);
        else if (blue) RT_LAUNCH_SHADE(false, true, true);
        else RT_LAUNCH_SHADE(false, false, true);
    }
    else if (f->white_furnace && blue) RT_LAUNCH_SHADE(true, true, false);
    else if (f->white_furnace) RT_LAUNCH_SHADE(true, false, false);
    else if (blue) RT_LAUNCH_SHADE(false, true, false);
    else RT_LAUNCH_SHADE(false, false, false);
#undef RT_LAUNCH_SHADE
    HIPCHK(ctx, hipGetLastError());
    f->side_active = side_on(f);
    if (f->side_active) HIPCHK(ctx, hipEventRecord(p.ev_shaded, p.stream));
    return RT_OK;
}

// IntersectShadowRays + AccumulateDirectSamples: the trace of pipe p's shadow queue of `bounce`, on the side stream where the shade step chose it
int launch::shadow_pipe(rt_frame* f, PathPipe& p, uint32_t bounce)
{
    rt_ctx* ctx = f->ctx;
    const uint32_t q = bounce & 1u;
    const TraceTarget t = {f->side_active ? p.side : p.stream, p.sh_spill, p.sh_slow_list, 1u + q, nullptr, dlog(f, p), p.counters, p.batch_paths(), bounce,
                           f->trace_variant, f->trace_waves_per_cu};
    if (f->side_active) HIPCHK(ctx, hipStreamWaitEvent(p.side, p.ev_shaded, 0));
    {
        KernelSpan span(f, 3, t.stream);
        launch_trace<true>(f, t, p.sh_o4[q], p.sh_d4[q], (const uint32_t*)p.sh_aux[q], &p.counters->shadow[bounce]);
    }
    p.shadow_pending = false;
    HIPCHK(ctx, hipGetLastError());
    if (f->side_active)
    {
        HIPCHK(ctx, hipEventRecord(p.ev_shadow[q], p.side));
        p.shadow_in_flight[q] = true;
    }
    return RT_OK;
}

extern "C" {

int rt_compute_aovs(rt_frame* f)                        // ComputeAOVs, :541-562 (after rt_intersect(frame, 0))
{
    FRAME_PROLOGUE(f, "rt_compute_aovs");
    if (f->aov == 0 && !f->denoiser) return RT_OK;      // outputs unobservable: skip the work
    const PathPipe& p = f->ps[0];                       // (AOVs need the whole tile in one chunk: it travels on pipe 0)
    if (p.cur_slots != 1) return fail(ctx, "rt_compute_aovs: AOVs need one sample in flight (use the stage API or rt_integrate with the denoiser/AOV option set)");
    if (f->n_local == 0) return RT_OK;
    uint32_t blocks = (f->n_local + 255u) / 256u;
    hipLaunchKernelGGL(k_aov_clear, dim3(blocks), dim3(256), 0, ctx->stream, f->aov_buf, f->n_local);
    hipLaunchKernelGGL(k_aov, dim3(blocks), dim3(256), 0, ctx->stream, ctx->scene.d, (const float4*)p.o4[0],
        (const float4*)p.d4[0], (const float4*)p.hits, (const uint32_t*)&p.counters->queue[0], f->camera, f->prev_camera,
        rt_tanf(0.5f * f->camera.fov), rt_tanf(0.5f * f->prev_camera.fov), f->aov_buf);
    HIPCHK(ctx, hipGetLastError());
    return RT_OK;
}

int rt_denoise(rt_frame* f)                             // Denoise, :665-668
{
    FRAME_PROLOGUE(f, "rt_denoise");
    if (f->denoiser != 1 || f->n_local == 0) return RT_OK;   // 2: rt_group_denoise does it on the gathered image
    if (flush_log(f, f->ps[0]) != RT_OK) return RT_ERROR;
    uint32_t blocks = (f->n_local + 255u) / 256u;
    hipLaunchKernelGGL(k_denoise, dim3(blocks), dim3(256), 0, ctx->stream, f->tile.width, f->tile.height, f->radiance,
        (const float4*)f->prev_radiance, (const float*)f->aov_buf.depth, (const float*)f->prev_depth,
        (const float2*)f->aov_buf.velocity);
    HIPCHK(ctx, hipGetLastError());
    return RT_OK;
}

int rt_copy_history(rt_frame* f)                        // CopyHistoryBuffers, :670-675
{
    FRAME_PROLOGUE(f, "rt_copy_history");
    if (f->denoiser != 1 || f->n_local == 0) return RT_OK;
    HIPCHK(ctx, hipMemcpyAsync(f->prev_radiance, f->radiance, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToDevice,
        ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(f->prev_depth, f->aov_buf.depth, (size_t)f->n_local * sizeof(float), hipMemcpyDeviceToDevice,
        ctx->stream));
    return RT_OK;
}

} // extern "C"

// RT_OPT_SAMPLES_AHEAD: slot `slot` of bank h's log, replayed into the radiance of its owner f on the context's stream (ahead_consume, frame_schedule.cpp)
int launch::replay_bank_slot(rt_frame* f, rt_frame* h, uint32_t slot)
{
    rt_ctx* ctx = f->ctx;
    const uint32_t blocks = (f->n_local + 255u) / 256u;
    hipLaunchKernelGGL(k_flush, dim3(blocks), dim3(256), 0, ctx->stream, f->radiance, dlog(h, h->ps[0]), f->n_local, 1u, h->chunk_pixels, 0u, slot);
    HIPCHK(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" {

// ---- output ----------------------------------------------------------------
int rt_frame_present_wait(rt_frame* f)
{
    if (!f) return fail(nullptr, "rt_frame_present_wait: frame is NULL");
    if (!f->present_pending) return RT_OK;
    (void)hipSetDevice(f->ctx->device);
    HIPCHK(f->ctx, hipEventSynchronize(f->ev_copied[(f->present_flip ^ 1u) & 1u]));      // the latest copy (its stream carries later frames' work too)
    f->present_pending = false;
    return RT_OK;
}

// ResolveRadiance + Finish() AS THE REFERENCE HAS THEM (cl_pt_integrator.cpp:677-684): the kernels have finished when this
// returns; the resolved image is on its way.  The reference resolves into a GL image its window blits later -- nothing crosses
// PCIe at all; headless, the image has to reach the host, and it does so on a copy stream of its own, double-buffered on the
// device, while the next frame's rays are already being traced (0.6 of the 4.7 ms of a 1080p frame were this read-back).
int rt_frame_present(rt_frame* f, float* host_rgba)
{
    if (!f || !host_rgba) return fail(nullptr, "rt_frame_present: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (f->n_local == 0) return RT_OK;
    if (!f->present_stream)
    {
        // all or nothing: a frame whose second image could not be allocated keeps presenting through rt_frame_resolve's path
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        hipStream_t st = nullptr;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        float4* second = nullptr;
        bool ok = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo) == hipSuccess;           // (used only by a frame without a side stream)
        for (hipEvent_t& e : ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMalloc((void**)&second, (size_t)f->n_local * sizeof(float4)) == hipSuccess;
        ok = ok && hipEventRecord(ev[2], st) == hipSuccess && hipEventRecord(ev[3], st) == hipSuccess;
        if (!ok)
        {
            (void)hipGetLastError();
            if (second) (void)hipFree(second);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            if (st) (void)hipStreamDestroy(st);
            return rt_frame_resolve(f, host_rgba);       // the synchronous form: same image, no overlap
        }
        f->present_stream = st; f->resolved_b = second;
        f->ev_resolved[0] = ev[0]; f->ev_resolved[1] = ev[1]; f->ev_copied[0] = ev[2]; f->ev_copied[1] = ev[3];
    }
    if (flush_stage(f) != RT_OK) return RT_ERROR;
    const uint32_t i = f->present_flip & 1u;
    float4* image = i ? f->resolved_b : f->resolved;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, f->ev_copied[i], 0));      // the copy that last read this device image (two frames ago)
    uint32_t blocks = (f->n_local + 255u) / 256u;
    hipLaunchKernelGGL(k_resolve, dim3(blocks), dim3(256), 0, ctx->stream, (const float4*)f->radiance, f->aov_buf,
        image, f->n_local, f->sample_count, f->aov, f->denoiser);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(f->ev_resolved[i], ctx->stream));
    // The copy goes to pipe 0's SIDE stream (where the shadow traces run), not to a stream of its own: which hardware queue a further stream lands
    // on is the runtime's business, and when it was the side stream's the copy's completion barrier held the next frame's shadow traces back for
    // the whole 0.6 ms -- in rt_render's process with a low-priority copy stream (3.87 instead of 3.33 ms per frame), in bench.py's (PyTorch has
    // made streams before) with a normal-priority one (3.86 instead of 3.38): profiles/r05_call19.log.  On the side stream itself the order is
    // explicit and harmless: the copy is enqueued at the end of frame N and runs while frame N + 1 generates, traces and shades its camera rays --
    // longer than the copy takes -- before that frame's first shadow trace is enqueued behind it.  3.30 / 3.31 ms per frame in both processes.
    hipStream_t const copy_stream = f->ps[0].side ? f->ps[0].side : f->present_stream;
    HIPCHK(ctx, hipStreamWaitEvent(copy_stream, f->ev_resolved[i], 0));
    // (The runtime's copy of a page-locked destination is a blit kernel, 441 us for a 1080p image; a 64-block copy kernel of our
    // own that left the other CUs alone was tried and is SLOWER end to end -- it holds PCIe for milliseconds and every persistent
    // grid launched meanwhile finds part of its residency taken: 4.22 instead of 3.70 ms per frame, profiles/r04_call07_*.  The
    // stream's low priority is what keeps the blit's workgroups behind the next frame's first launches.)
    HIPCHK(ctx, hipMemcpyAsync(host_rgba, image, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToHost, copy_stream));
    HIPCHK(ctx, hipEventRecord(f->ev_copied[i], copy_stream));
    f->present_flip ^= 1u;
    f->present_pending = true;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // Finish(), :682: every kernel of the frame has run
    return RT_OK;
}

int rt_frame_resolve(rt_frame* f, float* host_rgba)     // ResolveRadiance, :677-684
{
    if (!f || !host_rgba) return fail(nullptr, "rt_frame_resolve: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (f->n_local == 0) return RT_OK;
    if (rt_frame_present_wait(f) != RT_OK) return RT_ERROR;                // an image still travelling to (possibly) the same host buffer
    if (flush_stage(f) != RT_OK) return RT_ERROR;
    uint32_t blocks = (f->n_local + 255u) / 256u;
    hipLaunchKernelGGL(k_resolve, dim3(blocks), dim3(256), 0, ctx->stream, (const float4*)f->radiance, f->aov_buf,
        f->resolved, f->n_local, f->sample_count, f->aov, f->denoiser);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(host_rgba, f->resolved, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToHost,
        ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // the frame's only host sync, like Finish() at :682
    return RT_OK;
}

} // extern "C"

// The spatial and temporal filters and the readers that launch no kernel are units of their own (frame_filters.cpp, frame_readers.cpp, on frame.h).  What stays
// here of the filters is the guide pass's one launch of this unit's code object.
void frame::trace_guides(rt_frame* f, const float4* o4, const float4* d4, float4* hits, uint2* spill, const uint32_t* count, size_t n)
{
    rt_ctx* ctx = f->ctx;
    {
        // the closest-hit trace through launch_trace's per-ray kernel k_trace_v1<false> (variant 0: the reference's BVH2 walk; waves 0: the grid is trace_blocks), on the
        // context's stream with the filter's own hits and spill area; a closest-hit trace logs nothing and that kernel counts nothing.  (Through launch_trace and
        // not a launch of its own: a new use of the template kernel here moves where clang places its code, and the hot path's code object --
        // codeobj.code_object_sha256 -- must stay byte for byte what it is.)
        const TraceTarget t = {ctx->stream, spill, nullptr, 0u, hits, DLog{}, nullptr, (uint64_t)n, 0u, 0u, 0u};
        launch_trace<false>(f, t, o4, d4, (const uint32_t*)nullptr, count);
    }
}

extern "C" {

int rt_frame_get_stats(rt_frame* f, rt_stats* out)
{
    if (!f || !out) return fail(nullptr, "rt_frame_get_stats: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (f->deferred.active && deferred_materialize(f) != RT_OK) return RT_ERROR;     // RT_OPT_FRAME_KERNEL: the counters of the stages recorded so far
    if (join_pipes(f) != RT_OK || sync_frame_streams(f) != RT_OK) return RT_ERROR;   // a shadow trace on a side stream still counts rays
    memset(out, 0, sizeof(*out));
    for (uint32_t i = 0; i < RT_MAX_PIPES; ++i)              // the pipes' counters add up
    {
        PathPipe& q = f->ps[i];
        if (!q.counters) continue;
        hipLaunchKernelGGL(k_fold_counters, dim3(1), dim3(64), 0, ctx->stream, q.counters, q.prev_bounces, q.fold_accumulates);
        q.fold_accumulates = 1;       // whatever is folded next belongs to the same batch's totals unless a new batch starts
        DCounters h;
        HIPCHK(ctx, hipMemcpyAsync(&h, q.counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        out->closest_rays += h.total_closest;
        out->shadow_rays += h.total_shadow;
        out->stack_spills += h.stack_spills;
        out->slow_rays += h.slow_rays;
        if (i < f->n_pipes)
            for (int b = 0; b < 64; ++b) { out->last_active[b] += h.last_queue[b]; out->last_shadow[b] += h.last_shadow[b]; }
    }
    out->samples = f->sample_count;
    out->samples_in_flight = f->slots;
    out->samples_in_flight_limit = f->slots_limit;
    out->path_state_bytes = (uint64_t)f->log_stride * bytes_per_path(f, f->log_ovf_blocks ? f->slots : 1u) * f->n_pipes;
    out->log_inline_entries = f->log_ovf_blocks ? f->log_inline : 0u;
    out->log_fallbacks = f->log_fallbacks;
    out->frame_kernel_samples = (uint32_t)f->frame_launches;
    out->fused_raygen_launches = f->fused_launches;
    out->chunk_pixels = f->chunk_pixels;
    out->pipelines = f->n_pipes;
    if (f->ahead)
    {
        // RT_OPT_SAMPLES_AHEAD: the rays of the samples that came out of the banks were counted there -- whole batches at a time, so the totals
        // include `samples_ahead` samples that `samples` does not yet
        for (const AheadBank& b : f->ahead->bank)
        {
            if (!b.h) continue;
            rt_stats hs;
            if (rt_frame_get_stats(b.h, &hs) != RT_OK) return RT_ERROR;
            out->closest_rays += hs.closest_rays; out->shadow_rays += hs.shadow_rays;
            out->stack_spills += hs.stack_spills; out->slow_rays += hs.slow_rays;
            out->path_state_bytes += hs.path_state_bytes;
            out->samples_ahead += b.n - b.next;
        }
        out->samples_from_banks = f->ahead->consumed;
    }
    return RT_OK;
}

int rt_debug_eval(rt_ctx* ctx, int fn, const float* a, const float* b, float* out, uint32_t n)
{
    if (!ctx || !a || !out) return fail(ctx, "rt_debug_eval: NULL argument");
    (void)hipSetDevice(ctx->device);
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    struct Free { float*& a; float*& b; float*& c; ~Free() { for (float* p : {a, b, c}) if (p) (void)hipFree(p); } } guard{da, db, dout};
    HIPCHK(ctx, hipMalloc((void**)&da, (size_t)n * 4 + 16));
    HIPCHK(ctx, hipMalloc((void**)&dout, (size_t)n * 4 + 16));
    HIPCHK(ctx, hipMemcpy(da, a, (size_t)n * 4, hipMemcpyHostToDevice));
    if (b)
    {
        HIPCHK(ctx, hipMalloc((void**)&db, (size_t)n * 4 + 16));
        HIPCHK(ctx, hipMemcpy(db, b, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_debug_eval, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fn, da, db, dout, n);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

} // extern "C"

#include "group_impl.h"
