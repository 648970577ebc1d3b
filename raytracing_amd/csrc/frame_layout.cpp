// frame_layout.cpp -- what a frame is made of and how it is laid out: its creation and destruction, the per-path buffers (how many samples travel together,
// how the tile is cut into chunks and dealt to pipes, the full and the compact log layout), the pipes' streams and their ordering, the frame's options, camera
// and reset, and the three picks.  Host code only, on frame.h and frame_launch.h: the only launch it needs is the log's replay before buffers change hands
// (launch::flush_log, rt_hip.hip's); the banks and the measuring schedule it tells of a change are frame_schedule.cpp's.  Replaces the frame's half of the
// reference's src/integrator/cl_pt_integrator.cpp (ctor, Reset, the option setters).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <assert.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "query_host.h"      // the ray through a pixel, for rt_frame_pick and rt_frame_pick_all (query.hip)
#include "region_host.h"     // the region of a pixel rectangle, for rt_frame_pick_rect (region.hip)
#include "context.h"         // rt_ctx, fail / HIPCHK
#include "frame.h"           // rt_frame, its pipes, banks and buffer lists
#include "frame_launch.h"    // launch::flush_log; the layout's own functions as the other units see them
using namespace context;
using namespace frame;
using namespace launch;

// ---- frame -----------------------------------------------------------------
namespace
{
void free_path_buffers(rt_frame* f)
{
    // a shadow trace may still be running on a pipe's side stream (rt_integrate overlaps it with the next bounce, and an
    // rt_integrate that failed mid-bounce never waited for it): nothing is freed under it
    for (PathPipe& q : f->ps)
    {
        if (q.side) (void)hipStreamSynchronize(q.side);
        q.shadow_in_flight[0] = q.shadow_in_flight[1] = false;
    }
    for (PathPipe& q : f->ps) free_buffers(q.buffers());
}
} // namespace

// Per-path state: ray queues for `slots` samples in flight and the radiance log
// with 2 * (max_bounces + 1) entries per path.  (Re)allocated when either changes.
// Compact radiance log (kernels_common.h, DLog): six inline entries per path + overflow blocks for an eighth of the paths.
#define RT_LOG_INLINE 6u
// may a batch of `slots` samples in flight use the compact layout?  (It pays from ~10 entries per path up, needs batches large
// enough for the pool's statistics, and one pipe: the pool-dry check synchronises the host with the chunk's stream.)
bool frame::log_is_compact(const rt_frame* f, uint32_t slots)
{
    const bool asked = f->compact_log_opt == 1u || (f->compact_log_opt == 2u && f->state_limit_mb != 0u);
    return asked && !f->log_full_forced && slots >= 8u && f->pipelines == 1u && 2u * (f->max_bounces + 1u) >= RT_LOG_INLINE + 4u;
}

// A path's bytes in the full layout: the fixed buffers + a log of 2 (B + 1) entries of 12 bytes -- 412 bytes at 8 bounces (rounds 1-2: 540).
size_t frame::full_bytes_per_path(uint32_t max_bounces) { return RT_PATH_FIXED_BYTES + 12u * 2u * (max_bounces + 1u); }

// ... and in the layout a batch of `slots` samples in flight gets; compact: 6 inline entries + the path's share of the overflow pool + its block
// index -- 290 bytes at 8 bounces, 314 at 16.
size_t frame::bytes_per_path(const rt_frame* f, uint32_t slots)
{
    if (!log_is_compact(f, slots)) return full_bytes_per_path(f->max_bounces);
    const size_t entries = 2u * (f->max_bounces + 1u);
    return RT_PATH_FIXED_BYTES + 4u + 12u * RT_LOG_INLINE + (12u * (entries - RT_LOG_INLINE) + f->log_pool_div - 1u) / f->log_pool_div;
}

namespace
{
// auto: the most samples (<= 1024; a multiple of 8 above 8, of 16 above 64 -- rounds 1-2 took powers of two, which left up to
// half of the budget unused: a 4K frame with 16 bounces got 16 samples in flight where 24 fit) that keep tile pixels x
// samples inside 32-bit path ids and the per-path buffers under 144 GiB (half of the 288 GB of HBM)
uint32_t auto_slots(const rt_frame* f)
{
    const uint64_t n = tile_pixels(f);
    const uint64_t max_paths = 0xFFFFFFF0ull;
    uint64_t by_memory = (144ull << 30) / (n * bytes_per_path(f, 1024u));        // the compact layout, if this frame may use it ...
    if (by_memory < 8u) by_memory = (144ull << 30) / (n * bytes_per_path(f, 1u));  // ... which takes 8 samples in flight
    const uint64_t by_ids = max_paths / n;
    uint64_t s = by_memory < by_ids ? by_memory : by_ids;
    // ... and no more than fill a launch: beyond ~270 M paths in flight (128 samples of a 1080p frame) a larger batch buys
    // nothing (176 in flight, 140 GB: 6112 Mrays/s; 128, 102 GB: 6195 -- profiles/r03_call02_bench.json, r03_mid_bench.json)
    const uint64_t by_fill = (270000000ull + n - 1) / n;
    if (s > by_fill) s = by_fill;
    if (s > 1024) s = 1024;
    if (s > 64) s &= ~15ull;
    else if (s > 8) s &= ~7ull;
    return s ? (uint32_t)s : 1u;
}
} // namespace

// the most samples rt_integrate will trace together
uint32_t frame::slot_cap(const rt_frame* f)
{
    uint32_t cap = f->slots_opt ? f->slots_opt : auto_slots(f);
    return f->slots_limit && f->slots_limit < cap ? f->slots_limit : cap;    // what the device could actually hold
}

// How the tile is cut for `slots` samples in flight: number of pipes and pixels per chunk.
//  * two (RT_OPT_PIPELINES) pipes when a batch is large enough for its launches to fill the machine twice over
//    (>= 2 samples in flight and >= 4 M paths): the tile's halves then overlap each other's launch tails;
//  * RT_OPT_PATH_STATE_LIMIT_MB bounds the per-path buffers of all pipes together: more, smaller chunks
//    (multiples of 4096 pixels), still dealt round-robin to the pipes.
void frame::chunk_plan(const rt_frame* f, uint32_t slots, uint32_t& n_pipes, uint32_t& chunk_pixels)
{
    const uint64_t n = tile_pixels(f);
    slots = slots ? slots : 1u;
    n_pipes = 1;
    if (f->pipelines > 1 && slots >= 2 && n * slots >= 4000000ull) n_pipes = f->pipelines < RT_MAX_PIPES ? f->pipelines : RT_MAX_PIPES;
    // one sample per pixel in flight (RT_OPT_STAGE_PIPES): the interactive features need the whole tile in one chunk
    if (f->stage_pipes > 1 && slots == 1 && n >= 262144ull && !(f->denoiser || f->aov != 0)) n_pipes = f->stage_pipes < RT_MAX_PIPES ? f->stage_pipes : RT_MAX_PIPES;
    uint64_t c = (n + n_pipes - 1) / n_pipes;                        // pixels per chunk without a memory limit
    if (n_pipes > 1) c = (c + 63ull) & ~63ull;
    // the caller's limit, and -- after a batch had to fall back from the compact to the full log layout -- the library's own
    // 144 GiB rule (the full layout then runs the same batch size in more chunks instead of asking for more memory than that)
    const uint64_t limit_mb = f->state_limit_mb && f->fallback_limit_mb ? (f->state_limit_mb < f->fallback_limit_mb ? f->state_limit_mb : f->fallback_limit_mb)
                                                                         : (f->state_limit_mb ? f->state_limit_mb : f->fallback_limit_mb);
    if (limit_mb)
    {
        const uint64_t per_pixel = (uint64_t)slots * bytes_per_path(f, slots);
        const uint64_t limit = (limit_mb << 20) / n_pipes;
        if (c * per_pixel > limit)
        {
            c = (limit / per_pixel) & ~4095ull;
            if (c < 4096) c = 4096;
        }
    }
    chunk_pixels = (uint32_t)(c < n ? c : n);
    if ((uint64_t)chunk_pixels * n_pipes > n + chunk_pixels) n_pipes = (uint32_t)((n + chunk_pixels - 1) / chunk_pixels);
}

uint32_t frame::chunk_for(const rt_frame* f, uint32_t slots)
{
    uint32_t np, c;
    chunk_plan(f, slots, np, c);
    return c;
}

int frame::alloc_path_buffers(rt_frame* f, uint32_t slots)
{
    rt_ctx* ctx = f->ctx;
    free_path_buffers(f);
    // test hook (tests/test_gpu_headline_parity.py): pretend the device cannot hold more than N samples in flight
    if (f->debug_alloc_limit && slots > f->debug_alloc_limit)
        return fail(ctx, "out of device memory for the per-path buffers (RT_OPT_DEBUG_ALLOC_LIMIT)");
    f->slots = slots ? slots : 1u;
    chunk_plan(f, f->slots, f->n_pipes, f->chunk_pixels);
    uint64_t paths = (uint64_t)f->chunk_pixels * f->slots;
    if (paths > 0xFFFFFFF0ull) return fail(ctx, "samples in flight x tile pixels exceeds the 32-bit path-id range");
    f->log_stride = (uint32_t)paths;
    f->log_entries = 2u * (f->max_bounces + 1u);
    const bool compact = log_is_compact(f, f->slots);
    f->log_inline = compact ? RT_LOG_INLINE : f->log_entries;
    f->log_ovf_blocks = compact ? (uint32_t)(paths / f->log_pool_div > 64u ? paths / f->log_pool_div : 64u) : 0u;
    const size_t log_elems = (size_t)f->log_inline * paths + (size_t)(f->log_entries - f->log_inline) * f->log_ovf_blocks;
    // RT_PATH_FIXED_BYTES is the list's own sum: what one more path adds to everything but the log
    assert(total_bytes(PathPipe().buffers(2, 0, false)) - total_bytes(PathPipe().buffers(1, 0, false)) == RT_PATH_FIXED_BYTES);
    bool ok = true;
    for (uint32_t i = 0; i < f->n_pipes && ok; ++i)
    {
        PathPipe& pp = f->ps[i];
        for (const DevBuf& b : pp.buffers((size_t)paths, log_elems, compact)) ok = ok && hipMalloc(b.p, b.bytes) == hipSuccess;
        // ordered on the context's stream: the pipes' streams wait for it before their first launch (fork_pipes)
        ok = ok && hipMemsetAsync(pp.cnt, 0, (size_t)paths * sizeof(uint32_t), ctx->stream) == hipSuccess;
        pp.cur_slots = 0;
        pp.chunk_base = 0;
        pp.chunk_count = 0;
        pp.shadow_pending = false;
    }
    if (!ok)
    {
        free_path_buffers(f);
        (void)hipGetLastError();      // the failed hipMalloc is handled here: do not let it surface at the next launch check
        return fail(ctx, "out of device memory for the per-path buffers");
    }
    return RT_OK;
}

// Cross-stream ordering.  fork: the pipes' own streams wait for everything enqueued on the context's stream
// so far; join: the context's stream waits for everything the pipes have been given.
int frame::fork_pipes(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    if (f->n_pipes <= 1) return RT_OK;
    HIPCHK(ctx, hipEventRecord(f->ps[0].done, ctx->stream));
    for (uint32_t i = 1; i < f->n_pipes; ++i) HIPCHK(ctx, hipStreamWaitEvent(f->ps[i].stream, f->ps[0].done, 0));
    return RT_OK;
}

int frame::join_pipes(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    for (uint32_t i = 1; i < RT_MAX_PIPES; ++i)
    {
        if (!f->ps[i].stream) continue;
        HIPCHK(ctx, hipEventRecord(f->ps[i].done, f->ps[i].stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, f->ps[i].done, 0));
    }
    return RT_OK;
}

namespace
{

// stream, event, counters and spill area of pipes 0 .. count-1 (created once, kept for the frame's life)
int ensure_pipe_resources(rt_frame* f, uint32_t count)
{
    rt_ctx* ctx = f->ctx;
    if (count > RT_MAX_PIPES) count = RT_MAX_PIPES;
    // worst case over the kernel variants: 32 one-wave blocks per CU, 8-entry LDS stack
    const size_t spill_bytes = (size_t)ctx->prop.multiProcessorCount * 32 * 64 * (RT_W4_STACK_MAX - 8) * sizeof(uint2);
    for (uint32_t i = 0; i < (count ? count : 1u); ++i)
    {
        PathPipe& q = f->ps[i];
        if (!q.stream)
        {
            if (i == 0) q.stream = ctx->stream;
            else HIPCHK(ctx, hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking));
        }
        if (!q.done) HIPCHK(ctx, hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
        if (!q.side)
        {
            // lower priority than the main stream: when both have workgroups waiting, the closest-hit trace and
            // k_shade (the critical chain of a bounce) get the free slots first
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            HIPCHK(ctx, hipStreamCreateWithPriority(&q.side, hipStreamNonBlocking, lo));
            HIPCHK(ctx, hipEventCreateWithFlags(&q.ev_shaded, hipEventDisableTiming));
            for (hipEvent_t& e : q.ev_shadow) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        if (!q.counters)
        {
            HIPCHK(ctx, hipMalloc((void**)&q.counters, sizeof(DCounters)));
            HIPCHK(ctx, hipMemsetAsync(q.counters, 0, sizeof(DCounters), ctx->stream));
        }
        if (!q.spill) HIPCHK(ctx, hipMalloc((void**)&q.spill, spill_bytes));
        if (!q.sh_spill) HIPCHK(ctx, hipMalloc((void**)&q.sh_spill, spill_bytes));
    }
    return RT_OK;
}

} // namespace

// The pipe's main stream waits for the shadow trace that last used its shadow queue `q` (those run on PathPipe::side);
// nothing to do when none is outstanding.
int frame::wait_shadow(rt_frame* f, PathPipe& p, uint32_t q)
{
    if (!p.shadow_in_flight[q]) return RT_OK;
    HIPCHK(f->ctx, hipStreamWaitEvent(p.stream, p.ev_shadow[q], 0));
    p.shadow_in_flight[q] = false;
    return RT_OK;
}

// Does the shadow trace of this bounce go to the pipe's side stream?  Inside rt_integrate AND through the stage API (the
// reference's own call pattern, one Integrate() per frame: its launches are small, and the shadow trace of bounce b beside
// the closest-hit trace of bounce b + 1 fills the machine twice as well).  Everything that reads what a shadow trace writes
// waits for it: k_shade(b + 2) (wait_shadow), the log replay (flush_log), rt_reset, the debug readers.
bool frame::side_on(const rt_frame* f) { return f->overlap_shadow != 0 && !(f->denoiser || f->aov != 0); }

// Grows the per-path buffers to hold `want` samples in flight (clamped to slot_cap); they
// are sized by the largest batch actually requested, not by the cap.
int frame::ensure_slots(rt_frame* f, uint32_t want)
{
    uint32_t cap = slot_cap(f);
    if (want > cap) want = cap;
    if (want <= f->slots && 2u * (f->max_bounces + 1u) <= f->log_entries && f->chunk_pixels == chunk_for(f, f->slots) &&
        (f->log_ovf_blocks != 0u) == log_is_compact(f, f->slots))
        return RT_OK;
    if (flush_log(f, f->ps[0]) != RT_OK || join_pipes(f) != RT_OK) return RT_ERROR;
    HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));
    uint32_t keep = f->slots < cap ? f->slots : cap;
    uint32_t n = want > keep ? want : keep;
    // HBM shared with other frames / processes: halve the batch until the buffers fit
    while (alloc_path_buffers(f, n) != RT_OK)
    {
        if (n == 1) return RT_ERROR;
        n = n > 2u * keep && keep > 0 ? n / 2u : (n > keep ? keep : n / 2u);
        if (n == 0) n = 1;
        f->slots_limit = n;
    }
    return RT_OK;
}

// The stage API and the per-frame features (AOVs, denoiser) trace ONE sample of the WHOLE tile.  The buffers may have
// been cut into chunks for an earlier, larger batch under RT_OPT_PATH_STATE_LIMIT_MB (ensure_slots keeps an allocation
// that is large enough in SLOTS): re-allocate for one sample in flight, which the caller has checked does fit.
int frame::ensure_whole_tile(rt_frame* f)
{
    if (f->chunk_pixels >= tile_pixels(f)) return RT_OK;
    if (f->ps[0].cur_slots != 0) return fail(f->ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
    if (flush_log(f, f->ps[0]) != RT_OK || join_pipes(f) != RT_OK) return RT_ERROR;
    HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return alloc_path_buffers(f, 1);
}

// waits (host side) for every stream a frame launches on besides the context's own
int frame::sync_frame_streams(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    for (PathPipe& q : f->ps)
    {
        if (q.stream && q.stream != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(q.stream));
        if (q.side) HIPCHK(ctx, hipStreamSynchronize(q.side));
    }
    if (f->present_stream) HIPCHK(ctx, hipStreamSynchronize(f->present_stream));   // an image on its way to the host (rt_frame_present)
    f->present_pending = false;
    return RT_OK;
}

namespace
{
// An option that decides the per-path layout changes (rt_set_option).  Nothing of this frame is in flight any more -- its log replayed, its pipes joined
// where the change moves chunks between them (`join`), the context's stream drained -- then `change` applies the new value and the buffers are laid out again.
//   change  returns the samples in flight to lay the buffers out for, 0 to leave them as they are, or -1 after a failure of its own
//   grow    the layout goes through ensure_slots (an allocation that is large enough stays), not alloc_path_buffers
//   undo    after a layout that failed: puts the old value back, and the buffers come back for the samples they held (nullptr: the new value stays)
int relayout(rt_frame* f, bool join, bool grow, const std::function<int()>& change, const std::function<void()>& undo = nullptr)
{
    if (flush_log(f, f->ps[0]) != RT_OK || (join && join_pipes(f) != RT_OK)) return RT_ERROR;
    HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));
    const uint32_t old_slots = f->slots;
    const int slots = change();
    if (slots <= 0) return slots < 0 ? RT_ERROR : RT_OK;
    if ((grow ? ensure_slots(f, (uint32_t)slots) : alloc_path_buffers(f, (uint32_t)slots)) == RT_OK) return RT_OK;
    if (undo) { undo(); (void)alloc_path_buffers(f, old_slots); }
    return RT_ERROR;
}
} // namespace

// borrowed_main_stream != NULL: pipe 0 launches there instead of on the context's stream (a bank of RT_OPT_SAMPLES_AHEAD; the stream stays the lender's)
int frame::create_frame(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out, hipStream_t borrowed_main_stream)
{
    if (!ctx || !fd || !out) return fail(ctx, "rt_frame_create: NULL argument");
    *out = nullptr;
    if (fd->width == 0 || fd->height == 0) return fail(ctx, "rt_frame_create: empty image");
    if (fd->tile_count == 0 || fd->tile_rank >= fd->tile_count || fd->band_height == 0)
        return fail(ctx, "rt_frame_create: bad tile description");
    (void)hipSetDevice(ctx->device);
    rt_frame* f = new rt_frame();
    f->ctx = ctx;
    f->tile.width = fd->width; f->tile.height = fd->height;
    f->tile.band_h = fd->band_height; f->tile.rank = fd->tile_rank; f->tile.nranks = fd->tile_count;
    uint32_t rows = 0;
    for (uint32_t band = fd->tile_rank; (uint64_t)band * fd->band_height < fd->height; band += fd->tile_count)
    {
        uint32_t start = band * fd->band_height;
        uint32_t h = fd->height - start < fd->band_height ? fd->height - start : fd->band_height;
        rows += h;
    }
    f->tile.local_rows = rows;
    if ((uint64_t)rows * fd->width > 0x7FFFFFFFull) { delete f; return fail(ctx, "rt_frame_create: tile too large"); }
    f->n_local = rows * fd->width;
    const size_t n = tile_pixels(f);
    f->trace_blocks = (uint32_t)ctx->prop.multiProcessorCount * 12u;
    f->trace_blocks = (f->trace_blocks + 7u) & ~7u;
    f->ps[0].stream = borrowed_main_stream;              // (NULL: ensure_pipe_resources gives pipe 0 the context's stream)
    bool ok = true;
    for (const DevBuf& b : f->images(n)) ok = ok && hipMalloc(b.p, b.bytes) == hipSuccess;
    for (const DevBuf& b : f->images(n)) if (b.clear) ok = ok && hipMemsetAsync(*b.p, 0, b.bytes, ctx->stream) == hipSuccess;
    ok = ok && alloc_path_buffers(f, 1) == RT_OK;     // grows on demand (ensure_slots)
    ok = ok && ensure_pipe_resources(f, f->pipelines) == RT_OK;
    if (!ok)
    {
        rt_frame_destroy(f);
        (void)hipGetLastError();
        return fail(ctx, "rt_frame_create: out of device memory");
    }
    memset(&f->camera, 0, sizeof(f->camera));
    memset(&f->camera_last, 0, sizeof(f->camera_last));
    memset(&f->prev_camera, 0, sizeof(f->prev_camera));
    *out = f;
    ctx->frames.push_back(f);
    return rt_reset(f);                                  // the reference ctor ends with Reset(), cl_pt_integrator.cpp:258
}

extern "C" {

int rt_frame_create(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out) { return create_frame(ctx, fd, out, nullptr); }

int rt_frame_destroy(rt_frame* f)
{
    if (!f) return RT_OK;
    (void)hipSetDevice(f->ctx->device);
    ahead_destroy(f);                                     // its banks first (frames of their own)
    f->ctx->frames.erase(std::remove(f->ctx->frames.begin(), f->ctx->frames.end(), f), f->ctx->frames.end());
    // every stream it launches on has drained before anything is freed
    for (PathPipe& q : f->ps) for (hipStream_t st : {q.stream, q.side}) if (st) (void)hipStreamSynchronize(st);
    if (f->present_stream) (void)hipStreamSynchronize(f->present_stream);
    (void)hipStreamSynchronize(f->ctx->stream);
    // device memory: the per-path buffers, the images, k_frame's buffers
    free_path_buffers(f);
    free_buffers(f->images());
    f->kf.release();
    if (f->resolved_b) (void)hipFree(f->resolved_b);
    // streams and events (pipe 0's stream is the context's or a bank owner's)
    for (uint32_t i = 0; i < RT_MAX_PIPES; ++i) f->ps[i].destroy(i > 0);
    if (f->present_stream) (void)hipStreamDestroy(f->present_stream);
    for (auto& pair : f->fk_auto.ev) for (hipEvent_t e : pair) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {f->ev_resolved[0], f->ev_resolved[1], f->ev_copied[0], f->ev_copied[1]}) if (e) (void)hipEventDestroy(e);
    for (auto& sp : f->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (auto e : f->event_pool) (void)hipEventDestroy(e);
    // the filters' states
    free_filter_state(f);
    delete f;
    return RT_OK;
}

uint32_t rt_frame_local_rows(rt_frame* f) { return f ? f->tile.local_rows : 0; }

uint32_t rt_frame_global_row(rt_frame* f, uint32_t ly)
{
    if (!f) return 0;
    uint32_t band = ly / f->tile.band_h;
    return (band * f->tile.nranks + f->tile.rank) * f->tile.band_h + (ly - band * f->tile.band_h);
}

int rt_set_option(rt_frame* f, int option, uint32_t value)
{
    if (!f) return fail(nullptr, "rt_set_option: frame is NULL");
    if (f->deferred.active && option != RT_OPT_FRAME_KERNEL && deferred_materialize(f) != RT_OK) return RT_ERROR;   // an option changed between two recorded stages
    if (f->ahead && option != RT_OPT_PROFILE_KERNELS && !(option == RT_OPT_MAX_BOUNCES && value == f->max_bounces) && !(option == RT_OPT_WHITE_FURNACE && (value ? 1u : 0u) == f->white_furnace))
        ahead_discard(f);                                 // (the two exceptions: HIPPathTraceIntegrator::SyncOptions sets them before every frame)
    switch (option)
    {
    case RT_OPT_SAMPLES_AHEAD:
        if ((value & 0xFFu) > 64u && (value & 0xFFu) != 255u) return fail(f->ctx, "rt_set_option: RT_OPT_SAMPLES_AHEAD is 0 (off), 1 (automatic depth) or 2..64 samples per batch (+ 256: one stream per bank)");
        if (f->ahead_owner) return fail(f->ctx, "rt_set_option: RT_OPT_SAMPLES_AHEAD on a bank");
        f->ahead_opt = value & 0x1FFu;
        if (f->ahead) f->ahead->configured = false;
        return RT_OK;
    case RT_OPT_MAX_BOUNCES:
        if (value > RT_MAX_BOUNCES_LIMIT) return fail(f->ctx, "rt_set_option: max_bounces above RT_MAX_BOUNCES_LIMIT");
        if (value == f->max_bounces) return RT_OK;
        fk_auto_restart(f);
        // log rows / payload split follow max_bounces; another path length: the compact layout gets another chance
        return relayout(f, false, true, [&]() { f->max_bounces = value; f->log_full_forced = false; f->fallback_limit_mb = 0; return 1; });
    case RT_OPT_SAMPLES_IN_FLIGHT:
    {
        if (value > 1024) return fail(f->ctx, "rt_set_option: samples in flight must be 0 (auto) or 1..1024");
        if (value == f->slots_opt) return RT_OK;
        const uint32_t old = f->slots_opt;
        // an explicit count is allocated now; auto (0) grows with the batches requested.  The caller decides anew how the buffers are sized: lean growth starts over
        return relayout(f, false, false, [&]() { f->slots_opt = value; f->reserved_explicitly = false; f->samples_asked = 0; return value ? (int)value : 1; },
                        [&]() { f->slots_opt = old; });
    }
    case RT_OPT_WHITE_FURNACE: f->white_furnace = value ? 1 : 0; return RT_OK;
    case RT_OPT_SAMPLER:
        if (value > 1) return fail(f->ctx, "rt_set_option: sampler must be 0 (kRandom) or 1 (kBlueNoise)");
        if (value == 1 && !f->ctx->blue_noise)
            return fail(f->ctx, "rt_set_option: SamplerType::kBlueNoise needs rt_upload_blue_noise_tables first");
        if (value != f->sampler) fk_auto_restart(f);
        f->sampler = value;
        return RT_OK;
    case RT_OPT_AOV:
        if (value > 4) return fail(f->ctx, "rt_set_option: AOV index must be 0..4");
        f->aov = value;
        return RT_OK;
    case RT_OPT_DENOISER:
        // 1: the frame runs TemporalAccumulation itself -- the reprojection crosses rows, so it needs the whole image;
        // 2: the frame only prepares the filter's inputs (reset every frame, one sample, depth and motion AOVs) and
        //    rt_group_denoise runs the filter on the gathered image: the mode for tiles.
        if (value > 2) return fail(f->ctx, "rt_set_option: RT_OPT_DENOISER is 0, 1 or 2");
        if (value == 1 && f->tile.nranks != 1)
            return fail(f->ctx, "rt_set_option: the temporal denoiser reprojects across rows and needs the whole image "
                                "on one GPU (tile_count == 1); on tiles use RT_OPT_DENOISER = 2 + rt_group_denoise");
        f->denoiser = value;
        return RT_OK;
    case RT_OPT_TRACE_DROP_LAST_BOUNCE_RAYS:
        if ((value ? 1u : 0u) != f->drop_last) fk_auto_restart(f);
        f->drop_last = value ? 1 : 0;
        return RT_OK;
    case RT_OPT_PROFILE_KERNELS: f->profile = value ? 1 : 0; return RT_OK;
    case RT_OPT_TRACE_WAVES_PER_CU: f->trace_waves_per_cu = value; return RT_OK;
    case RT_OPT_TRACE_PACKET_BOUNCES:
        if (value != 0) return fail(f->ctx, "rt_set_option: the packet kernel was removed (RT_OPT_TRACE_PACKET_BOUNCES accepts only 0)");
        return RT_OK;
    case RT_OPT_TRACE_SELECT_FORM_BOX: f->select_form_box = value ? RT_SIGN_SLOW : 0u; return RT_OK;
    case RT_OPT_TRACE_TUNE: f->trace_tune = value; return RT_OK;
    case RT_OPT_SHADE_PARTITION: f->shade_partition = value & 3u; return RT_OK;
    case RT_OPT_OVERLAP_SHADOW: f->overlap_shadow = value ? 1u : 0u; return RT_OK;
    case RT_OPT_PIPELINES:
        if (value == 0 || value > RT_MAX_PIPES) return fail(f->ctx, "rt_set_option: pipelines must be 1..RT_MAX_PIPES");
        if (value == f->pipelines) return RT_OK;
        return relayout(f, true, false, [&]() { if (ensure_pipe_resources(f, value) != RT_OK) return -1; f->pipelines = value; return (int)f->slots; });
    case RT_OPT_FRAME_KERNEL:
        if (f->deferred.active) return fail(f->ctx, "rt_set_option: RT_OPT_FRAME_KERNEL cannot change while a sample is in flight (rt_advance_sample first)");
        if (value == f->frame_kernel) return RT_OK;
        HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));
        f->kf.release();                                  // (the grid and its buffers are sized by the value: the next launch makes them again)
        f->frame_kernel = value == 255u ? 255u : (value > 64u ? 64u : value);
        fk_auto_restart(f);
        return RT_OK;
    case RT_OPT_STAGE_PIPES:
        if (value == 0 || value > RT_MAX_PIPES) return fail(f->ctx, "rt_set_option: stage pipes must be 1..RT_MAX_PIPES");
        if (value == f->stage_pipes) return RT_OK;
        if (f->ps[0].cur_slots != 0) return fail(f->ctx, "rt_set_option: RT_OPT_STAGE_PIPES cannot change while a sample is in flight (rt_advance_sample first)");
        return relayout(f, true, false, [&]() { if (ensure_pipe_resources(f, value) != RT_OK) return -1; f->stage_pipes = value; f->stage_chunks = 1; return f->slots == 1 ? 1 : 0; });
    case RT_OPT_PATH_STATE_LIMIT_MB:
    {
        if (value == f->state_limit_mb) return RT_OK;
        const uint32_t old = f->state_limit_mb;
        return relayout(f, false, false, [&]() { f->state_limit_mb = value; return (int)f->slots; }, [&]() { f->state_limit_mb = old; });
    }
    case RT_OPT_DEBUG_ALLOC_LIMIT: f->debug_alloc_limit = value; return RT_OK;
    case RT_OPT_SMALL_LAUNCH_PATHS: f->small_launch_paths = value; f->small_launch_set = true; return RT_OK;
    case RT_OPT_TRACE_TAIL_LANES: f->trace_tail_lanes = value > 64u ? 64u : value; return RT_OK;
    case RT_OPT_TRACE_TAIL_PATHS: f->trace_tail_paths = value; return RT_OK;
    case RT_OPT_CHUNK_REFILL: f->chunk_refill = value ? 1u : 0u; return RT_OK;
    case RT_OPT_FUSED_RAYGEN:
        if (value > 1u) return fail(f->ctx, "rt_set_option: RT_OPT_FUSED_RAYGEN is 0 or 1");
        f->fused_raygen = value;
        return RT_OK;
    case RT_OPT_COMPACT_LOG:
    case RT_OPT_DEBUG_LOG_POOL_DIV:
        if (option == RT_OPT_DEBUG_LOG_POOL_DIV && value == 0) return fail(f->ctx, "rt_set_option: RT_OPT_DEBUG_LOG_POOL_DIV must be >= 1");
        if (option == RT_OPT_COMPACT_LOG && value > 2u) return fail(f->ctx, "rt_set_option: RT_OPT_COMPACT_LOG is 0, 1 or 2");
        return relayout(f, false, false, [&]()
        {
            if (option == RT_OPT_COMPACT_LOG) f->compact_log_opt = value; else f->log_pool_div = value;
            f->log_full_forced = false;
            f->fallback_limit_mb = 0;
            return (int)f->slots;
        });
    case RT_OPT_TRACE_VARIANT:
        if (!(value == 0 || value == 5 || (value >= 8 && value <= 11))) return fail(f->ctx, "rt_set_option: unknown trace kernel variant (0, 5, 8..11)");
        f->trace_variant = value;
        return RT_OK;
    default: return fail(f->ctx, "rt_set_option: unknown option");
    }
}

int rt_set_camera(rt_frame* f, const rt_camera* camera)
{
    if (!f || !camera) return fail(nullptr, "rt_set_camera: NULL argument");
    //  a camera set between rt_generate_rays and rt_advance_sample: the recorded stages belong to the OLD camera -- they run now, with it
    if (f->deferred.active && memcmp(&f->camera, camera, sizeof(rt_camera)) != 0 && deferred_materialize(f) != RT_OK) return RT_ERROR;
    if (f->ahead && memcmp(&f->camera, camera, sizeof(rt_camera)) != 0) ahead_discard(f);              // whatever was traced ahead (and the quiet count) belonged to another view
                                                                                                       // (HIPPathTraceIntegrator sets the SAME camera before every frame: nothing happens)
    f->camera = *camera;
    f->prev_camera = f->camera_last;     // what GenerateAOV sees as prev_camera this frame
    f->camera_last = *camera;
    return RT_OK;
}

int rt_reset(rt_frame* f)                               // CLPathTraceIntegrator::Reset, cl_pt_integrator.cpp:497-508
{
    if (!f) return fail(nullptr, "rt_reset: frame is NULL");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (join_pipes(f) != RT_OK) return RT_ERROR;
    ahead_discard(f);                        // RT_OPT_SAMPLES_AHEAD: the samples traced ahead continued a sum that starts again
    if (!f->denoiser) f->sample_count = 0;   // Reset() keeps the frame index while denoising (:499-504)
    for (PathPipe& q : f->ps)                             // a shadow trace still running on a side stream writes the log
        if (q.stream && (wait_shadow(f, q, 0) != RT_OK || wait_shadow(f, q, 1) != RT_OK)) return RT_ERROR;
    f->stage_chunks = 1;
    f->deferred.active = false; f->deferred.ahead = false;  // a recorded sample that was never advanced: nothing has run
    for (uint32_t i = 0; i < RT_MAX_PIPES; ++i)
    {
        PathPipe& q = f->ps[i];
        q.prev_bounces = 0;
        q.cur_slots = 0;
        q.chunk_base = 0;
        q.chunk_count = 0;
        q.fold_accumulates = 0;
        q.shadow_pending = false;
        if (q.cnt) HIPCHK(ctx, hipMemsetAsync(q.cnt, 0, (size_t)f->log_stride * sizeof(uint32_t), ctx->stream));
        if (q.counters) HIPCHK(ctx, hipMemsetAsync(q.counters, 0, sizeof(DCounters), ctx->stream));
    }
    HIPCHK(ctx, hipMemsetAsync(f->radiance, 0, (size_t)tile_pixels(f) * sizeof(float4), ctx->stream));
    return RT_OK;
}

int rt_frame_reserve_samples(rt_frame* f, uint32_t n_samples, uint32_t* reserved)
{
    FRAME_PROLOGUE(f, "rt_frame_reserve_samples");
    f->reserved_explicitly = true;                       // (rt_integrate then takes the buffers as they are: no lean growth)
    if (ensure_slots(f, n_samples ? n_samples : 1u) != RT_OK) return RT_ERROR;
    if (reserved) *reserved = f->slots;
    return RT_OK;
}

} // extern "C"

// ---- picks: a pixel or a rectangle of the frame's camera, asked of the scene's queries (scene_queries.cpp) through their public entries
// what every pick refuses before it looks at its pixels
static int pick_refused(const rt_frame* f, const char* who)
{
    const std::string name(who);
    if (!f) return fail(nullptr, name + ": frame is NULL");
    if (!f->ctx->scene.valid) return fail(f->ctx, name + ": no scene uploaded");
    if (f->tile.nranks > 1) return fail(f->ctx, name + ": a tile frame (tile_count > 1): pick on a frame of the whole image");
    return RT_OK;
}

extern "C" {

int rt_frame_pick(rt_frame* f, uint32_t x, uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface)
{
    if (pick_refused(f, "rt_frame_pick") != RT_OK) return RT_ERROR;
    rt_ctx* ctx = f->ctx;
    if (x >= f->tile.width || y >= f->tile.height) return fail(ctx, "rt_frame_pick: the pixel is outside the image");
    const rt_ray r = query::pick_ray(f->camera, f->tile.width, f->tile.height, x, y);
    rt_hit h;
    rt_surface s;
    if (rt_scene_trace(ctx, &r, 1u, RT_QUERY_CLOSEST, &h, nullptr, &s) != RT_OK) return RT_ERROR;
    if (ray) *ray = r;
    if (hit) *hit = h;
    if (surface) *surface = s;
    return RT_OK;
}

int rt_frame_pick_all(rt_frame* f, uint32_t x, uint32_t y, uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    if (pick_refused(f, "rt_frame_pick_all") != RT_OK) return RT_ERROR;
    rt_ctx* ctx = f->ctx;
    if (x >= f->tile.width || y >= f->tile.height) return fail(ctx, "rt_frame_pick_all: the pixel is outside the image");
    const rt_ray r = query::pick_ray(f->camera, f->tile.width, f->tile.height, x, y);
    if (rt_scene_trace_all(ctx, &r, 1u, max_hits, out, hits, surfaces) != RT_OK) return RT_ERROR;
    if (ray) *ray = r;
    return RT_OK;
}

int rt_frame_pick_rect(rt_frame* f, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far, rt_region* region, uint32_t* touching,
    uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    if (pick_refused(f, "rt_frame_pick_rect") != RT_OK) return RT_ERROR;
    rt_ctx* ctx = f->ctx;
    if (const char* why = region::rect_refused(f->tile.width, f->tile.height, x0, y0, x1, y1)) return fail(ctx, std::string("rt_frame_pick_rect: ") + why);
    if ((object_touching || object_inside) && !ctx->scene.pose) return fail(ctx, "rt_frame_pick_rect: the per-object outputs need rt_scene_set_objects");
    const rt_region g = region::rect_region(f->camera, f->tile.width, f->tile.height, x0, y0, x1, y1, t_near, t_far);
    if ((touching || inside || object_touching || object_inside) && rt_scene_select(ctx, &g, 1u, touching, inside, object_touching, object_inside) != RT_OK) return RT_ERROR;
    if (region) *region = g;
    return RT_OK;
}

} // extern "C"
