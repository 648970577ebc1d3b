// frame_schedule.cpp -- when a frame's samples run: the stage entries' record-or-run logic (RT_OPT_FRAME_KERNEL's deferred sample and its measuring schedule at
// 255), the wavefront loop over a pipe's bounces, rt_advance_sample, rt_integrate's batch schedule with its compact-log fallback, and the banks of samples
// traced ahead (RT_OPT_SAMPLES_AHEAD).  Host code only, on frame.h and frame_launch.h: every kernel it has run is a function of namespace launch (rt_hip.hip's),
// every buffer it has laid out one of frame_layout.cpp's.  Replaces the device-facing half of the reference's src/integrator/cl_pt_integrator.cpp (Integrate
// and its hooks).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "context.h"         // rt_ctx, fail / HIPCHK
#include "frame.h"           // rt_frame, its pipes, banks and buffer lists
#include "frame_launch.h"    // namespace launch (rt_hip.hip), the layout's functions (frame_layout.cpp)
#include "fold_adapt.h"      // FoldAdapt::state, for the measuring schedule (a frame traced while a fold adaptation is under way is not timed)
using namespace context;
using namespace frame;
using namespace launch;

namespace
{
// The stage API over every pipe that holds a chunk of its sample (RT_OPT_STAGE_PIPES; one pipe is the plain case): `body` is handed each
// of them in turn.
template <class F>
int for_stage_pipes(rt_frame* f, F&& body)
{
    int rc = RT_OK;
    const uint32_t n = f->stage_chunks ? f->stage_chunks : 1u;
    for (uint32_t i = 0; i < n && rc == RT_OK; ++i) rc = body(f->ps[i]);
    return rc;
}

} // namespace

// ... their logs replayed into the radiance (keep: the sample stays open), and the context's stream made to see all of them
int frame::flush_stage(rt_frame* f, bool keep)
{
    if (f->deferred.active && deferred_materialize(f) != RT_OK) return RT_ERROR;    // RT_OPT_FRAME_KERNEL: the recorded stages run after all
    const uint32_t n = f->stage_chunks ? f->stage_chunks : 1u;
    if (for_stage_pipes(f, [&](PathPipe& p) { return keep ? flush_log_keep(f, p) : flush_log(f, p); }) != RT_OK) return RT_ERROR;
    return n > 1 ? join_pipes(f) : RT_OK;
}

// RT_OPT_FRAME_KERNEL = 255 measures again: another workload, or another grid
void frame::fk_auto_restart(rt_frame* f) { f->fk_auto.frames = 0; f->fk_auto.timing = -1; f->fk_auto.decided = false; f->fk_auto.use_kernel = false; }

namespace
{

// RT_OPT_FRAME_KERNEL = 255, at the start of a stage-API sample of the whole tile on one pipe: frames 0 - 3 warm up (two each way), frames 4 - 19 alternate
// stage kernels / k_frame and are timed; once the last timed frame's events have completed, the faster way stays (until the next scene upload)
void fk_auto_begin_frame(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    auto& m = f->fk_auto;
    if (m.scene != ctx->scene_uploads) { m.frames = 0; m.timing = -1; m.decided = false; m.use_kernel = false; m.scene = ctx->scene_uploads; }
    m.timing = -1;
    m.skip = false;
    if (!m.decided)
    {
        const int k = m.frames;
        if (k >= 20 && hipEventQuery(m.ev[15][1]) == hipSuccess)
        {
            m.ms_stage = m.ms_kernel = 0.0f;
            bool ok = true;
            for (int i = 0; i < 16 && ok; ++i)
            {
                float t = 0.0f;
                ok = hipEventElapsedTime(&t, m.ev[i][0], m.ev[i][1]) == hipSuccess;
                ((i & 1) ? m.ms_kernel : m.ms_stage) += t;
            }
            if (!ok) (void)hipGetLastError();
            m.decided = true;
            m.use_kernel = ok && m.ms_kernel < m.ms_stage;
        }
        else if (k >= 4 && k < 20 && ctx->scene.adapt && (ctx->scene.adapt->state == FoldAdapt::ARMED || ctx->scene.adapt->state == FoldAdapt::PROBING || ctx->scene.adapt->state == FoldAdapt::COMPUTING))
        {
            //  a fold adaptation is under way -- probe launches on this stream, a fold swapped mid-window: such a frame is not one
            // of the sixteen that are compared (it runs through the stage kernels, untimed; the schedule goes on once the folds have settled)
            m.skip = true;
        }
        else if (k >= 4 && k < 20)
        {
            m.timing = k - 4;
            bool ok = true;
            for (hipEvent_t& e : m.ev[m.timing]) if (!e) ok = ok && hipEventCreate(&e) == hipSuccess;
            if (!ok || hipEventRecord(m.ev[m.timing][0], ctx->stream) != hipSuccess) { (void)hipGetLastError(); m.decided = true; m.use_kernel = false; m.timing = -1; }
        }
        if (!m.decided && !m.skip) ++m.frames;
    }
    if (m.decided) m.frames = 1 << 20;          // (frame_kernel_eligible reads `decided`; keep frames - 1 out of the schedule's range)
}

// ... and at its end: the closing event of a frame that is being timed
void fk_auto_end_frame(rt_frame* f)
{
    if (f->fk_auto.timing < 0) return;
    (void)hipEventRecord(f->fk_auto.ev[f->fk_auto.timing][1], f->ctx->stream);
    f->fk_auto.timing = -1;
}
} // namespace

// The wavefront loop of the rays in pipe p's queue (rt_integrate's chunks, the batches traced ahead): closest-hit trace, then per bounce
// k_shade, shadow trace, next closest-hit trace.  The shadow trace of bounce b and the closest-hit trace of bounce b + 1 both depend on k_shade(b)
// only, and k_shade(b + 1) on the latter only (the shadow queue is double-buffered): with overlap_shadow the shadow trace goes to the pipe's side
// stream, AFTER the next closest-hit launch has been enqueued -- it moves in as that launch's last rays drain and leaves as k_shade(b + 1) moves
// in, so neither tail idles the machine (tools/launch_timeline.py: 0.75-0.95 ms each).  per_frame: the AOVs of the first hits (ComputeAOVs).
static int trace_bounces(rt_frame* f, PathPipe& p, bool per_frame)
{
    if (intersect_pipe(f, p, 0) != RT_OK) return RT_ERROR;
    for (uint32_t bounce = 0; bounce <= f->max_bounces; ++bounce)
    {
        const bool more = bounce < f->max_bounces;
        if (bounce == 0 && per_frame && rt_compute_aovs(f) != RT_OK) return RT_ERROR;
        if (shade_pipe(f, p, bounce, true) != RT_OK) return RT_ERROR;
        if (f->side_active && more && intersect_pipe(f, p, bounce + 1u) != RT_OK) return RT_ERROR;
        if (shadow_pipe(f, p, bounce) != RT_OK) return RT_ERROR;
        if (!f->side_active && more && intersect_pipe(f, p, bounce + 1u) != RT_OK) return RT_ERROR;
    }
    return RT_OK;
}

// ---- RT_OPT_SAMPLES_AHEAD: samples traced ahead of the caller's Integrate() calls -------------------------------------------------------
// The reference's own pattern is one Integrate() per frame at one sample per pixel (src/render.cpp:197); while the camera stands still -- its
// progressive accumulation -- sample s + 1 .. s + k are known the moment sample s is: same camera, consecutive sample indices.  A launch of one
// sample per pixel is its own tail (3.3 ms per 1080p frame where the work is worth 1.6), a launch of k samples is not.  So,
// once `RT_AHEAD_QUIET` samples have been advanced without a reset, the frame traces BATCHES of the next samples into two banks (frames of its
// own: same tile, same options, the rt_integrate schedule without its replay) on streams beside the context's, 2, 4, 8 .. `depth` samples at a time,
// and a later rt_advance_sample whose sample sits in a bank only REPLAYS that sample's slot of the bank's radiance log into the radiance
// (k_flush, first_slot) -- the sum after every Integrate() is the reference's bit for bit, sample by sample, in sample order.  One bank is
// consumed while the other computes; the moment a bank is empty its next batch is enqueued, so the device always has one batch running and one
// queued.  A reset, another camera, another option, a scene upload, rt_integrate or anything that looks between two stages DISCARDS what was
// traced ahead (its launches finish on their own streams, unobserved): the price of a camera that starts to move is at most 2 x depth samples
// of device time, once; a camera that moves every frame never leaves the quiet phase and pays nothing.
#define RT_AHEAD_QUIET 3u

static bool ahead_bank_idle(const AheadBank& b) { return b.next >= b.n; }

// the bank that holds sample `s` as its next slot, or -1
static int ahead_holds(const rt_frame* f, uint32_t s)
{
    if (!f->ahead || !f->ahead_opt) return -1;
    const Ahead& A = *f->ahead;
    if (A.scene != f->ctx->scene_uploads || memcmp(&A.camera, &f->camera, sizeof(rt_camera)) != 0) return -1;
    for (int i = 0; i < 2; ++i)
        if (A.bank[i].h && !ahead_bank_idle(A.bank[i]) && A.bank[i].base + A.bank[i].next == s) return i;
    return -1;
}

// Samples per batch: the caller's (2 .. 64), or -- 1 = automatic -- what makes a batch ~32 M paths: 16 samples of a 1080p frame, 4 of a 4K one
// (rt_integrate at 2 / 4 / 8 / 16 samples of the 1080p headline frame in flight: 2.67 / 2.26 / 1.97 / 1.80 ms per sample where one alone costs 3.3 and
// 128 together 1.56; the 4K / 16-bounce config: 22.7 / 19.4 / 17.9 ms at 1 / 2 / 4 -- profiles/r06_call01.log), within 64 GiB of path state for the two banks.
uint32_t frame::ahead_depth(const rt_frame* f)
{
    const uint64_t n = tile_pixels(f);
    uint64_t k = f->ahead_opt & 0xFFu;
    if (k == 0) return 0;
    if (k == 1 || k == 255) { k = (32000000ull + n - 1) / n; if (k > 64) k = 64; }
    const uint64_t budget = f->state_limit_mb ? ((uint64_t)f->state_limit_mb << 20) : (64ull << 30);
    const uint64_t per_sample = 2ull * n * full_bytes_per_path(f->max_bounces);
    if (k * per_sample > budget) k = budget / per_sample;
    return k >= 2 ? (uint32_t)k : 0u;
}

// Is the stage API's next sample one this mode may serve?  (One sample of the whole tile in one chunk on the context's stream, nothing that reads
// between the stages.)
bool frame::ahead_wanted(const rt_frame* f)
{
    return f->ahead_opt != 0u && !f->ahead_owner && f->n_local != 0u && !(f->denoiser || f->aov != 0) && !f->profile && !f->timeline &&
           f->stage_pipes <= 1u && f->pipelines == 1u && f->ctx->scene.valid && ahead_depth(f) >= 2u;
}

// ---- what a bank follows ---------------------------------------------------------------------------------------------------------------
// Every RT_OPT_* is in one of three classes.  A new option goes into the table, into ahead_wanted, or into the last list with its reason.
//  * FOLLOWED BY THE BANKS (they decide what a batch computes or how it is launched): the twelve rows of RT_AHEAD_FOLLOWED, and as the named exception
//    RT_OPT_SMALL_LAUNCH_PATHS and RT_OPT_TRACE_TAIL_PATHS (64-bit fields, one with a "set" flag: copied by ahead_configure, compared by ahead_key).
//  * RULES THE MODE OUT (ahead_wanted): RT_OPT_AOV, RT_OPT_DENOISER (read between stages), RT_OPT_PROFILE_KERNELS (events per launch),
//    RT_OPT_PIPELINES, RT_OPT_STAGE_PIPES (one chunk on one stream).
//  * DOES NOT CONCERN A BANK: RT_OPT_SAMPLES_AHEAD (the mode itself: its depth and stream bit are in the key), RT_OPT_PATH_STATE_LIMIT_MB (bounds the depth:
//    in the key), RT_OPT_SAMPLES_IN_FLIGHT (a bank holds `depth` samples), RT_OPT_COMPACT_LOG, RT_OPT_DEBUG_LOG_POOL_DIV (a bank has no limit: full layout),
//    RT_OPT_FRAME_KERNEL (banks trace batches), RT_OPT_DEBUG_ALLOC_LIMIT (the owner's test hook), RT_OPT_TRACE_PACKET_BOUNCES (accepts only 0),
//    RT_OPT_FUSED_RAYGEN (rt_integrate's batches only: a bank's batch writes its primary queue, ahead_launch).
static const struct { int option; uint32_t rt_frame::*field; } RT_AHEAD_FOLLOWED[12] = {
    {RT_OPT_MAX_BOUNCES, &rt_frame::max_bounces}, {RT_OPT_SAMPLER, &rt_frame::sampler}, {RT_OPT_WHITE_FURNACE, &rt_frame::white_furnace},
    {RT_OPT_TRACE_DROP_LAST_BOUNCE_RAYS, &rt_frame::drop_last}, {RT_OPT_OVERLAP_SHADOW, &rt_frame::overlap_shadow}, {RT_OPT_TRACE_VARIANT, &rt_frame::trace_variant},
    {RT_OPT_TRACE_TUNE, &rt_frame::trace_tune}, {RT_OPT_SHADE_PARTITION, &rt_frame::shade_partition}, {RT_OPT_TRACE_TAIL_LANES, &rt_frame::trace_tail_lanes},
    {RT_OPT_CHUNK_REFILL, &rt_frame::chunk_refill}, {RT_OPT_TRACE_WAVES_PER_CU, &rt_frame::trace_waves_per_cu}, {RT_OPT_TRACE_SELECT_FORM_BOX, &rt_frame::select_form_box}};

static AheadKey ahead_key(const rt_frame* f)
{
    AheadKey k;
    for (int i = 0; i < 12; ++i) k.followed[i] = f->*RT_AHEAD_FOLLOWED[i].field;
    k.small_launch = f->small_launch_set ? (uint32_t)std::min<uint64_t>(f->small_launch_paths, 0xFFFFFFFFull) : 0xFFFFFFFFu;
    k.tail_paths = (uint32_t)std::min<uint64_t>(f->trace_tail_paths, 0xFFFFFFFFull);
    k.depth = ahead_depth(f);
    k.two_streams = f->ahead_opt & 0x100u;
    return k;
}

// The banks exist, are laid out for `depth` samples in flight and have the owner's options.  (Anything here may wait for the device: it runs when
// the mode starts and after an option has changed, never between two frames of a quiet camera.)
static int ahead_configure(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    if (!f->ahead) f->ahead = new Ahead();
    Ahead& A = *f->ahead;
    const AheadKey want = ahead_key(f);
    if (A.configured && memcmp(&want, &A.mirrored, sizeof(want)) == 0) return RT_OK;
    ahead_discard(f);
    A.configured = false;
    const bool two_streams = want.two_streams != 0u;
    for (int i = 0; i < 2; ++i)
    {
        // the banks' launches go beside the frame's own: one stream for both banks (their batches in order) or one each (they overlap)
        if (!A.stream[i] && (i == 0 || two_streams)) HIPCHK(ctx, hipStreamCreateWithFlags(&A.stream[i], hipStreamNonBlocking));
        AheadBank& b = A.bank[i];
        hipStream_t const st = two_streams ? A.stream[i] : A.stream[0];
        if (b.h && b.h->ps[0].stream != st) { (void)rt_frame_destroy(b.h); b.h = nullptr; }
        if (!b.h)
        {
            rt_frame_desc fd = {f->tile.width, f->tile.height, f->tile.rank, f->tile.nranks, f->tile.band_h};
            if (create_frame(ctx, &fd, &b.h, st) != RT_OK) { b.h = nullptr; return RT_ERROR; }
            b.h->ahead_owner = f;
        }
        if (!b.done) HIPCHK(ctx, hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
        if (!b.order) HIPCHK(ctx, hipEventCreateWithFlags(&b.order, hipEventDisableTiming));
        if (sync_frame_streams(b.h) != RT_OK) return RT_ERROR;
        rt_frame* h = b.h;
        for (const auto& row : RT_AHEAD_FOLLOWED)
            if (rt_set_option(h, row.option, f->*row.field) != RT_OK) return RT_ERROR;
        h->trace_tail_paths = f->trace_tail_paths;
        h->small_launch_paths = f->small_launch_paths; h->small_launch_set = f->small_launch_set;
        if (ensure_slots(h, want.depth) != RT_OK) return RT_ERROR;
        if (h->slots < 2u || h->chunk_pixels < tile_pixels(f)) return fail(ctx, "RT_OPT_SAMPLES_AHEAD: a bank could not be laid out for the whole tile");
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // the banks' allocations were cleared on the context's stream
    A.depth = std::min(want.depth, std::min(A.bank[0].h->slots, A.bank[1].h->slots));
    A.mirrored = want;
    A.configured = true;
    return RT_OK;
}

// A batch: samples base .. base + n - 1 through the wavefront loop of bank i, as rt_integrate runs one (trace_bounces), but the
// log is left as it is: its replay happens sample by sample, by ahead_consume.
static int ahead_launch(rt_frame* f, int i, uint32_t base, uint32_t n)
{
    rt_ctx* ctx = f->ctx;
    Ahead& A = *f->ahead;
    AheadBank& b = A.bank[i];
    rt_frame* h = b.h;
    hipStream_t const st = h->ps[0].stream;
    h->camera = f->camera;
    h->sample_count = base;
    // behind whatever the owner's stream holds: the last replay out of this bank's log
    HIPCHK(ctx, hipEventRecord(b.order, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(st, b.order, 0));
    PathPipe& p = h->ps[0];
    h->side_active = side_on(h);
    int rc = generate_rays(h, p, n, 0, false);
    if (rc == RT_OK) rc = trace_bounces(h, p, false);
    if (rc == RT_OK && (wait_shadow(h, p, 0) != RT_OK || wait_shadow(h, p, 1) != RT_OK)) rc = RT_ERROR;
    if (rc == RT_OK && hipEventRecord(b.done, st) != hipSuccess) rc = fail(ctx, "RT_OPT_SAMPLES_AHEAD: recording a batch's end failed");
    if (rc != RT_OK)
    {
        // nothing of a batch that could not be enqueued is ever replayed
        (void)hipGetLastError();
        (void)sync_frame_streams(h);
        (void)hipMemsetAsync(p.cnt, 0, (size_t)h->log_stride * sizeof(uint32_t), st);
        p.cur_slots = 0; p.shadow_pending = false; p.shadow_in_flight[0] = p.shadow_in_flight[1] = false;
        b.n = b.next = 0;
        return RT_ERROR;
    }
    b.base = base; b.n = n; b.next = 0;
    A.camera = f->camera;
    A.scene = ctx->scene_uploads;
    A.last_n = n;
    A.launched += n;
    return RT_OK;
}

// rt_advance_sample for a sample that sits in bank i: its slot of the bank's log, replayed into the radiance on the context's stream
static int ahead_consume(rt_frame* f, int i)
{
    rt_ctx* ctx = f->ctx;
    AheadBank& b = f->ahead->bank[i];
    rt_frame* h = b.h;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, b.done, 0));
    if (replay_bank_slot(f, h, b.next) != RT_OK) return RT_ERROR;
    ++b.next;
    ++f->sample_count;
    ++f->ahead->consumed;
    if (ahead_bank_idle(b)) h->ps[0].cur_slots = 0;       // every slot replayed (k_flush has set their counts back to zero)
    return RT_OK;
}

// Every idle bank gets the next batch -- the samples behind the last one traced ahead -- as long as some bank holds the next sample (otherwise the
// mode is starting: `first` = the sample to begin with).  A failure to launch only ends the speculation: the samples are traced when they are asked for.
static void ahead_schedule(rt_frame* f, bool starting)
{
    if (!ahead_wanted(f)) return;
    if (ahead_configure(f) != RT_OK) { (void)hipGetLastError(); f->ahead_opt = 0; return; }   // (e.g. no memory for the banks: the mode switches itself off)
    Ahead& A = *f->ahead;
    if (A.depth < 2u) return;
    const uint32_t s = f->sample_count;
    if (!starting && ahead_holds(f, s) < 0 && !(ahead_bank_idle(A.bank[0]) && ahead_bank_idle(A.bank[1]))) return;
    for (int i = 0; i < 2; ++i)
    {
        if (!ahead_bank_idle(A.bank[i])) continue;
        uint32_t end = s;
        for (const AheadBank& o : A.bank) if (!ahead_bank_idle(o)) end = std::max(end, o.base + o.n);
        const uint32_t n = ahead_bank_idle(A.bank[i ^ 1]) ? 2u : std::min(A.depth, 2u * std::max(1u, A.last_n));
        if (end > 0xFFFFFFFFu - n) return;
        if (ahead_launch(f, i, end, n) != RT_OK) { (void)hipGetLastError(); return; }
        if (starting) return;                               // the first batch alone: the ramp's next step follows at its first replay
    }
}

void frame::ahead_discard(rt_frame* f)
{
    if (!f || !f->ahead) return;
    Ahead& A = *f->ahead;
    A.quiet = 0;
    A.last_n = 0;
    for (AheadBank& b : A.bank)
    {
        if (!b.h) continue;
        rt_frame* h = b.h;
        hipStream_t const st = h->ps[0].stream;
        if (!ahead_bank_idle(b) || h->ps[0].cur_slots != 0)
        {
            // behind the owner's last replay out of this log AND behind the batch itself (same stream): the slots nobody replayed go back to zero, and so
            // do the bank's ray counters (rt_frame_get_stats adds them to the owner's)
            (void)hipEventRecord(b.order, f->ctx->stream);
            (void)hipStreamWaitEvent(st, b.order, 0);
            (void)hipMemsetAsync(h->ps[0].cnt, 0, (size_t)h->log_stride * sizeof(uint32_t), st);
            A.discarded += b.n - b.next;
        }
        if (h->ps[0].counters) (void)hipMemsetAsync(h->ps[0].counters, 0, sizeof(DCounters), st);
        h->ps[0].cur_slots = 0; h->ps[0].shadow_pending = false; h->ps[0].prev_bounces = 0; h->ps[0].fold_accumulates = 0;
        b.n = b.next = 0;
    }
}

void frame::ahead_destroy(rt_frame* f)
{
    if (!f || !f->ahead) return;
    Ahead* A = f->ahead;
    f->ahead = nullptr;
    for (AheadBank& b : A->bank)
    {
        if (b.h) (void)rt_frame_destroy(b.h);             // (waits for its streams)
        if (b.done) (void)hipEventDestroy(b.done);
        if (b.order) (void)hipEventDestroy(b.order);
    }
    for (hipStream_t st : A->stream) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    delete A;
}

// A sample the frame traced itself has been advanced: RT_AHEAD_QUIET of them in a row (no reset between) start the mode -- a first batch of two.
static void ahead_after_plain_sample(rt_frame* f)
{
    if (!f->ahead_opt || !ahead_wanted(f)) return;
    if (!f->ahead) f->ahead = new Ahead();
    Ahead& A = *f->ahead;
    if (++A.quiet < RT_AHEAD_QUIET) return;
    if (ahead_bank_idle(A.bank[0]) && ahead_bank_idle(A.bank[1])) ahead_schedule(f, true);
}

// The recorded stages of a deferred sample, run with the stage kernels after all (somebody wants the state between two stages).
int frame::deferred_materialize(rt_frame* f)
{
    if (!f->deferred.active) return RT_OK;
    const uint32_t done = f->deferred.bounce;
    const int next = f->deferred.next;
    f->deferred.active = false;
    // RT_OPT_SAMPLES_AHEAD: somebody looks between the stages of a sample that sits in a bank -- the frame traces it itself after all, and what
    // was traced ahead (that sample's slot first of all) is dropped
    if (f->deferred.ahead) { f->deferred.ahead = false; ahead_discard(f); }
    if (generate_rays(f, f->ps[0], 1) != RT_OK) return RT_ERROR;
    for (uint32_t b = 0; b <= done; ++b)
    {
        const int upto = b < done ? 3 : next;                            // stages of bounce b that were recorded
        if (upto >= 1 && rt_intersect(f, b) != RT_OK) return RT_ERROR;
        if (upto >= 2 && rt_shade(f, b) != RT_OK) return RT_ERROR;
        if (upto >= 3 && rt_intersect_shadow(f, b) != RT_OK) return RT_ERROR;
    }
    return RT_OK;
}

// ---- stages ----------------------------------------------------------------
extern "C" {

int rt_generate_rays(rt_frame* f)                       // GenerateRays, :516-520
{
    FRAME_PROLOGUE(f, "rt_generate_rays");
    // the reference's own pattern (one Integrate() per frame through the hooks) adapts its folds too: probe, worker and adoption ride on
    // the frames' first stage (rt_integrate calls the same hook)
    if (fold_adapt_hook(f) != RT_OK) return RT_ERROR;
    // The stages run on the FULL log layout.  A compact log's pool can run dry (k_shade raises DCounters::log_ovf_flag); rt_integrate then repeats the batch in the
    // full layout, but here the caller drives the stages and there is nothing to repeat -- the sample's later entries would simply be missing from the sum (fuzz seed
    // 5652 of a 10 000-seed campaign, round 6: RT_OPT_COMPACT_LOG + a test-sized pool + the stage API, 20 pixels short).  One reallocation, the first time a frame
    // whose buffers are compact is driven through the stages.
    if (f->log_ovf_blocks != 0u)
    {
        if (f->ps[0].cur_slots != 0 || f->deferred.active) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
        if (flush_log(f, f->ps[0]) != RT_OK || join_pipes(f) != RT_OK) return RT_ERROR;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        f->log_full_forced = true;
        if (alloc_path_buffers(f, f->slots ? f->slots : 1u) != RT_OK) return RT_ERROR;
    }
    const uint32_t n_local = tile_pixels(f);
    uint32_t np = 1, cp = 0;
    chunk_plan(f, 1, np, cp);
    if ((uint64_t)cp * np < n_local)
        return fail(ctx, "rt_generate_rays: RT_OPT_PATH_STATE_LIMIT_MB is too small for one sample of the whole tile "
                         "(the stage API keeps every chunk on a pipe of its own; use rt_integrate)");
    if (f->deferred.active) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
    if (np <= 1)
    {
        f->stage_chunks = 1;
        if (ensure_whole_tile(f) != RT_OK) return RT_ERROR;
        if (f->ahead && ahead_wanted(f) && ahead_holds(f, f->sample_count) >= 0)
        {
            // RT_OPT_SAMPLES_AHEAD: this sample has been traced ahead -- nothing is launched, the stages are recorded, rt_advance_sample replays its log
            if (f->ps[0].cur_slots != 0) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
            f->deferred.active = true; f->deferred.bounce = 0; f->deferred.next = 0; f->deferred.ahead = true;
            return RT_OK;
        }
        if (f->frame_kernel == 255u) fk_auto_begin_frame(f);
        if (frame_kernel_eligible(f))
        {
            // RT_OPT_FRAME_KERNEL: nothing is launched yet -- the stages are recorded, rt_advance_sample launches k_frame
            if (f->ps[0].cur_slots != 0) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
            if (ensure_slots(f, 1) != RT_OK) return RT_ERROR;
            if (frame_kernel_eligible(f)) { f->deferred.active = true; f->deferred.bounce = 0; f->deferred.next = 0; f->deferred.ahead = false; return RT_OK; }
        }
        return generate_rays(f, f->ps[0], 1);
    }
    // RT_OPT_STAGE_PIPES: the sample's chunks travel side by side, one per pipe; an allocation made for a larger batch (one pipe, the
    // whole tile) gives way to the one-sample layout
    if (f->chunk_pixels != cp || f->n_pipes != np)
    {
        for (const PathPipe& q : f->ps) if (q.cur_slots != 0) return fail(ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
        if (flush_log(f, f->ps[0]) != RT_OK || join_pipes(f) != RT_OK) return RT_ERROR;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (alloc_path_buffers(f, 1) != RT_OK) return RT_ERROR;
        if (f->chunk_pixels != cp || f->n_pipes != np) return fail(ctx, "rt_generate_rays: the one-sample layout did not come out as planned");
    }
    if (fork_pipes(f) != RT_OK) return RT_ERROR;         // the pipes' streams see what the context's stream has been given (reset, the last resolve)
    const uint32_t n_chunks = (n_local + f->chunk_pixels - 1u) / f->chunk_pixels;
    f->stage_chunks = n_chunks;
    uint32_t c = 0;
    return for_stage_pipes(f, [&](PathPipe& p) { return generate_rays(f, p, 1, (c++) * f->chunk_pixels, false); });
}

int rt_intersect(rt_frame* f, uint32_t bounce)          // IntersectRays, :522-539
{
    FRAME_PROLOGUE(f, "rt_intersect");
    if (bounce > RT_MAX_BOUNCES_LIMIT) return fail(ctx, "rt_intersect: bounce out of range");
    if (f->deferred.active)
    {
        if (f->deferred.next == 0 && bounce == f->deferred.bounce) { f->deferred.next = 1; return RT_OK; }
        if (deferred_materialize(f) != RT_OK) return RT_ERROR;
    }
    return for_stage_pipes(f, [&](PathPipe& p) { return intersect_pipe(f, p, bounce); });
}

int rt_shade_miss(rt_frame* f, uint32_t) { return f ? RT_OK : fail(nullptr, "rt_shade_miss: frame is NULL"); }
int rt_clear_outgoing_counter(rt_frame* f, uint32_t) { return f ? RT_OK : fail(nullptr, "rt_clear_outgoing_counter: frame is NULL"); }
int rt_clear_shadow_counter(rt_frame* f) { return f ? RT_OK : fail(nullptr, "rt_clear_shadow_counter: frame is NULL"); }
int rt_accumulate_direct(rt_frame* f) { return f ? RT_OK : fail(nullptr, "rt_accumulate_direct: frame is NULL"); }

int rt_shade(rt_frame* f, uint32_t bounce)              // ShadeMissedRays + ShadeSurfaceHits, :582-643
{
    FRAME_PROLOGUE(f, "rt_shade");
    if (bounce > RT_MAX_BOUNCES_LIMIT) return fail(ctx, "rt_shade: bounce out of range");
    if (2u * (bounce + 1u) > f->log_entries) return fail(ctx, "rt_shade: bounce beyond the configured max_bounces");
    if (f->deferred.active)
    {
        if (f->deferred.next == 1 && bounce == f->deferred.bounce) { f->deferred.next = 2; return RT_OK; }
        if (deferred_materialize(f) != RT_OK) return RT_ERROR;
    }
    return for_stage_pipes(f, [&](PathPipe& p) { return shade_pipe(f, p, bounce, false); });
}

int rt_intersect_shadow(rt_frame* f, uint32_t bounce)   // IntersectShadowRays + AccumulateDirectSamples, :564-580,645-649
{
    FRAME_PROLOGUE(f, "rt_intersect_shadow");
    if (bounce > RT_MAX_BOUNCES_LIMIT) return fail(ctx, "rt_intersect_shadow: bounce out of range");
    if (f->deferred.active)
    {
        if (f->deferred.next == 2 && bounce == f->deferred.bounce) { f->deferred.next = 0; ++f->deferred.bounce; return RT_OK; }
        if (deferred_materialize(f) != RT_OK) return RT_ERROR;
    }
    return for_stage_pipes(f, [&](PathPipe& p) { return shadow_pipe(f, p, bounce); });
}

int rt_advance_sample(rt_frame* f)                      // AdvanceSampleCount, :510-514
{
    if (!f) return fail(nullptr, "rt_advance_sample: frame is NULL");
    (void)hipSetDevice(f->ctx->device);
    if (f->deferred.active)
    {
        const bool whole = f->deferred.next == 0 && f->deferred.bounce == f->max_bounces + 1u;
        if (f->deferred.ahead)
        {
            // RT_OPT_SAMPLES_AHEAD: the sample was traced ahead; its recorded stages are dropped and its log slot is replayed
            const int bank = whole ? ahead_holds(f, f->sample_count) : -1;
            if (bank >= 0)
            {
                f->deferred.active = false; f->deferred.ahead = false;
                if (ahead_consume(f, bank) != RT_OK) return RT_ERROR;
                ++f->ahead->quiet;
                ahead_schedule(f, false);
                return RT_OK;
            }
        }
        // the whole sample was recorded in the canonical order: ONE launch (k_frame replays its own pixels' log, too)
        else if (whole && frame_kernel_eligible(f))
        {
            if (launch_frame_kernel(f) != RT_OK)
            {
                //  the recorded sample is not lost: it runs through the stage kernels, and this frame stops asking for k_frame
                (void)hipGetLastError();
                f->frame_kernel = 0u;
                f->fk_auto.decided = true; f->fk_auto.use_kernel = false; f->fk_auto.timing = -1;
                if (deferred_materialize(f) != RT_OK || flush_stage(f) != RT_OK) return RT_ERROR;
                f->sample_count += 1;
                ahead_after_plain_sample(f);
                return RT_OK;
            }
            f->deferred.active = false;
            f->sample_count += 1;
            fk_auto_end_frame(f);
            ahead_after_plain_sample(f);
            return RT_OK;
        }
        if (deferred_materialize(f) != RT_OK) return RT_ERROR;
    }
    uint32_t n = f->ps[0].cur_slots ? f->ps[0].cur_slots : 1u;
    if (flush_stage(f) != RT_OK) return RT_ERROR;        // radiance_buffer_ += this sample's contributions (of every chunk: RT_OPT_STAGE_PIPES)
    f->sample_count += n;
    fk_auto_end_frame(f);                                // RT_OPT_FRAME_KERNEL = 255
    ahead_after_plain_sample(f);
    return RT_OK;
}

int rt_integrate(rt_frame* f, uint32_t n_samples)       // n x Integrator::Integrate(), integrator.cpp:27-59
{
    FRAME_PROLOGUE(f, "rt_integrate");
    if (f->deferred.active) return fail(ctx, "rt_integrate: a sample of the stage API is in flight (rt_advance_sample first)");
    if (f->stage_chunks > 1)
    {
        for (const PathPipe& q : f->ps) if (q.cur_slots != 0) return fail(ctx, "rt_integrate: a sample of the stage API is in flight (rt_advance_sample first)");
        f->stage_chunks = 1;
    }
    ahead_discard(f);                                   // RT_OPT_SAMPLES_AHEAD serves the stage API; these samples are traced here
    if (fold_adapt_hook(f) != RT_OK) return RT_ERROR;
    // `slots` samples travel through the wavefront together (more rays per launch ->
    // fuller machine, shorter relative tails); the radiance log keeps the sum exact.
    uint32_t done = 0;
    const bool per_frame = f->denoiser || f->aov != 0;  // interactive features: one sample per Integrate()
    uint32_t cap = per_frame ? 1u : slot_cap(f);
    uint32_t want = n_samples < cap ? n_samples : cap;
    // Lean growth (round 6).  Mapping the per-path buffers is not free: a hipMalloc of the 102 GB that 128 samples of a 1080p frame in flight take costs 2.4 - 3.5 s on
    // an MI355X box (bench.py: config.path_state_alloc_s, cold_job.alloc_s) -- six times what BASELINE's whole 256-spp job renders in.  So a job that has to GROW the buffers,
    // was not told how many samples to keep in flight (RT_OPT_SAMPLES_IN_FLIGHT = 0) and did not reserve them (rt_frame_reserve_samples) grows them with what it has been asked
    // for so far: an eighth of the samples requested since the frame was made (at least 16), never below what 8 GiB hold -- 256 spp at 1080p: 32 in flight, 27 GB, ~5 % below the
    // full batch's rate; a job that keeps asking reaches the full batch by doubling.
    f->samples_asked += n_samples;
    if (!per_frame && f->slots_opt == 0u && !f->reserved_explicitly && want > f->slots)
    {
        const uint64_t per_slot = (uint64_t)bytes_per_path(f, want) * tile_pixels(f);
        const uint64_t lean = std::max<uint64_t>(16u, (f->samples_asked + 7u) / 8u), floor_slots = (8ull << 30) / (per_slot ? per_slot : 1u);
        const uint64_t grown = std::max<uint64_t>(std::max(lean, floor_slots), f->slots);
        if (grown < want) want = (uint32_t)grown;
    }
    if (ensure_slots(f, want) != RT_OK) return RT_ERROR;
    // ensure_slots may have halved the batch to fit the device (slots_limit): never ask for more than it got
    if (!per_frame) cap = slot_cap(f) < f->slots ? slot_cap(f) : f->slots;
    if (cap == 0) cap = 1;
    if (per_frame && chunk_for(f, 1) >= tile_pixels(f) && ensure_whole_tile(f) != RT_OK) return RT_ERROR;
    if (per_frame && f->chunk_pixels < tile_pixels(f))
        return fail(ctx, "rt_integrate: AOVs / the denoiser need the whole tile in one chunk (raise RT_OPT_PATH_STATE_LIMIT_MB)");
    if (fork_pipes(f) != RT_OK) return RT_ERROR;
    int rc = RT_OK;
    f->side_active = side_on(f);
    while (done < n_samples && rc == RT_OK)
    {
        // batches of (nearly) equal size: 1024 samples with room for 160 in flight go as 7 x 146-147, not 6 x 160 + 64 --
        // every launch costs its tail whatever its size (DESIGN.md "Where a launch's time goes")
        const uint32_t left = n_samples - done, n_batches = (left + cap - 1u) / cap;
        uint32_t batch = (left + n_batches - 1u) / n_batches;
        if (per_frame) batch = 1;
        if (f->denoiser && rt_reset(f) != RT_OK) { rc = RT_ERROR; break; }   // integrator.cpp:29: Reset() every frame
        // The whole wavefront loop per chunk of pixels; chunk c runs on pipe c % n_pipes (its own stream), so the
        // chunks' launches overlap each other's tails.  A chunk always lands on the same pipe: its log replays
        // (k_flush) stay in sample order.
        uint32_t c = 0;
        for (uint32_t base = 0; base < tile_pixels(f) && rc == RT_OK; ++c)
        {
            PathPipe& p = f->ps[c % f->n_pipes];
            if (generate_rays(f, p, batch, base, c >= f->n_pipes, !per_frame && primary_fusable(f)) != RT_OK) { rc = RT_ERROR; break; }
            rc = trace_bounces(f, p, per_frame);
            // Compact log layout: did this sequence run the overflow pool dry?  (The one host synchronisation of a batch; the
            // full layout has none.)  If so nothing of it has reached the radiance yet: drop it, switch the frame to the full
            // layout within the same memory, and run the SAME chunk again -- the sum stays exact.
            if (rc == RT_OK && f->log_ovf_blocks != 0u)
            {
                uint32_t dry = 0;
                if (wait_shadow(f, p, 0) != RT_OK || wait_shadow(f, p, 1) != RT_OK) { rc = RT_ERROR; break; }
                if (hipMemcpyAsync(&dry, &p.counters->log_ovf_flag, sizeof(dry), hipMemcpyDeviceToHost, p.stream) != hipSuccess ||
                    hipStreamSynchronize(p.stream) != hipSuccess)
                {
                    rc = fail(ctx, "rt_integrate: reading the log-pool flag failed");
                    break;
                }
                if (dry)
                {
                    if (hipMemsetAsync(p.counters->queue, 0, sizeof(p.counters->queue) + sizeof(p.counters->shadow), p.stream) != hipSuccess ||
                        hipMemsetAsync(&p.counters->log_ovf_flag, 0, sizeof(uint32_t), p.stream) != hipSuccess ||
                        hipStreamSynchronize(p.stream) != hipSuccess)
                    {
                        rc = fail(ctx, "rt_integrate: discarding a batch failed");
                        break;
                    }
                    p.cur_slots = 0;
                    p.shadow_pending = false;
                    f->log_full_forced = true;
                    // the full layout takes more bytes per path: it may use what the library would have given it in the first
                    // place (half of the HBM), and beyond that runs the same batch size in more chunks
                    f->fallback_limit_mb = 144u << 10;
                    ++f->log_fallbacks;
                    if (alloc_path_buffers(f, f->slots) != RT_OK) { rc = RT_ERROR; break; }     // cnt starts from zero again
                    continue;                                                                   // the same `base`, the new chunk size
                }
            }
            if (rc == RT_OK && flush_log(f, p) != RT_OK) rc = RT_ERROR;       // radiance_buffer_ += this chunk's contributions
            base += f->chunk_pixels;
        }
        if (rc != RT_OK) break;
        f->sample_count += batch;                                            // AdvanceSampleCount, :510-514
        if (f->denoiser && (join_pipes(f) != RT_OK || rt_denoise(f) != RT_OK || rt_copy_history(f) != RT_OK)) rc = RT_ERROR;
        done += batch;
    }
    if (rc != RT_OK)
        for (PathPipe& q : f->ps)                        // a failed batch leaves no shadow trace running behind the caller's back
        {
            if (q.side) (void)hipStreamSynchronize(q.side);
            q.shadow_in_flight[0] = q.shadow_in_flight[1] = false;
        }
    if (join_pipes(f) != RT_OK) return RT_ERROR;         // whatever follows on the context's stream sees every chunk
    return rc;
}

} // extern "C"
