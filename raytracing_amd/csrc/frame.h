// frame.h -- what a frame is, for the translation units that implement entry points on it: the record behind the C-ABI's opaque rt_frame with its pipes, its
// banks of samples traced ahead and its buffer lists, and the few functions of the frames' units that a filter, a reader or the context calls before it touches
// a frame's memory.  Internal like context.h: never installed, never included by include/, plain C++ (no device code: the records a frame hands to its
// launches are device_scene.h's).  Who owns what: frame_layout.cpp makes and destroys a frame, lays its per-path buffers out and takes its options;
// frame_schedule.cpp decides when its samples run (the stage entries, rt_integrate, the banks); frame_fold_hooks.cpp is the render thread's side of the fold
// adaptation; rt_hip.hip holds every launch of the hot path's code object (frame_launch.h: what the three call there and on each other).  A FEATURE unit
// (frame_filters.cpp, frame_readers.cpp) includes this header alone.  It gets every field of a frame; it may have the stage API's sample replayed into the
// radiance (flush_stage), a deferred sample run after all (deferred_materialize), the pipes joined and the frame's own streams waited for (join_pipes,
// sync_frame_streams), and the guide pass's rays traced (trace_guides: the one launch of the hot path's code object a filter needs).  It cannot launch a
// stage, lay the per-path buffers out or reach the banks' schedule: those are frame_launch.h's, which a feature unit does not include.  The filters' state on
// a frame is a name only here (SfGuides, TfState, SfMotion: frame_filters.cpp), freed through free_filter_state.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "rt_hip.h"
#include "device_scene.h"    // DTile, DLog, DAov, DCounters and the sizes the buffers are made by
#include "context.h"         // rt_ctx

// An owner's device buffers: each one's address and size (clear: it starts from zero).  An owner lists them once (buffers()), for the allocation and for the free.
struct DevBuf { void** p; size_t bytes; bool clear = false; };
static size_t total_bytes(const std::vector<DevBuf>& bufs) { size_t n = 0; for (const DevBuf& b : bufs) n += b.bytes; return n; }
static void free_buffers(const std::vector<DevBuf>& bufs)
{
    for (const DevBuf& b : bufs) if (*b.p) { (void)hipFree(*b.p); *b.p = nullptr; }
}
// a new state S with every buffer of s->buffers(sizes...) allocated, or nullptr with everything freed again if one allocation fails
template <class S, class... Sizes> static S* alloc_state(Sizes... sizes)
{
    S* s = new S();
    const std::vector<DevBuf> bufs = s->buffers(sizes...);
    for (const DevBuf& b : bufs)
        if (hipMalloc(b.p, b.bytes) != hipSuccess)
        {
            (void)hipGetLastError();
            free_buffers(bufs);
            delete s;
            return nullptr;
        }
    return s;
}
template <class S> static void free_state(S*& s)
{
    if (!s) return;
    free_buffers(s->buffers());
    delete s;
    s = nullptr;
}

#define RT_MAX_PIPES 4
// Per-path state of one chunk in flight and the stream its launches go to (see rt_frame::ps).
struct PathPipe
{
    hipStream_t stream = nullptr;      // pipe 0: the context's stream; others: their own
    hipEvent_t done = nullptr;         // cross-stream ordering (fork_pipes / join_pipes)
    // ray queues (ping-pong), hits, shadow queue
    float4* o4[2] = {nullptr, nullptr}; float4* d4[2] = {nullptr, nullptr};
    float4* thr[2] = {nullptr, nullptr};
    float4* hits = nullptr;
    // shadow queue, two of them: bounce b fills [b & 1] while the shadow trace of bounce b - 1 may still read the other
    float4* sh_o4[2] = {nullptr, nullptr}; float4* sh_d4[2] = {nullptr, nullptr}; uint32_t* sh_aux[2] = {nullptr, nullptr};
    // the shadow trace's own stream (rt_integrate: it runs beside the next bounce's closest-hit trace and k_shade,
    // filling the tail of one and the ramp of the other), its spill area and slow-ray list
    hipStream_t side = nullptr;
    hipEvent_t ev_shaded = nullptr, ev_shadow[2] = {nullptr, nullptr};
    bool shadow_in_flight[2] = {false, false};   // ev_shadow[i] recorded and not yet waited for by the main stream
    uint2* sh_spill = nullptr;
    uint32_t* sh_slow_list = nullptr;
    // radiance log (kernels_common.h header): cnt[id], rlog[entry][id]; id < slots * chunk_pixels
    float* rlog = nullptr; uint32_t* cnt = nullptr;   // rlog: 3 floats per entry
    uint32_t* ovf_slot = nullptr;      // compact log layout: a path's overflow block (DLog, kernels_common.h)
    uint32_t* slow_list = nullptr;     // queue indices k_trace_w4 leaves to k_trace2 (one per path)
    DCounters* counters = nullptr;
    uint2* spill = nullptr;
    uint32_t cur_slots = 0;            // slots used by the batch in flight on this pipe (0 = nothing pending)
    uint32_t chunk_base = 0;           // first local pixel of the chunk in flight
    uint32_t chunk_count = 0;          // pixels of the chunk in flight
    uint32_t prev_bounces = 0;
    uint32_t fold_accumulates = 0;     // the sequence in flight is a 2nd+ chunk of its batch: its counters ADD to last_*
    bool shadow_pending = false;       // rt_shade issued, rt_intersect_shadow not yet
    bool primary_fused = false;        // RT_OPT_FUSED_RAYGEN: the batch in flight has no bounce-0 queue in memory: its bounce-0 trace and shade launches make the primary rays (generate_rays)
    uint64_t batch_paths() const { return (uint64_t)chunk_count * (cur_slots ? cur_slots : 1u); }   // paths of the batch in flight (a trace launch's size class)
    // The per-path buffers for `paths` paths in flight and a log of `log_elems` entries, in the order they are allocated (alloc_path_buffers /
    // free_path_buffers; no arguments: all of them, for the free).  The queues carry 4 elements of padding, the slow lists 64, the log 16 bytes;
    // ovf_slot exists in the compact layout only.  RT_PATH_FIXED_BYTES is this list without the log and ovf_slot, per path.
    std::vector<DevBuf> buffers(size_t paths = 0, size_t log_elems = 0, bool compact = true)
    {
        const size_t q = (paths + 4) * sizeof(float4), w = (paths + 4) * sizeof(uint32_t), slow = (paths + 64) * sizeof(uint32_t);
        std::vector<DevBuf> b = {{(void**)&o4[0], q}, {(void**)&o4[1], q}, {(void**)&d4[0], q}, {(void**)&d4[1], q}, {(void**)&thr[0], q}, {(void**)&thr[1], q},
            {(void**)&hits, q}, {(void**)&sh_o4[0], q}, {(void**)&sh_d4[0], q}, {(void**)&sh_o4[1], q}, {(void**)&sh_d4[1], q}, {(void**)&sh_aux[0], w},
            {(void**)&sh_aux[1], w}, {(void**)&rlog, log_elems * 3u * sizeof(float) + 16u}};
        if (compact) b.push_back({(void**)&ovf_slot, w});
        b.insert(b.end(), {DevBuf{(void**)&cnt, paths * sizeof(uint32_t)}, DevBuf{(void**)&slow_list, slow}, DevBuf{(void**)&sh_slow_list, slow}});
        return b;
    }
    // what a pipe keeps for the frame's life (ensure_pipe_resources); its streams have drained.  Pipe 0's stream is borrowed: never destroyed.
    void destroy(bool own_stream)
    {
        for (void* m : {(void*)counters, (void*)spill, (void*)sh_spill}) if (m) (void)hipFree(m);
        for (hipEvent_t e : {done, ev_shaded, ev_shadow[0], ev_shadow[1]}) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};
#define RT_PATH_FIXED_BYTES (11u * 16u + 5u * 4u)   // ray queues o4, d4, thr (x2), hits, shadow queue o4, d4 (x2) = 11 x 16; sh_aux (x2), cnt, two slow lists = 5 x 4

// RT_OPT_SAMPLES_AHEAD: samples of the stage API traced ahead of the caller's Integrate() calls (below, "samples ahead").  A BANK is a frame of its
// own -- same tile, same options, its own per-path buffers -- that holds one batch; two banks, so that one computes while the other is consumed.
struct AheadBank
{
    rt_frame* h = nullptr;
    uint32_t base = 0, n = 0, next = 0;     // holds samples base .. base + n - 1; slots < next have reached the owner's radiance
    hipEvent_t done = nullptr;              // the batch's last launch (the bank's stream, after its side stream has been joined)
    hipEvent_t order = nullptr;             // what the bank's stream waits for before it starts another batch: the owner's last replay of the old one
};
// what a bank is made for: a change in any of the sixteen makes the banks over (ahead_key / ahead_configure, frame_schedule.cpp)
struct AheadKey
{
    uint32_t followed[12] = {};             // the options of RT_AHEAD_FOLLOWED, in its order
    uint32_t small_launch = 0, tail_paths = 0;   // RT_OPT_SMALL_LAUNCH_PATHS (unset: 0xFFFFFFFF), RT_OPT_TRACE_TAIL_PATHS
    uint32_t depth = 0;                     // samples per batch (ahead_depth)
    uint32_t two_streams = 0;               // RT_OPT_SAMPLES_AHEAD + 256: one stream per bank
};
struct Ahead
{
    AheadBank bank[2];
    hipStream_t stream[2] = {nullptr, nullptr};
    uint32_t quiet = 0;                     // samples advanced since the last reset / discard
    uint32_t depth = 0, last_n = 0;         // the most samples a batch holds (resolved for this tile); the latest batch's size (the ramp: 2, 4, .. depth)
    bool configured = false;
    AheadKey mirrored;                      // the owner's options as the banks have them
    rt_camera camera;                       // what the batches in flight were traced for
    uint64_t scene = 0;
    uint64_t launched = 0, consumed = 0, discarded = 0;   // samples
};

// the filters' state on a frame (frame_filters.cpp)
struct SfGuides;
struct TfState;
struct SfMotion;

struct rt_frame
{
    rt_ctx* ctx;
    DTile tile;
    uint32_t n_local;
    float4* radiance = nullptr; float4* resolved = nullptr;
    // rt_frame_present: the resolved image goes to the host on a stream of its own while the next frame is traced
    float4* resolved_b = nullptr;      // the second device image (double buffering)
    hipStream_t present_stream = nullptr;
    hipEvent_t ev_resolved[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    uint32_t present_flip = 0;
    bool present_pending = false;
    // Per-path state lives in PIPES (PathPipe): the tile is cut into chunks of pixels and chunk c travels through
    // the wavefront loop on pipe c % n_pipes, each pipe on its own HIP stream.  One chunk on one pipe is the plain
    // case.  More pipes let chunks overlap; measured on MI355X this does NOT pay (a trace launch costs ~0.8 ms
    // beyond its rays whatever shares the machine with it: profiles/r02_pipelines_sweep.log), so the default is 1.
    PathPipe ps[RT_MAX_PIPES];
    uint32_t pipelines = 1;        // RT_OPT_PIPELINES: pipes rt_integrate may use
    uint32_t stage_pipes = 1;      // RT_OPT_STAGE_PIPES: ONE sample per pixel in flight (the stage API, rt_integrate(f, 1): the reference's frame-by-frame
                                   // pattern) is cut into this many chunks, each on a pipe (stream) of its own: every launch of that pattern is
                                   // its own tail, and the chunks' tails overlap
    uint32_t stage_chunks = 1;     // pipes holding a chunk of the stage API's sample in flight (set by rt_generate_rays)
    // RT_OPT_FRAME_KERNEL: the stage API's sample as ONE launch (k_frame, frame_kernels.h).  The stage calls of a sample are only RECORDED
    // while they come in the canonical order; rt_advance_sample launches the kernel.  Anything that needs the state between two stages
    // (a debug reader, the radiance mid-sample, another order of calls) first replays the recorded stages with the stage kernels.
    uint32_t frame_kernel = 0;
    struct { bool active = false; uint32_t bounce = 0; int next = 0; bool ahead = false; } deferred;   // next: 0 = rt_intersect(bounce), 1 = rt_shade, 2 = rt_intersect_shadow;
                                                                                                      // ahead: the sample is in a bank (RT_OPT_SAMPLES_AHEAD)
    uint32_t ahead_opt = 0;            // RT_OPT_SAMPLES_AHEAD
    Ahead* ahead = nullptr;            // ... its banks (made when the first batch is launched)
    rt_frame* ahead_owner = nullptr;   // this frame IS a bank of that frame
    struct KFrame                      // k_frame's grid and its buffers, all three or none (blocks != 0: they exist)
    {
        uint32_t* counts = nullptr; uint32_t* slow = nullptr;                      // per-wave rows and slow-ray lists
        uint2* spill = nullptr;                                                    // ... and its blocks' stack spill area
        uint32_t blocks = 0;
        std::vector<DevBuf> buffers(size_t n_blocks = 0, size_t chunks_per_wave = 0)
        {
            return {{(void**)&counts, n_blocks * RT_FRAME_COUNT_STRIDE * sizeof(uint32_t)}, {(void**)&slow, n_blocks * chunks_per_wave * 64u * sizeof(uint32_t)},
                    {(void**)&spill, n_blocks * 64u * (RT_W4_STACK_MAX - 12) * sizeof(uint2)}};
        }
        void release() { free_buffers(buffers()); blocks = 0; }
    } kf;
    uint32_t frame_chunks_per_wave = 0;
    uint64_t fused_launches = 0;                                                   // RT_OPT_FUSED_RAYGEN: k_raygen launches that ran their prologue only (rt_stats)
    uint64_t frame_launches = 0;                                                   // samples rendered by k_frame so far (rt_stats)
    // RT_OPT_FRAME_KERNEL = 255: the choice is MEASURED -- k_frame wins by 1.4 - 1.8 x on scenes of up to ~1 M triangles and loses 7 - 10 % on the 2.8 M /
    // 10 M ones (profiles/r05_call13.log), so the first frames of a scene time both: frames 0 - 1 (stage kernels) and 2 - 3 (k_frame) warm up, frames 4 - 19
    // ALTERNATE between the two (the device's clocks ramp over a process's first frames: timed in two blocks, whichever came second looked faster --
    // rt_render --frames chose k_frame for the 2.8 M-triangle scene, profiles/r05_call18.log) with HIP events around each frame's launches on the frame's
    // stream, read once the last has completed; then the faster way stays.
    struct { int frames = 0, timing = -1; bool decided = false, use_kernel = false, skip = false; uint64_t scene = 0; hipEvent_t ev[16][2] = {}; float ms_stage = 0.0f, ms_kernel = 0.0f; } fk_auto;
    uint32_t n_pipes = 1;          // pipes the current allocation holds
    uint32_t slots = 1;            // samples traced concurrently (resolved from slots_opt)
    uint32_t slots_opt = 0;        // RT_OPT_SAMPLES_IN_FLIGHT as set by the caller (0 = auto)
    uint32_t slots_limit = 0;      // != 0: a larger batch did not fit into device memory
    bool reserved_explicitly = false;  // rt_frame_reserve_samples has been called: rt_integrate does not second-guess the buffers' size
    uint64_t samples_asked = 0;        // samples rt_integrate has been asked for since the frame was made (lean growth of the buffers)
    uint32_t log_stride = 0;       // elements per log entry row = slots * chunk_pixels
    // Chunks also bound memory: RT_OPT_PATH_STATE_LIMIT_MB caps the per-path buffers of all pipes together
    // (path ids are chunk-relative, the radiance log is replayed per chunk).
    uint32_t chunk_pixels = 0;     // pixels per chunk as allocated (n_local when the tile is not chunked)
    uint32_t state_limit_mb = 0;   // RT_OPT_PATH_STATE_LIMIT_MB (0 = only the built-in 144 GB rule)
    uint32_t log_entries = 0;      // entries a path may log: 2 * (max_bounces + 1)
    // Radiance-log layout (DLog): compact = log_inline rows for every path + a pool of log_ovf_blocks overflow blocks;
    // full = every row for every path (log_inline == log_entries, no pool).
    uint32_t log_inline = 0, log_ovf_blocks = 0;
    uint32_t compact_log_opt = 2;  // RT_OPT_COMPACT_LOG: 0 = always the full layout, 1 = compact for batches of >= 8 samples in flight,
                                   // 2 (default) = compact when the caller bounds the path state (RT_OPT_PATH_STATE_LIMIT_MB)
    uint32_t log_pool_div = 8;     // the pool holds paths / log_pool_div blocks (RT_OPT_DEBUG_LOG_POOL_DIV: test hook)
    bool log_full_forced = false;  // a batch ran its pool dry: this frame stays on the full layout (until bounces / scene change)
    uint32_t fallback_limit_mb = 0;   // ... within the bytes the compact layout held (chunk_plan)
    uint32_t log_fallbacks = 0;    // batches repeated in the full layout
    uint32_t trace_blocks;       // v1 grid
    uint32_t trace_variant = 5;  // RT_OPT_TRACE_VARIANT (5 = auto)
    uint64_t small_launch_paths = 3000000ull;   // RT_OPT_SMALL_LAUNCH_PATHS: launches of fewer rays run k_trace_w4 in chunk mode
    bool small_launch_set = false;              // ... set by the caller (otherwise the loop-D instance uses 8 M: launch_trace_w4)
    uint32_t trace_waves_per_cu = 0;   // RT_OPT_TRACE_WAVES_PER_CU (0 = LDS-limited residency)
    uint32_t chunk_refill = 1;                 // RT_OPT_CHUNK_REFILL: chunk mode refills idle lanes from the wave's own chunks
    uint32_t fused_raygen = 1;                 // RT_OPT_FUSED_RAYGEN: rt_integrate's bounce-0 launches make their primary rays themselves (primary_fusable)
    uint64_t trace_tail_paths = 100000000ull; // RT_OPT_TRACE_TAIL_PATHS: batches of fewer paths launch the instance with loop D and refilled chunks (8 / 16 / 32 / 64 /
                                              // 128 samples of a 1080p frame in flight: +8 / +5 / +2.3 / -1.6 / -2.8 %, profiles/r04_call20_21.log, r04_call22.log)
    uint32_t trace_tail_lanes = 40;    // RT_OPT_TRACE_TAIL_LANES: k_trace_w4's loop D (0 = off); sweep: profiles/r04_call04_kernel_ab.log
    uint32_t select_form_box = 0;      // RT_OPT_TRACE_SELECT_FORM_BOX: every ray takes the select-form slab test
    uint32_t trace_tune = 0;           // RT_OPT_TRACE_TUNE: k_trace2 loop thresholds (0 = defaults)
    uint32_t timeline = 0;             // rt_frame_debug_timeline armed: k_trace_w4<closest> records its launch timeline
    uint32_t overlap_shadow = 1;       // RT_OPT_OVERLAP_SHADOW
    bool side_active = false;          // shadow traces go to PathPipe::side (what the last shade step decided, side_on(): it holds until that bounce's shadow trace)
    uint32_t shade_partition = 3;      // RT_OPT_SHADE_PARTITION: bit 0: k_shade sorts each block's entries hits first / misses last; bit 1: groups its output rays by octant
    uint32_t debug_alloc_limit = 0;    // RT_OPT_DEBUG_ALLOC_LIMIT: allocations above this many samples in flight fail
    // integrator state
    rt_camera camera;
    rt_camera camera_last;        // Integrator::prev_camera_ (integrator.hpp:89)
    rt_camera prev_camera;        // the kPrevCamera argument bound by the last rt_set_camera
    uint32_t sampler = 0;         // RT_OPT_SAMPLER: 0 kRandom, 1 kBlueNoise
    uint32_t aov = 0;             // RT_OPT_AOV
    uint32_t denoiser = 0;        // RT_OPT_DENOISER
    DAov aov_buf = {nullptr, nullptr, nullptr, nullptr};
    float4* prev_radiance = nullptr; float* prev_depth = nullptr;
    uint32_t max_bounces = 3;
    uint32_t white_furnace = 0;
    uint32_t drop_last = 1;
    uint32_t sample_count = 0;
    // RT_OPT_PROFILE_KERNELS
    uint32_t profile = 0;
    struct Span { hipEvent_t a, b; int cls; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    struct SfGuides* sf = nullptr;     // rt_frame_filter / rt_frame_read_guides: the guide pass's buffers and what they were made for (made on first use)
    struct TfState* tf = nullptr;      // rt_frame_filter_temporal: the history (made on first use)
    struct SfMotion* sm = nullptr;     // RT_CTX_OPT_REFIT_MOTION: where each first hit was before the last refit (made on first use)
    // the images a frame is made with, n pixels each (the radiance and the resolved image are written before they are read: rt_reset, rt_frame_resolve)
    std::vector<DevBuf> images(size_t n = 0)
    {
        return {{(void**)&radiance, n * sizeof(float4)}, {(void**)&resolved, n * sizeof(float4)}, {(void**)&aov_buf.diffuse_albedo, n * sizeof(float4), true},
                {(void**)&aov_buf.depth, n * sizeof(float), true}, {(void**)&aov_buf.normal, n * sizeof(float4), true}, {(void**)&aov_buf.velocity, n * sizeof(float2), true},
                {(void**)&prev_radiance, n * sizeof(float4), true}, {(void**)&prev_depth, n * sizeof(float), true}};
    }
};

// the tile's pixels, at least 1: a rank may hold no row of a small image, and buffers, grids and chunks are sized for one pixel then
static uint32_t tile_pixels(const rt_frame* f) { return f->n_local ? f->n_local : 1u; }

// what every entry that works on a frame's scene begins with
#define FRAME_PROLOGUE(f, name)                                                         \
    if (!(f)) return fail(nullptr, name ": frame is NULL");                             \
    rt_ctx* ctx = (f)->ctx;                                                             \
    if (!ctx->scene.valid) return fail(ctx, name ": no scene uploaded");                \
    (void)hipSetDevice(ctx->device)

// What a feature unit, or the context, calls on the frames' units.  Each is defined among the functions it works with: flush_stage, deferred_materialize and
// ahead_discard in frame_schedule.cpp, join_pipes and sync_frame_streams in frame_layout.cpp, fold_adapt_hook in frame_fold_hooks.cpp, trace_guides in rt_hip.hip.
namespace frame
{
// the logs of the pipes that hold the stage API's sample replayed into the radiance (keep: the sample stays open; a deferred sample runs its recorded
// stages first), and the context's stream made to see all of them
int flush_stage(rt_frame* f, bool keep = false);
// the context's stream waits for everything the pipes have been given
int join_pipes(rt_frame* f);
// waits (host side) for every stream a frame launches on besides the context's own
int sync_frame_streams(rt_frame* f);
// RT_OPT_FRAME_KERNEL: the recorded stages of a deferred sample, run with the stage kernels after all (nothing deferred: nothing to do)
int deferred_materialize(rt_frame* f);
// RT_OPT_SAMPLES_AHEAD: whatever was traced ahead is dropped (reset, another camera, another option, a peek; context::quiesce before a scene changes)
void ahead_discard(rt_frame* f);
// RT_CTX_OPT_ADAPTIVE_FOLD on the render thread: probe, hand-over to the worker, adoption.  rt_generate_rays and rt_integrate call it before a frame's first stage.
int fold_adapt_hook(rt_frame* f);
// The guide pass's closest-hit trace (ensure_guides, frame_filters.cpp): the n rays o4 / d4, live count `count`, by the per-ray BVH2 kernel on the context's
// stream into the filter's own `hits`, with its own `spill` area.  A launch of the hot path's code object, hence rt_hip.hip's; the caller reads hipGetLastError.
void trace_guides(rt_frame* f, const float4* o4, const float4* d4, float4* hits, uint2* spill, const uint32_t* count, size_t n);
// frees the three filter states of a frame that is being destroyed (frame_filters.cpp, where their records are)
void free_filter_state(rt_frame* f);
} // namespace frame
