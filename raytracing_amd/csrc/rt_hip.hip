// rt_hip.hip -- implementation of the C-ABI in include/rt_hip.h over HIP for
// gfx950.  Replaces the reference's src/gpu_wrappers/cl_context.cpp and the
// device-facing half of src/integrator/cl_pt_integrator.cpp.
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
#include <map>
#include <thread>
#include <atomic>
#include <array>
#include <functional>
#include "rt_hip.h"
#include "kernels.h"
#include <chrono>
#include "wide_bvh.h"        // truncated_walks_exchange, for the adaptation's report line (wide_bvh.cpp)
#include "query_host.h"      // the queries' scratch areas and the ray through a pixel, for rt_frame_pick and rt_frame_pick_all (query.hip)
#include "bake_host.h"       // bake::CHUNK_POINTS, for RT_CTX_OPT_BAKE_CHUNK_POINTS (bake.hip)
#include "region_host.h"     // the region of a pixel rectangle, for rt_frame_pick_rect (region.hip)
#include "device_memory.h"   // who owns a device allocation: dev::Mem
#include "context.h"         // Scene, rt_ctx, rt_buffer, fail / HIPCHK: what this unit shares with the feature units that implement entry points (scene_upload.cpp, scene_queries.cpp)
#include "frame.h"           // rt_frame, its pipes, banks and buffer lists, and what the frames' feature units call here (frame_filters.cpp, frame_readers.cpp): namespace frame
#include "fold_adapt.h"      // FoldAdapt, for the render thread's side of the adaptation (fold_hooks_impl.h); the upload's side and the worker: scene_upload.cpp
using namespace rtw;
using namespace context;
using namespace frame;

namespace
{
thread_local std::string g_thread_error;
} // namespace

static void ahead_discard(rt_frame* f);      // RT_OPT_SAMPLES_AHEAD: whatever was traced ahead is dropped (reset, another camera, another option, a peek)
static void ahead_destroy(rt_frame* f);
static bool ahead_wanted(const rt_frame* f);
static int ahead_holds(const rt_frame* f, uint32_t sample);

// context.h's functions: the one place a message is stored, the device copies of an upload, the queries' status word
namespace context
{
int fail(rt_ctx* ctx, const std::string& msg)
{
    if (ctx) ctx->error = msg;
    g_thread_error = msg;
    return RT_ERROR;
}

// m = `bytes` of device memory with src's bytes on their way into it on ctx's stream (no src: nothing is copied); a failure is `who`'s error
int dev_fill(rt_ctx* ctx, const char* who, dev::Mem& m, const void* src, size_t bytes)
{
    if (!m.alloc(bytes)) return fail(ctx, std::string(who) + ": out of device memory");
    if (!m.upload(ctx->stream, src, bytes)) return fail(ctx, std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

// the same for a raw field of the Scene (free_scene's to free): it is set only when the allocation and the copy both worked
int scene_array(rt_ctx* ctx, void** field, const void* src, size_t bytes)
{
    dev::Mem m;
    *field = nullptr;
    if (dev_fill(ctx, "rt_scene_upload", m, src, bytes) != RT_OK) return RT_ERROR;
    *field = m.release();
    return RT_OK;
}

// Ray queries: the walk's status word (pinned host memory; bit 0: a traversal stack ran over its bound, query_kernels.h), read and cleared wherever the
// context's stream has just been waited for -- rt_scene_trace, rt_finish, rt_buffer_read -- so that the buffer form's queries report it too.
int query_check_status(rt_ctx* ctx, const char* who)
{
    volatile uint32_t* st = ctx->query.status;
    if (!st || *st == 0u) return RT_OK;
    *st = 0u;
    return fail(ctx, std::string(who) + ": a ray query's traversal stack ran over its bound (a tree deeper than the walk's stack): that query's results are not valid");
}

// Nothing in flight may still read what is about to be freed or rewritten: batches traced ahead are dropped (RT_OPT_SAMPLES_AHEAD), and every stream a frame
// launches on -- side streams, pipes, banks -- has drained.
int quiesce(rt_ctx* ctx)
{
    for (rt_frame* f : ctx->frames) ahead_discard(f);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (rt_frame* f : ctx->frames)
        if (sync_frame_streams(f) != RT_OK) return RT_ERROR;
    return RT_OK;
}
} // namespace context

extern "C" {

const char* rt_last_error(rt_ctx* ctx)
{
    return ctx ? ctx->error.c_str() : g_thread_error.c_str();
}

int rt_ctx_create(int device_ordinal, rt_ctx** out)
{
    if (!out) return fail(nullptr, "rt_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, std::string("rt_ctx_create: no HIP device (") + hipGetErrorString(e) + ")");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, "rt_ctx_create: bad device ordinal");
    rt_ctx* ctx = new rt_ctx;
    ctx->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_ordinal) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
    {
        delete ctx;
        return fail(nullptr, "rt_ctx_create: device initialisation failed");
    }
    if (hipMalloc((void**)&ctx->gamma_lut, 256 * sizeof(float)) != hipSuccess)
    {
        delete ctx;
        return fail(nullptr, "rt_ctx_create: out of device memory");
    }
    hipLaunchKernelGGL(k_fill_gamma_lut, dim3(1), dim3(256), 0, ctx->stream, ctx->gamma_lut);
    *out = ctx;
    return RT_OK;
}

int rt_ctx_destroy(rt_ctx* ctx)
{
    if (!ctx) return RT_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    free_scene(ctx->scene);
    query::release(ctx->query);
    query::release(ctx->bake);
    if (ctx->blue_noise) (void)hipFree(ctx->blue_noise);
    if (ctx->gamma_lut) (void)hipFree(ctx->gamma_lut);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return RT_OK;
}

int rt_finish(rt_ctx* ctx)
{
    if (!ctx) return fail(nullptr, "rt_finish: ctx is NULL");
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // ... and for whatever the frames put on streams of their own: chunks on other pipes, shadow traces on the side streams
    // (the stage API sends them there too since round 3) -- Finish() means everything (cl_context.cpp:115-118)
    // (not for the banks of RT_OPT_SAMPLES_AHEAD: what they trace ahead is the library's own business until a later Integrate() consumes it)
    for (rt_frame* f : ctx->frames)
        if (!f->ahead_owner && sync_frame_streams(f) != RT_OK) return RT_ERROR;
    return query_check_status(ctx, "rt_finish");
}

int rt_ctx_device_info(rt_ctx* ctx, char* name, size_t name_len, int* compute_units, size_t* hbm_bytes)
{
    if (!ctx) return fail(nullptr, "rt_ctx_device_info: ctx is NULL");
    if (name && name_len) snprintf(name, name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = ctx->prop.totalGlobalMem;
    return RT_OK;
}

void* rt_ctx_stream(rt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int rt_host_register(rt_ctx* ctx, void* host_ptr, size_t bytes)
{
    if (!ctx || !host_ptr || bytes == 0) return fail(ctx, "rt_host_register: bad argument");
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    return RT_OK;
}

int rt_host_unregister(rt_ctx* ctx, void* host_ptr)
{
    if (!ctx || !host_ptr) return fail(ctx, "rt_host_unregister: bad argument");
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipHostUnregister(host_ptr));
    return RT_OK;
}

// The sampler tables CLPathTraceIntegrator uploads in its ctor (cl_pt_integrator.cpp:222-235)
int rt_upload_blue_noise_tables(rt_ctx* ctx, const int* sobol_256spp_256d, const int* scramblingTile, const int* rankingTile)
{
    if (!ctx || !sobol_256spp_256d || !scramblingTile || !rankingTile)
        return fail(ctx, "rt_upload_blue_noise_tables: NULL argument");
    (void)hipSetDevice(ctx->device);
    std::vector<uint8_t> packed(65536 + 131072 + 131072);
    const int* src[3] = {sobol_256spp_256d, scramblingTile, rankingTile};
    const size_t n[3] = {65536, 131072, 131072};
    size_t o = 0;
    for (int t = 0; t < 3; ++t)
        for (size_t i = 0; i < n[t]; ++i)
        {
            if (src[t][i] < 0 || src[t][i] > 255) return fail(ctx, "rt_upload_blue_noise_tables: table value outside 0..255");
            packed[o++] = (uint8_t)src[t][i];
        }
    if (!ctx->blue_noise) HIPCHK(ctx, hipMalloc((void**)&ctx->blue_noise, packed.size()));
    HIPCHK(ctx, hipMemcpy(ctx->blue_noise, packed.data(), packed.size(), hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_ctx_set_option(rt_ctx* ctx, int option, uint32_t value)
{
    if (!ctx) return fail(nullptr, "rt_ctx_set_option: ctx is NULL");
    if (option == RT_CTX_OPT_TREELET_NODES)
    {
        if (value == 0 || value > 4096) return fail(ctx, "rt_ctx_set_option: treelet size must be 1..4096");
        ctx->treelet_nodes = value;
        return RT_OK;
    }
    if (option == RT_CTX_OPT_WIDE_BVH) { ctx->build_wide = value > 2u ? 1u : value; return RT_OK; }
    if (option == RT_CTX_OPT_SHADOW_TREE) { ctx->shadow_tree = value > 3u ? 1u : value; return RT_OK; }
    if (option == RT_CTX_OPT_CLOSEST_TREE) { ctx->closest_tree = value > 2u ? 1u : value; return RT_OK; }
    if (option == RT_CTX_OPT_ADAPTIVE_FOLD) { ctx->adaptive_fold = value & 31u; return RT_OK; }
    if (option == RT_CTX_OPT_DEVICE_FOLD) { ctx->device_fold = value ? 1u : 0u; return RT_OK; }
    if (option == RT_CTX_OPT_WIDE_LAYOUT) { ctx->wide_layout = value ? 1u : 0u; return RT_OK; }
    if (option == RT_CTX_OPT_REFITTABLE) { ctx->refittable = value ? 1u : 0u; return RT_OK; }
    if (option == RT_CTX_OPT_REFIT_MOTION) { ctx->refit_motion = value ? 1u : 0u; return RT_OK; }
    if (option == RT_CTX_OPT_TREE_BUILDER) { ctx->tree_builder = value > 2u ? 2u : value; return RT_OK; }
    if (option == RT_CTX_OPT_ADAPT_WAIT)
    {
        if (ctx->scene.adapt) fold_adapt_set_wait(ctx->scene.adapt, value != 0u);          // the scene in place only
        return RT_OK;
    }
    if (option == RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS)
    {
        ctx->adapt_min_interval_ms = value;
        if (ctx->scene.adapt) fold_adapt_set_interval(ctx->scene.adapt, value);     // the scene in place too
        return RT_OK;
    }
    if (option == RT_CTX_OPT_BAKE_CHUNK_POINTS) { ctx->bake_chunk_points = value == 0u || value > (uint32_t)bake::CHUNK_POINTS ? (uint32_t)bake::CHUNK_POINTS : value; return RT_OK; }
    return fail(ctx, "rt_ctx_set_option: unknown option");
}

// ---- buffers ---------------------------------------------------------------
int rt_buffer_create(rt_ctx* ctx, size_t bytes, const void* init, rt_buffer** out)
{
    if (!ctx || !out) return fail(ctx, "rt_buffer_create: NULL argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    void* p = nullptr;
    HIPCHK(ctx, hipMalloc(&p, bytes ? bytes : 16));
    if (init && bytes)
    {
        hipError_t e = hipMemcpy(p, init, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return fail(ctx, "rt_buffer_create: upload failed"); }
    }
    *out = new rt_buffer{ctx, p, bytes};
    return RT_OK;
}

int rt_buffer_destroy(rt_buffer* buf)
{
    if (!buf) return RT_OK;
    (void)hipStreamSynchronize(buf->ctx->stream);
    (void)hipFree(buf->ptr);
    delete buf;
    return RT_OK;
}

int rt_buffer_write(rt_buffer* buf, size_t offset, const void* src, size_t bytes)
{
    if (!buf || !src) return fail(nullptr, "rt_buffer_write: NULL argument");
    if (offset + bytes > buf->bytes) return fail(buf->ctx, "rt_buffer_write: out of range");
    HIPCHK(buf->ctx, hipMemcpyAsync((char*)buf->ptr + offset, src, bytes, hipMemcpyHostToDevice, buf->ctx->stream));
    HIPCHK(buf->ctx, hipStreamSynchronize(buf->ctx->stream));   // blocking, like WriteBuffer (CL_TRUE)
    return RT_OK;
}

int rt_buffer_read(rt_buffer* buf, size_t offset, void* dst, size_t bytes)
{
    if (!buf || !dst) return fail(nullptr, "rt_buffer_read: NULL argument");
    if (offset + bytes > buf->bytes) return fail(buf->ctx, "rt_buffer_read: out of range");
    HIPCHK(buf->ctx, hipMemcpyAsync(dst, (char*)buf->ptr + offset, bytes, hipMemcpyDeviceToHost, buf->ctx->stream));
    HIPCHK(buf->ctx, hipStreamSynchronize(buf->ctx->stream));
    return query_check_status(buf->ctx, "rt_buffer_read");
}

int rt_buffer_copy(rt_buffer* src, rt_buffer* dst, size_t src_offset, size_t dst_offset, size_t bytes)
{
    if (!src || !dst) return fail(nullptr, "rt_buffer_copy: NULL argument");
    if (src_offset + bytes > src->bytes || dst_offset + bytes > dst->bytes)
        return fail(src->ctx, "rt_buffer_copy: out of range");
    HIPCHK(src->ctx, hipMemcpyAsync((char*)dst->ptr + dst_offset, (char*)src->ptr + src_offset, bytes,
        hipMemcpyDeviceToDevice, src->ctx->stream));
    return RT_OK;
}

void* rt_buffer_device_ptr(rt_buffer* buf) { return buf ? buf->ptr : nullptr; }
size_t rt_buffer_size(rt_buffer* buf) { return buf ? buf->bytes : 0; }

} // extern "C"

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

// Per-path state: ray queues for `slots` samples in flight and the radiance log
// with 2 * (max_bounces + 1) entries per path.  (Re)allocated when either changes.
// Compact radiance log (kernels_common.h, DLog): six inline entries per path + overflow blocks for an eighth of the paths.
#define RT_LOG_INLINE 6u
// may a batch of `slots` samples in flight use the compact layout?  (It pays from ~10 entries per path up, needs batches large
// enough for the pool's statistics, and one pipe: the pool-dry check synchronises the host with the chunk's stream.)
bool log_is_compact(const rt_frame* f, uint32_t slots)
{
    const bool asked = f->compact_log_opt == 1u || (f->compact_log_opt == 2u && f->state_limit_mb != 0u);
    return asked && !f->log_full_forced && slots >= 8u && f->pipelines == 1u && 2u * (f->max_bounces + 1u) >= RT_LOG_INLINE + 4u;
}

// A path's bytes in the full layout: the fixed buffers + a log of 2 (B + 1) entries of 12 bytes -- 412 bytes at 8 bounces (rounds 1-2: 540).
size_t full_bytes_per_path(uint32_t max_bounces) { return RT_PATH_FIXED_BYTES + 12u * 2u * (max_bounces + 1u); }

// ... and in the layout a batch of `slots` samples in flight gets; compact: 6 inline entries + the path's share of the overflow pool + its block
// index -- 290 bytes at 8 bounces, 314 at 16.
size_t bytes_per_path(const rt_frame* f, uint32_t slots)
{
    if (!log_is_compact(f, slots)) return full_bytes_per_path(f->max_bounces);
    const size_t entries = 2u * (f->max_bounces + 1u);
    return RT_PATH_FIXED_BYTES + 4u + 12u * RT_LOG_INLINE + (12u * (entries - RT_LOG_INLINE) + f->log_pool_div - 1u) / f->log_pool_div;
}

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

// the most samples rt_integrate will trace together
uint32_t slot_cap(const rt_frame* f)
{
    uint32_t cap = f->slots_opt ? f->slots_opt : auto_slots(f);
    return f->slots_limit && f->slots_limit < cap ? f->slots_limit : cap;    // what the device could actually hold
}

// How the tile is cut for `slots` samples in flight: number of pipes and pixels per chunk.
//  * two (RT_OPT_PIPELINES) pipes when a batch is large enough for its launches to fill the machine twice over
//    (>= 2 samples in flight and >= 4 M paths): the tile's halves then overlap each other's launch tails;
//  * RT_OPT_PATH_STATE_LIMIT_MB bounds the per-path buffers of all pipes together: more, smaller chunks
//    (multiples of 4096 pixels), still dealt round-robin to the pipes.
void chunk_plan(const rt_frame* f, uint32_t slots, uint32_t& n_pipes, uint32_t& chunk_pixels)
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

uint32_t chunk_for(const rt_frame* f, uint32_t slots)
{
    uint32_t np, c;
    chunk_plan(f, slots, np, c);
    return c;
}

int alloc_path_buffers(rt_frame* f, uint32_t slots)
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
int fork_pipes(rt_frame* f)
{
    rt_ctx* ctx = f->ctx;
    if (f->n_pipes <= 1) return RT_OK;
    HIPCHK(ctx, hipEventRecord(f->ps[0].done, ctx->stream));
    for (uint32_t i = 1; i < f->n_pipes; ++i) HIPCHK(ctx, hipStreamWaitEvent(f->ps[i].stream, f->ps[0].done, 0));
    return RT_OK;
}

} // namespace

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

int flush_log(rt_frame* f, PathPipe& p, bool keep_open = false);

// The pipe's main stream waits for the shadow trace that last used its shadow queue `q` (those run on PathPipe::side);
// nothing to do when none is outstanding.
int wait_shadow(rt_frame* f, PathPipe& p, uint32_t q)
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
bool side_on(const rt_frame* f) { return f->overlap_shadow != 0 && !(f->denoiser || f->aov != 0); }

// Grows the per-path buffers to hold `want` samples in flight (clamped to slot_cap); they
// are sized by the largest batch actually requested, not by the cap.
int ensure_slots(rt_frame* f, uint32_t want)
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

// the radiance log of a pipe as the kernels see it
DLog dlog(const rt_frame* f, const PathPipe& p)
{
    DLog L;
    L.rlog = p.rlog; L.cnt = p.cnt; L.ovf_slot = f->log_ovf_blocks ? p.ovf_slot : nullptr;
    L.stride = f->log_stride; L.inline_entries = f->log_inline; L.ovf_blocks = f->log_ovf_blocks;
    return L;
}

// The stage API and the per-frame features (AOVs, denoiser) trace ONE sample of the WHOLE tile.  The buffers may have
// been cut into chunks for an earlier, larger batch under RT_OPT_PATH_STATE_LIMIT_MB (ensure_slots keeps an allocation
// that is large enough in SLOTS): re-allocate for one sample in flight, which the caller has checked does fit.
int ensure_whole_tile(rt_frame* f)
{
    if (f->chunk_pixels >= tile_pixels(f)) return RT_OK;
    if (f->ps[0].cur_slots != 0) return fail(f->ctx, "rt_generate_rays: the previous sample was not advanced (rt_advance_sample)");
    if (flush_log(f, f->ps[0]) != RT_OK || join_pipes(f) != RT_OK) return RT_ERROR;
    HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return alloc_path_buffers(f, 1);
}

// Adds the logged contributions of the batch in flight on pipe `p` to the running sum.
int flush_log(rt_frame* f, PathPipe& p, bool keep_open)
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

} // namespace

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
// Mid-sample read (stage API / debugging): apply what has been logged so far but
// keep the sample open -- later contributions append again from entry 0.
int flush_log_keep(rt_frame* f, PathPipe& p)
{
    uint32_t keep = p.cur_slots;
    int rc = flush_log(f, p, true);
    p.cur_slots = keep;
    return rc;
}

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

namespace
{

// RT_OPT_FRAME_KERNEL = 255 measures again: another workload, or another grid
void fk_auto_restart(rt_frame* f) { f->fk_auto.frames = 0; f->fk_auto.timing = -1; f->fk_auto.decided = false; f->fk_auto.use_kernel = false; }

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

extern "C" {

static int create_frame(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out, hipStream_t borrowed_main_stream);

int rt_frame_create(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out) { return create_frame(ctx, fd, out, nullptr); }

// borrowed_main_stream != NULL: pipe 0 launches there instead of on the context's stream (a bank of RT_OPT_SAMPLES_AHEAD; the stream stays the lender's)
static int create_frame(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out, hipStream_t borrowed_main_stream)
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

#define FRAME_PROLOGUE(f, name)                                                         \
    if (!(f)) return fail(nullptr, name ": frame is NULL");                             \
    rt_ctx* ctx = (f)->ctx;                                                             \
    if (!ctx->scene.valid) return fail(ctx, name ": no scene uploaded");                \
    (void)hipSetDevice(ctx->device)

} // extern "C"

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

extern "C" {

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

} // extern "C"

namespace
{
// Primary rays for `n_slots` consecutive samples (sample indices sample_count ..
// sample_count + n_slots - 1) in one launch on pipe `p`; they then travel through that pipe's queues.
// RT_OPT_FUSED_RAYGEN: may a batch of rt_integrate leave its bounce-0 queue unwritten?  Its bounce-0 closest-hit launch must be one of the k_trace_w4
// instances that have a primary form (the 12-entry stack, plain or loop D: what launch_trace picks under these conditions), and nothing else may read that
// queue: the instrumented instance (rt_frame_debug_timeline) does, and so does k_aov (per_frame: the caller rules it out).  The rays k_trace_w4 hands to
// k_trace2's list are written out by the primary instance itself.
bool primary_fusable(const rt_frame* f)
{
    return f->fused_raygen != 0u && !f->timeline && f->ctx->scene.wide_ok && (f->trace_variant == 5u || f->trace_variant == 10u);
}

// fused: only the prologue runs (one block); the pipe's bounce-0 launches make the rays (intersect_pipe, shade_pipe)
int generate_rays(rt_frame* f, PathPipe& p, uint32_t n_slots, uint32_t chunk_base = 0, bool later_chunk_on_this_pipe = false, bool fused = false)
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
} // namespace

extern "C" {

static int fold_adapt_hook(rt_frame* f);

} // extern "C"

namespace
{
// ---- RT_OPT_FRAME_KERNEL: the stage API's sample as one launch (k_frame) ---------------------------------------------------------
// Can this frame's next sample go through k_frame?  One sample in flight over the whole tile in one chunk on one pipe, the full log layout,
// the wide tree in place, no per-frame feature that reads between the stages, and none of the paths k_frame has no instance for.
bool frame_kernel_eligible(const rt_frame* f)
{
    const rt_ctx* ctx = f->ctx;
    const uint32_t n_local = tile_pixels(f);
    // (fk_auto.frames has been advanced past the frame being started: frame k = frames - 1)
    const int fk = f->fk_auto.frames - 1;
    const bool wanted = f->frame_kernel == 255u ? (f->fk_auto.decided ? f->fk_auto.use_kernel : (!f->fk_auto.skip && (fk == 2 || fk == 3 || (fk >= 4 && (fk & 1))))) : f->frame_kernel != 0u;
    return wanted && f->n_local != 0u && !(f->denoiser || f->aov != 0) && ctx->scene.wide_ok && !ctx->scene.slow_shadow &&
           ctx->scene.d.emissive_nee == 0u && f->log_ovf_blocks == 0u && f->n_pipes == 1u && f->chunk_pixels >= n_local && f->stage_chunks <= 1u &&
           (f->trace_variant == 5u || f->trace_variant == 10u) && !f->profile && !f->timeline && f->select_form_box == 0u && f->max_bounces < 63u;
}

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

int launch_frame_kernel(rt_frame* f)
{
    const bool blue = f->sampler == 1;
    if (f->white_furnace) return blue ? launch_frame_kernel_t<true, true>(f) : launch_frame_kernel_t<true, false>(f);
    return blue ? launch_frame_kernel_t<false, true>(f) : launch_frame_kernel_t<false, false>(f);
}

// ---- the three stages, one pipe's work each: the C entry points run them over the pipes that hold the stage API's sample, rt_integrate and the banks
// (trace_bounces) over the pipe of each chunk ------------------------------------------------------------------------------------------
// IntersectRays: the closest-hit trace of pipe p's ray queue of `bounce`
int intersect_pipe(rt_frame* f, PathPipe& p, uint32_t bounce)
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
int shade_pipe(rt_frame* f, PathPipe& p, uint32_t bounce, bool count_in_ray)
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
int shadow_pipe(rt_frame* f, PathPipe& p, uint32_t bounce)
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

} // namespace

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

#include "samples_ahead_impl.h"

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

int rt_frame_reserve_samples(rt_frame* f, uint32_t n_samples, uint32_t* reserved)
{
    FRAME_PROLOGUE(f, "rt_frame_reserve_samples");
    f->reserved_explicitly = true;                       // (rt_integrate then takes the buffers as they are: no lean growth)
    if (ensure_slots(f, n_samples ? n_samples : 1u) != RT_OK) return RT_ERROR;
    if (reserved) *reserved = f->slots;
    return RT_OK;
}

#include "fold_hooks_impl.h"

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
