// frame_readers.cpp -- the entry points that read a frame without launching a kernel: its radiance to the host or to a device pointer, its kernel spans
// (RT_OPT_PROFILE_KERNELS) and the debug readers of the parity tests -- the ray queues and the hits of the sample in flight, k_frame's per-wave rows, the
// closest-hit trace's launch timeline.  Host code only, on frame.h and context.h: each one first has whatever it is about to read made final by the frames'
// own file (frame::flush_stage, deferred_materialize, join_pipes, sync_frame_streams), then copies.  (What launches a kernel of the hot path's code object
// to read -- rt_frame_resolve, rt_frame_present, rt_frame_get_stats -- is rt_hip.hip's.)
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rt_hip.h"
#include "frame.h"
#include "context.h"
using namespace context;
using namespace frame;

extern "C" {

int rt_frame_read_radiance(rt_frame* f, float* host_rgba)
{
    if (!f || !host_rgba) return fail(nullptr, "rt_frame_read_radiance: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (f->n_local == 0) return RT_OK;
    if (flush_stage(f, true) != RT_OK) return RT_ERROR;
    HIPCHK(ctx, hipMemcpyAsync(host_rgba, f->radiance, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToHost,
        ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

void* rt_frame_radiance_device_ptr(rt_frame* f) { return f ? (void*)f->radiance : nullptr; }
uint32_t rt_frame_sample_count(rt_frame* f) { return f ? f->sample_count : 0; }

int rt_frame_get_profile(rt_frame* f, rt_profile* out)
{
    if (!f || !out) return fail(nullptr, "rt_frame_get_profile: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (join_pipes(f) != RT_OK || sync_frame_streams(f) != RT_OK) return RT_ERROR;   // spans on the side streams end when their launches do
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memset(out, 0, sizeof(*out));
    double* ms[4] = {&out->ms_raygen, &out->ms_trace_closest, &out->ms_shade, &out->ms_trace_shadow};
    uint32_t* cnt[4] = {&out->n_raygen, &out->n_trace_closest, &out->n_shade, &out->n_trace_shadow};
    for (auto& s : f->spans)
    {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) { *ms[s.cls] += t; (*cnt[s.cls])++; }
        f->event_pool.push_back(s.a);
        f->event_pool.push_back(s.b);
    }
    f->spans.clear();
    return RT_OK;
}

int rt_frame_copy_radiance(rt_frame* f, void* device_dst)
{
    if (!f || !device_dst) return fail(nullptr, "rt_frame_copy_radiance: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (f->n_local == 0) return RT_OK;
    if (flush_stage(f, true) != RT_OK) return RT_ERROR;
    HIPCHK(ctx, hipMemcpyAsync(device_dst, f->radiance, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToDevice,
        ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// ---- debug / parity --------------------------------------------------------
int rt_frame_debug_read_queue(rt_frame* f, int which, uint32_t bounce, rt_ray* rays, uint32_t* pixel_indices,
    rt_float4* payload, uint32_t capacity, uint32_t* count)
{
    if (!f || !count) return fail(nullptr, "rt_frame_debug_read_queue: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (bounce > RT_MAX_BOUNCES_LIMIT + 1) return fail(ctx, "rt_frame_debug_read_queue: bounce out of range");
    if (f->stage_chunks > 1) return fail(ctx, "rt_frame_debug_read_queue: the sample in flight is spread over several pipes (set RT_OPT_STAGE_PIPES to 1 for the debug readers)");
    if (f->deferred.active && deferred_materialize(f) != RT_OK) return RT_ERROR;
    const PathPipe& q = f->ps[0];                                          // (one chunk: the sample in flight is on pipe 0)
    if (q.side) HIPCHK(ctx, hipStreamSynchronize(q.side));                 // a shadow trace may be retracting log entries
    DCounters h;
    HIPCHK(ctx, hipMemcpyAsync(&h, q.counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t n = which == 0 ? h.queue[bounce] : h.shadow[bounce];
    if (n > f->log_stride) return fail(ctx, "rt_frame_debug_read_queue: corrupt counter");
    *count = n;
    if (n == 0) return RT_OK;
    if (!rays && !pixel_indices && !payload) return RT_OK;                 // size query (two-call pattern)
    if (n > capacity) return fail(ctx, "rt_frame_debug_read_queue: the queue holds more entries than the caller's arrays");
    const float4* so = which == 0 ? q.o4[bounce & 1u] : q.sh_o4[bounce & 1u];
    const float4* sdir = which == 0 ? q.d4[bounce & 1u] : q.sh_d4[bounce & 1u];
    std::vector<float4> o(n), d(n), p(n);
    HIPCHK(ctx, hipMemcpy(o.data(), so, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(d.data(), sdir, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (which == 0) HIPCHK(ctx, hipMemcpy(p.data(), q.thr[bounce & 1u], (size_t)n * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
    {
        uint32_t pl;
        memcpy(&pl, &d[i].w, 4);
        uint32_t id = pl;
        uint32_t local_pix = q.chunk_base + id % (f->chunk_pixels ? f->chunk_pixels : 1);
        if (which == 1)   // the deferred direct-light sample lives in the radiance log
        {
            uint32_t entry = 0;
            HIPCHK(ctx, hipMemcpy(&entry, q.sh_aux[bounce & 1u] + i, 4, hipMemcpyDeviceToHost));
            p[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t oblk = 0;
            if (entry >= f->log_inline) HIPCHK(ctx, hipMemcpy(&oblk, q.ovf_slot + id, 4, hipMemcpyDeviceToHost));
            const size_t at = entry < f->log_inline ? (size_t)entry * f->log_stride + id
                                                    : (size_t)f->log_inline * f->log_stride + (size_t)(entry - f->log_inline) * f->log_ovf_blocks + oblk;
            HIPCHK(ctx, hipMemcpy(&p[i], q.rlog + 3u * at, 12, hipMemcpyDeviceToHost));
        }
        if (rays)
        {
            rays[i].origin.x = o[i].x; rays[i].origin.y = o[i].y; rays[i].origin.z = o[i].z; rays[i].origin.w = 0.0f;
            rays[i].direction.x = d[i].x; rays[i].direction.y = d[i].y; rays[i].direction.z = d[i].z;
            rays[i].direction.w = o[i].w;
        }
        if (pixel_indices)
        {
            uint32_t ly = local_pix / f->tile.width, px = local_pix - ly * f->tile.width;
            pixel_indices[i] = rt_frame_global_row(f, ly) * f->tile.width + px;   // GLOBAL pixel index
        }
        if (payload) { payload[i].x = p[i].x; payload[i].y = p[i].y; payload[i].z = p[i].z; payload[i].w = 0.0f; }
    }
    return RT_OK;
}

int rt_frame_debug_read_hits(rt_frame* f, rt_hit* hits, uint32_t count)
{
    if (!f || !hits) return fail(nullptr, "rt_frame_debug_read_hits: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (count > f->log_stride) return fail(ctx, "rt_frame_debug_read_hits: count too large");
    if (f->stage_chunks > 1) return fail(ctx, "rt_frame_debug_read_hits: the sample in flight is spread over several pipes (set RT_OPT_STAGE_PIPES to 1 for the debug readers)");
    if (f->deferred.active && deferred_materialize(f) != RT_OK) return RT_ERROR;
    std::vector<float4> h(count ? count : 1);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(h.data(), f->ps[0].hits, (size_t)count * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < count; ++i)
    {
        hits[i].bc.x = h[i].x; hits[i].bc.y = h[i].y;
        memcpy(&hits[i].primitive_id, &h[i].z, 4);
        hits[i].t = h[i].w;
    }
    return RT_OK;
}

// Debug: launch timeline of the closest-hit wide-tree kernel.  arm = 1 clears the slots and starts recording
// (pipe 0); arm = 0 reads them: out[b] = {first wave started, first wave found the queue dry, last wave left} of the
// most recent bounce-b launch, in ticks of the 100 MHz wall clock (0 where nothing ran), then the most traversal steps
// any ray took and the slowest ray's ticks from hand-out to retirement and its steps; after those 64 x 6 values, out[384 + i] =
// waves (of all recorded launches) that left in the i-th 25 us after their launch's queue ran dry.
// k_frame's per-wave rows of its latest launch (RT_FRAME_COUNT_STRIDE words each; frame_kernels.h): rays per bounce and the wave's ticks per phase
int rt_frame_debug_frame_rows(rt_frame* f, uint32_t* out, uint32_t capacity_rows, uint32_t* n_rows, uint32_t* row_words)
{
    if (!f || !n_rows || !row_words) return fail(nullptr, "rt_frame_debug_frame_rows: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    *n_rows = f->kf.blocks; *row_words = RT_FRAME_COUNT_STRIDE;
    if (!out || f->kf.blocks == 0u || !f->kf.counts) return RT_OK;
    if (capacity_rows < f->kf.blocks) return fail(ctx, "rt_frame_debug_frame_rows: the caller's array is too small");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, f->kf.counts, (size_t)f->kf.blocks * RT_FRAME_COUNT_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_frame_debug_timeline(rt_frame* f, int arm, unsigned long long* out /* [64][6] + [64] when reading */)
{
    if (!f) return fail(nullptr, "rt_frame_debug_timeline: frame is NULL");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (join_pipes(f) != RT_OK) return RT_ERROR;
    DCounters* c = f->ps[0].counters;
    if (arm)
    {
        HIPCHK(ctx, hipMemsetAsync(c->tl_start, 0xFF, sizeof(c->tl_start) + sizeof(c->tl_dry), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(c->tl_end, 0, sizeof(c->tl_end) + sizeof(c->tl_ray_steps) + sizeof(c->tl_ray_ticks) + sizeof(c->tl_exit_hist),
            ctx->stream));
        f->timeline = 1;
        return RT_OK;
    }
    if (!out) return fail(ctx, "rt_frame_debug_timeline: NULL output");
    f->timeline = 0;
    std::vector<unsigned long long> h(384);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), c->tl_start, 384 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < 64; ++b)
    {
        bool ran = h[128 + b] != 0ull;
        out[b * 6 + 0] = ran ? h[b] : 0ull;
        out[b * 6 + 1] = ran && h[64 + b] != ~0ull ? h[64 + b] : 0ull;
        out[b * 6 + 2] = h[128 + b];
        out[b * 6 + 3] = h[192 + b];                    // most steps any ray took
        out[b * 6 + 4] = h[256 + b] >> 24;              // the slowest ray: ticks from hand-out to retirement ...
        out[b * 6 + 5] = h[256 + b] & 0xFFFFFFull;      // ... and its steps
    }
    for (int b = 0; b < 64; ++b) out[384 + b] = h[320 + b];   // waves that left in the b-th 25 us after the queue ran dry
    return RT_OK;
}

} // extern "C"
