// context.cpp -- the context and the buffers behind the C-ABI's opaque rt_ctx and rt_buffer: the one place a message is stored (context::fail, the thread's
// message, rt_last_error), the device copies of an upload, the queries' status word, quiesce, a context's creation, destruction and options, page-locked host
// memory, the blue-noise tables, and every rt_buffer_* entry.  Host code only, on context.h; frame.h for what rt_finish and quiesce do to the frames alive on
// a context, frame_launch.h for the one launch a new context makes (context::fill_gamma_lut, rt_hip.hip's).  Replaces the reference's
// src/gpu_wrappers/cl_context.cpp.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "context.h"         // Scene, rt_ctx, rt_buffer, fail / HIPCHK
#include "frame.h"           // the frames alive on a context: ahead_owner, frame::ahead_discard, frame::sync_frame_streams
#include "frame_launch.h"    // context::fill_gamma_lut
#include "fold_adapt.h"      // fold_adapt_set_wait, fold_adapt_set_interval (scene_upload.cpp)
using namespace context;
using namespace frame;

// context.h's functions: the one place a message is stored, the device copies of an upload, the queries' status word
namespace context
{
thread_local std::string g_thread_error;

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
    fill_gamma_lut(ctx);
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
