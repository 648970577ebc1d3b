// frame_filters.cpp -- the spatial and the temporal filter's entry points on a frame and on caller arrays (spatial_filter.h and temporal_filter.h state the
// filters; their kernels, launch drivers and host restatements are filters.hip's, behind filters_host.h): rt_frame_filter, rt_frame_read_guides,
// rt_frame_filter_temporal, rt_frame_filter_history_reset, rt_frame_read_filter_history, rt_frame_read_guide_motion and the rt_debug_filter*,
// rt_debug_guide_motion forms, with the three states a filtered frame keeps.  Host code only, on frame.h and context.h: a filter reads the frame's radiance,
// camera and tile and writes f->resolved, on the context's stream, after the frame's own work has been flushed (frame::flush_stage).  The one launch it needs
// of the hot path's code object -- the guide pass's closest-hit trace -- is rt_hip.hip's frame::trace_guides.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "frame.h"
#include "context.h"
#include "filters_host.h"    // the guide pass, the a-trous passes, the temporal stages and their host restatements (filters.hip)
#include "device_memory.h"   // dev::Temps, for the debug forms' images
#include "rt_detmath.h"      // rt_tanf
using namespace context;
using namespace frame;

// The spatial filter's state on a frame (rt_frame_filter, rt_frame_read_guides): made on first use, freed by rt_frame_destroy.  Its own rays, hits,
// counter and spill area: batches traced ahead (RT_OPT_SAMPLES_AHEAD) may be using the frame's per-path buffers on other streams.  After the guide
// pass o4 / d4 are free again and serve as the a-trous passes' two ping-pong images.  80 bytes per pixel + the spill area.
struct SfGuides
{
    float4* o4 = nullptr; float4* d4 = nullptr; float4* hits = nullptr;
    float4* alb = nullptr; float4* nz = nullptr;       // the guides: albedo (w 0); unit normal + depth
    uint32_t* count = nullptr;
    uint2* spill = nullptr;
    rt_camera camera;                                  // what the guides were made for
    uint64_t scene = 0;
    bool valid = false;
    uint32_t passes = 0;                               // guide passes so far
    std::vector<DevBuf> buffers(size_t n = 0, size_t spill_bytes = 0)
    {
        const size_t b = n * sizeof(float4);
        return {{(void**)&o4, b}, {(void**)&d4, b}, {(void**)&hits, b}, {(void**)&alb, b}, {(void**)&nz, b}, {(void**)&count, sizeof(uint32_t)},
                {(void**)&spill, spill_bytes}};
    }
};

// The temporal filter's history on a frame (rt_frame_filter_temporal): made on first use, freed by rt_frame_destroy.  64 bytes per pixel: the colour
// history, two moments images (mu1, mu2, L) -- the accumulation reads one and writes the other, which is then the history -- and the previous call's
// normal + depth guide, copied after each call (the guide pass overwrites its own for a new camera).  Its scratch images are the spatial filter's o4 / d4.
struct TfState
{
    float4* hist = nullptr;
    float4* mom[2] = {nullptr, nullptr};
    float4* prev_nz = nullptr;
    uint32_t cur = 0;                                  // mom[cur] is the history
    rt_camera prev_cam;                                // the previous call's camera and scene (rt_scene_upload count; upload epoch and refit index)
    uint64_t prev_scene = 0;
    uint64_t prev_epoch = 0, prev_refit = 0;
    bool has_prev = false;                             // false: no call yet, or the history was dropped
    std::vector<DevBuf> buffers(size_t n = 0)
    {
        const size_t b = n * sizeof(float4);
        return {{(void**)&hist, b}, {(void**)&mom[0], b}, {(void**)&mom[1], b}, {(void**)&prev_nz, b}};
    }
};

// RT_CTX_OPT_REFIT_MOTION on a frame (rt_frame_filter_temporal after a refit, rt_frame_read_guide_motion): per pixel where its first hit was in the pose
// before the last refit and its normal there (filt::guide_motion over the guide pass's hits).  32 bytes per pixel, made on first use on a context that keeps
// a pose, freed by rt_frame_destroy.
struct SfMotion
{
    float4* prev_pos = nullptr; float4* prev_n = nullptr;
    rt_camera camera;                                  // what the images were made for
    uint64_t scene = 0;
    bool valid = false;
    std::vector<DevBuf> buffers(size_t n = 0)
    {
        const size_t b = n * sizeof(float4);
        return {{(void**)&prev_pos, b}, {(void**)&prev_n, b}};
    }
};

// rt_frame_destroy's part here: the filters' states
void frame::free_filter_state(rt_frame* f)
{
    free_state(f->sf);
    free_state(f->tf);
    free_state(f->sm);
}

// ---- the spatial and temporal filters (spatial_filter.h and temporal_filter.h state them; the kernels live in filters.hip)
// the checks both filters' descriptors share: iterations, flags, (the temporal filter's alphas,) three sigmas > 0 and finite
static int check_desc(rt_ctx* ctx, const char* who, uint32_t iterations, uint32_t flags, const float (&sigmas)[3], const char* sigma_names,
    bool alphas_ok = true)
{
    if (iterations > RT_FILTER_MAX_ITERATIONS) return fail(ctx, std::string(who) + ": iterations must be 0 .. 8");
    if (flags & ~RT_FILTER_DEMODULATE) return fail(ctx, std::string(who) + ": unknown flags (RT_FILTER_DEMODULATE is the only one)");
    if (!alphas_ok) return fail(ctx, std::string(who) + ": alpha_color and alpha_moments must be in 0 .. 1");
    for (float v : sigmas)
        if (!(v > 0.0f) || !std::isfinite(v)) return fail(ctx, std::string(who) + ": " + sigma_names + " must be > 0 and finite");
    return RT_OK;
}

static int check_filter_desc(rt_ctx* ctx, const char* who, const rt_filter_desc* d)
{
    return check_desc(ctx, who, d->iterations, d->flags, {d->sigma_color, d->sigma_normal, d->sigma_depth}, "sigma_color, sigma_normal and sigma_depth");
}

static int check_temporal_desc(rt_ctx* ctx, const char* who, const rt_temporal_filter_desc* d)
{
    const bool alphas_ok = d->alpha_color >= 0.0f && d->alpha_color <= 1.0f && d->alpha_moments >= 0.0f && d->alpha_moments <= 1.0f;
    return check_desc(ctx, who, d->iterations, d->flags, {d->sigma_luminance, d->sigma_normal, d->sigma_depth},
                      "sigma_luminance, sigma_normal and sigma_depth", alphas_ok);
}

static int check_filter_frame(rt_frame* f, const char* who)
{
    if (f->tile.nranks > 1) return fail(f->ctx, std::string(who) + ": a tile frame (tile_count > 1): the filter's stencil crosses rows, it needs the whole image");
    return RT_OK;
}

// the guides for the frame's current camera: one pixel-centre ray per pixel, traced by k_trace_v1<false> (the reference's BVH2 walk) on the context's
// stream with the filter's own buffers, then k_aov's formulas.  Recomputed when the camera or the scene (rt_scene_upload) has changed since.
static int ensure_guides(rt_frame* f, const char* who)
{
    rt_ctx* ctx = f->ctx;
    if (!ctx->scene.valid) return fail(ctx, std::string(who) + ": no scene uploaded");
    const size_t n = f->n_local;
    if (!f->sf)
    {
        const size_t spill_bytes = (size_t)f->trace_blocks * 64u * (RT_TRACE_STACK_MAX - RT_TRACE_STACK_LDS) * sizeof(uint2);
        f->sf = alloc_state<SfGuides>(n, spill_bytes);
        if (!f->sf) return fail(ctx, std::string(who) + ": out of device memory for the guide pass (80 bytes per pixel)");
    }
    SfGuides* g = f->sf;
    if (g->valid && g->scene == ctx->scene_uploads && memcmp(&g->camera, &f->camera, sizeof(rt_camera)) == 0) return RT_OK;
    g->valid = false;
    HIPCHK(ctx, filt::guide_rays(ctx->stream, f->tile.width, f->tile.height, f->camera, rt_tanf(0.5f * f->camera.fov), g->o4, g->d4));
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)g->count, (int)n, 1, ctx->stream));
    trace_guides(f, g->o4, g->d4, g->hits, g->spill, g->count, n);      // the closest-hit trace: a launch of the hot path's code object (rt_hip.hip)
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, filt::guide_values(ctx->stream, ctx->scene.d, g->o4, g->hits, (uint32_t)n, g->alb, g->nz));
    g->camera = f->camera;
    g->scene = ctx->scene_uploads;
    g->valid = true;
    ++g->passes;
    return RT_OK;
}

// RT_CTX_OPT_REFIT_MOTION: the frame's motion images for its current camera and the context's current snapshot (which must exist); the guides first
static int ensure_motion(rt_frame* f, const char* who)
{
    rt_ctx* ctx = f->ctx;
    if (ensure_guides(f, who) != RT_OK) return RT_ERROR;
    const size_t n = f->n_local;
    if (!f->sm)
    {
        f->sm = alloc_state<SfMotion>(n);
        if (!f->sm) return fail(ctx, std::string(who) + ": out of device memory for the motion images (32 bytes per pixel)");
    }
    SfMotion* m = f->sm;
    if (m->valid && m->scene == ctx->scene_uploads && memcmp(&m->camera, &f->camera, sizeof(rt_camera)) == 0) return RT_OK;
    m->valid = false;
    HIPCHK(ctx, filt::guide_motion(ctx->stream, (const float4*)ctx->scene.pose_snap, ctx->scene.n_tris, f->sf->hits, (uint32_t)n, m->prev_pos, m->prev_n));
    m->camera = f->camera;
    m->scene = ctx->scene_uploads;
    m->valid = true;
    return RT_OK;
}

// the refusals both frame filters share after their descriptor's check: a tile frame, RT_OPT_AOV
static int check_filter_call(rt_frame* f, const char* who)
{
    if (check_filter_frame(f, who) != RT_OK) return RT_ERROR;
    if (f->aov != 0) return fail(f->ctx, std::string(who) + ": RT_OPT_AOV != 0: the filter is for the shaded colour only");
    return RT_OK;
}

// what both frame filters need before their passes: the guides, the frame's own work done, f->resolved free to be the output image (as rt_frame_resolve)
static int filter_inputs_ready(rt_frame* f, const char* who)
{
    if (ensure_guides(f, who) != RT_OK || rt_frame_present_wait(f) != RT_OK || flush_stage(f) != RT_OK) return RT_ERROR;
    return RT_OK;
}

// the frame filters' read-back: the output image f->resolved to the caller
static int read_filtered(rt_frame* f, float* host_rgba)
{
    rt_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipMemcpyAsync(host_rgba, f->resolved, (size_t)f->n_local * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// the debug entry points' guide: normal (xyz) + depth per pixel
static std::vector<float> pack_nz(const float* normal_rgba, const float* depth, size_t n)
{
    std::vector<float> nz(4 * n);
    for (size_t i = 0; i < n; ++i)
    {
        nz[4 * i] = normal_rgba[4 * i]; nz[4 * i + 1] = normal_rgba[4 * i + 1]; nz[4 * i + 2] = normal_rgba[4 * i + 2]; nz[4 * i + 3] = depth[i];
    }
    return nz;
}

// the debug entry points on ctx's device: n_images images of n pixels, the first in.size() uploaded from `in`, run(images), the last out.size()
// downloaded to `out`; every image is freed on every path and a failure is reported as "who: <HIP error>"
template <class F> static int debug_on_device(rt_ctx* ctx, const char* who, size_t n, size_t n_images, std::initializer_list<const void*> in,
    std::initializer_list<void*> out, F&& run)
{
    (void)hipSetDevice(ctx->device);
    dev::Temps tmp(ctx->stream);
    std::vector<float4*> buf(n_images, nullptr);
    const size_t bytes = n * sizeof(float4);
    bool ok = true;
    for (float4*& b : buf) ok = ok && tmp.array(b, n);
    size_t k = 0;
    for (const void* p : in) ok = ok && hipMemcpyAsync(buf[k++], p, bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    hipError_t e = ok ? run(buf.data()) : hipErrorOutOfMemory;
    k = n_images - out.size();
    for (void* p : out) if (e == hipSuccess) e = hipMemcpyAsync(p, buf[k++], bytes, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, std::string(who) + ": " + hipGetErrorString(e)); }
    return RT_OK;
}

extern "C" {

int rt_frame_filter(rt_frame* f, const rt_filter_desc* desc, float* host_rgba)
{
    static const char* who = "rt_frame_filter";
    if (!f || !desc || !host_rgba) return fail(nullptr, "rt_frame_filter: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (check_filter_desc(ctx, who, desc) != RT_OK || check_filter_call(f, who) != RT_OK) return RT_ERROR;
    if (desc->iterations == 0) return rt_frame_resolve(f, host_rgba);      // exactly rt_frame_resolve's image
    if (f->n_local == 0) return RT_OK;
    if (filter_inputs_ready(f, who) != RT_OK) return RT_ERROR;
    SfGuides* g = f->sf;
    const filt::Spatial s = {f->tile.width, f->tile.height, *desc, f->denoiser == 0u, (float)f->sample_count, 1};
    HIPCHK(ctx, filt::spatial(ctx->stream, s, f->radiance, g->alb, g->nz, g->o4, g->d4, f->resolved));
    return read_filtered(f, host_rgba);
}

int rt_frame_read_guides(rt_frame* f, float* albedo_rgba, float* normal_rgba, float* depth, uint32_t* passes)
{
    if (!f) return fail(nullptr, "rt_frame_read_guides: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (check_filter_frame(f, "rt_frame_read_guides") != RT_OK) return RT_ERROR;
    if (f->n_local == 0) { if (passes) *passes = 0; return RT_OK; }
    if (ensure_guides(f, "rt_frame_read_guides") != RT_OK) return RT_ERROR;
    const size_t n = f->n_local;
    if (albedo_rgba) HIPCHK(ctx, hipMemcpyAsync(albedo_rgba, f->sf->alb, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float4> nz((normal_rgba || depth) ? n : 0);
    if (!nz.empty()) HIPCHK(ctx, hipMemcpyAsync(nz.data(), f->sf->nz, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < nz.size(); ++i)
    {
        if (normal_rgba) { normal_rgba[4 * i] = nz[i].x; normal_rgba[4 * i + 1] = nz[i].y; normal_rgba[4 * i + 2] = nz[i].z; normal_rgba[4 * i + 3] = 0.0f; }
        if (depth) depth[i] = nz[i].w;
    }
    if (passes) *passes = f->sf->passes;
    return RT_OK;
}

int rt_debug_filter(rt_ctx* ctx, uint32_t width, uint32_t height, const float* hdr_rgba, const float* albedo_rgba, const float* normal_rgba,
    const float* depth, const rt_filter_desc* desc, float* out_hdr_rgba)
{
    static const char* who = "rt_debug_filter";
    if (!hdr_rgba || !albedo_rgba || !normal_rgba || !depth || !desc || !out_hdr_rgba) return fail(ctx, "rt_debug_filter: NULL argument");
    if (width == 0 || height == 0) return fail(ctx, "rt_debug_filter: empty image");
    if (check_filter_desc(ctx, who, desc) != RT_OK) return RT_ERROR;
    const size_t n = (size_t)width * height;
    if (desc->iterations == 0) { memcpy(out_hdr_rgba, hdr_rgba, n * sizeof(float4)); return RT_OK; }
    const std::vector<float> nz = pack_nz(normal_rgba, depth, n);
    const filt::Spatial s = {width, height, *desc, 0, 1.0f, 0};
    if (!ctx)
    {
        filt::spatial_host(s, hdr_rgba, albedo_rgba, nz.data(), out_hdr_rgba);
        return RT_OK;
    }
    // images: hdr, albedo, nz, ping, pong, out
    return debug_on_device(ctx, who, n, 6, {hdr_rgba, albedo_rgba, nz.data()}, {out_hdr_rgba},
                           [&](float4** b) { return filt::spatial(ctx->stream, s, b[0], b[1], b[2], b[3], b[4], b[5]); });
}

int rt_frame_filter_temporal(rt_frame* f, const rt_temporal_filter_desc* desc, float* host_rgba)
{
    static const char* who = "rt_frame_filter_temporal";
    if (!f || !desc || !host_rgba) return fail(nullptr, "rt_frame_filter_temporal: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (check_temporal_desc(ctx, who, desc) != RT_OK || check_filter_call(f, who) != RT_OK) return RT_ERROR;
    if (f->denoiser != 0)
        return fail(ctx, "rt_frame_filter_temporal: RT_OPT_DENOISER != 0: the frame is already accumulated over time by the reference's denoiser");
    if (f->n_local == 0) return RT_OK;
    const size_t n = f->n_local;
    if (!f->tf)
    {
        TfState* t = alloc_state<TfState>(n);
        if (t && (hipMemsetAsync(t->hist, 0, n * sizeof(float4), ctx->stream) != hipSuccess ||
                  hipMemsetAsync(t->mom[0], 0, n * sizeof(float4), ctx->stream) != hipSuccess))
        {
            (void)hipGetLastError();
            free_state(t);
        }
        if (!t) return fail(ctx, "rt_frame_filter_temporal: out of device memory for the history (64 bytes per pixel)");
        f->tf = t;
    }
    if (filter_inputs_ready(f, who) != RT_OK) return RT_ERROR;
    TfState* t = f->tf;
    SfGuides* g = f->sf;
    filt::Temporal c;
    c.width = f->tile.width; c.height = f->tile.height;
    c.cam = f->camera;
    c.prev = t->has_prev ? t->prev_cam : f->camera;
    // what the history was made for against the scene now: the same upload and pose = as ever; the same upload, one refit on and the context kept the pose
    // that refit replaced = followed through the motion images; anything else (another upload, two refits or more, no pose kept) = dropped
    const bool same_upload = t->has_prev && t->prev_epoch == ctx->upload_epoch;
    const bool follow = same_upload && t->prev_refit + 1u == ctx->refit_index && ctx->scene.pose_snap && ctx->scene.pose_valid;
    if (follow && ensure_motion(f, who) != RT_OK) return RT_ERROR;
    c.mode = follow ? filt::REPROJECT
           : !same_upload || t->prev_refit != ctx->refit_index ? filt::NO_HISTORY
           : memcmp(&t->prev_cam, &f->camera, sizeof(rt_camera)) == 0 ? filt::IDENTITY : filt::REPROJECT;
    c.desc = *desc;
    c.divide = 1; c.spp = (float)f->sample_count; c.tonemap = 1;
    HIPCHK(ctx, filt::temporal(ctx->stream, c, f->radiance, g->alb, g->nz, t->prev_nz, t->hist, t->mom[t->cur], t->hist, t->mom[t->cur ^ 1u], g->o4,
        g->d4, f->resolved, follow ? f->sm->prev_pos : nullptr, follow ? f->sm->prev_n : nullptr));
    t->cur ^= 1u;
    HIPCHK(ctx, hipMemcpyAsync(t->prev_nz, g->nz, n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    t->prev_cam = f->camera;
    t->prev_scene = ctx->scene_uploads;
    t->prev_epoch = ctx->upload_epoch; t->prev_refit = ctx->refit_index;
    t->has_prev = true;
    return read_filtered(f, host_rgba);
}

int rt_frame_filter_history_reset(rt_frame* f)
{
    if (!f) return fail(nullptr, "rt_frame_filter_history_reset: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (!f->tf) return RT_OK;
    f->tf->has_prev = false;
    HIPCHK(ctx, hipMemsetAsync(f->tf->hist, 0, (size_t)f->n_local * sizeof(float4), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(f->tf->mom[f->tf->cur], 0, (size_t)f->n_local * sizeof(float4), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_frame_read_filter_history(rt_frame* f, float* color_rgba, float* moments_len)
{
    if (!f) return fail(nullptr, "rt_frame_read_filter_history: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (check_filter_frame(f, "rt_frame_read_filter_history") != RT_OK) return RT_ERROR;
    const size_t n = f->n_local;
    if (!f->tf)
    {
        if (color_rgba) memset(color_rgba, 0, n * sizeof(float4));
        if (moments_len) memset(moments_len, 0, n * sizeof(float4));
        return RT_OK;
    }
    if (color_rgba) HIPCHK(ctx, hipMemcpyAsync(color_rgba, f->tf->hist, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (moments_len) HIPCHK(ctx, hipMemcpyAsync(moments_len, f->tf->mom[f->tf->cur], n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_frame_read_guide_motion(rt_frame* f, float* prev_position_rgba, float* prev_normal_rgba)
{
    static const char* who = "rt_frame_read_guide_motion";
    if (!f) return fail(nullptr, "rt_frame_read_guide_motion: NULL argument");
    rt_ctx* ctx = f->ctx;
    (void)hipSetDevice(ctx->device);
    if (check_filter_frame(f, who) != RT_OK) return RT_ERROR;
    const size_t n = f->n_local;
    if (n == 0) return RT_OK;
    if (!ctx->scene.valid || !ctx->scene.pose_snap || !ctx->scene.pose_valid)           // no snapshot: no motion known anywhere
    {
        if (prev_position_rgba) memset(prev_position_rgba, 0, n * sizeof(float4));
        if (prev_normal_rgba) memset(prev_normal_rgba, 0, n * sizeof(float4));
        return RT_OK;
    }
    if (ensure_motion(f, who) != RT_OK) return RT_ERROR;
    if (prev_position_rgba) HIPCHK(ctx, hipMemcpyAsync(prev_position_rgba, f->sm->prev_pos, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (prev_normal_rgba) HIPCHK(ctx, hipMemcpyAsync(prev_normal_rgba, f->sm->prev_n, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_guide_motion(rt_ctx* ctx, uint32_t n, const float* hits, const rt_triangle* prev_triangles, uint32_t num_triangles, float* out_position_rgba,
    float* out_normal_rgba)
{
    if (!hits || (!prev_triangles && num_triangles) || !out_position_rgba || !out_normal_rgba) return fail(ctx, "rt_debug_guide_motion: NULL argument");
    if (n == 0) return RT_OK;
    const std::vector<float> records = filt::pose_records(prev_triangles, num_triangles);
    if (!ctx)
    {
        filt::guide_motion_host(records.data(), num_triangles, hits, n, out_position_rgba, out_normal_rgba);
        return RT_OK;
    }
    (void)hipSetDevice(ctx->device);
    const hipError_t e = filt::guide_motion_device(ctx->stream, records.data(), num_triangles, hits, n, out_position_rgba, out_normal_rgba);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, std::string("rt_debug_guide_motion: ") + hipGetErrorString(e)); }
    return RT_OK;
}

int rt_debug_filter_temporal(rt_ctx* ctx, uint32_t width, uint32_t height, const rt_camera* cam, const rt_camera* prev_cam, const float* hdr_rgba,
    const float* albedo_rgba, const float* normal_rgba, const float* depth, const float* prev_normal_rgba, const float* prev_depth,
    const float* hist_color, const float* hist_moments, const rt_temporal_filter_desc* desc, float* out_hdr_rgba, float* hist_color_out,
    float* hist_moments_out)
{
    return rt_debug_filter_temporal_motion(ctx, width, height, cam, prev_cam, hdr_rgba, albedo_rgba, normal_rgba, depth, prev_normal_rgba, prev_depth, hist_color,
        hist_moments, nullptr, nullptr, desc, out_hdr_rgba, hist_color_out, hist_moments_out);
}

int rt_debug_filter_temporal_motion(rt_ctx* ctx, uint32_t width, uint32_t height, const rt_camera* cam, const rt_camera* prev_cam, const float* hdr_rgba,
    const float* albedo_rgba, const float* normal_rgba, const float* depth, const float* prev_normal_rgba, const float* prev_depth,
    const float* hist_color, const float* hist_moments, const float* prev_position_rgba, const float* prev_pose_normal_rgba,
    const rt_temporal_filter_desc* desc, float* out_hdr_rgba, float* hist_color_out, float* hist_moments_out)
{
    // (the messages name rt_debug_filter_temporal, the family: the entry without motion images is this one with two NULLs)
    static const char* who = "rt_debug_filter_temporal";
    if (!cam || !hdr_rgba || !albedo_rgba || !normal_rgba || !depth || !prev_normal_rgba || !prev_depth || !hist_color || !hist_moments || !desc ||
        !out_hdr_rgba || !hist_color_out || !hist_moments_out)
        return fail(ctx, "rt_debug_filter_temporal: NULL argument");
    if (width == 0 || height == 0) return fail(ctx, "rt_debug_filter_temporal: empty image");
    const bool motion = prev_position_rgba && prev_pose_normal_rgba;
    if (check_temporal_desc(ctx, who, desc) != RT_OK) return RT_ERROR;
    const size_t n = (size_t)width * height;
    const std::vector<float> nz = pack_nz(normal_rgba, depth, n), pnz = pack_nz(prev_normal_rgba, prev_depth, n);
    filt::Temporal c;
    c.width = width; c.height = height;
    c.cam = *cam;
    c.prev = prev_cam ? *prev_cam : *cam;
    c.mode = !motion && (!prev_cam || memcmp(prev_cam, cam, sizeof(rt_camera)) == 0) ? filt::IDENTITY : filt::REPROJECT;
    c.desc = *desc;
    c.divide = 0; c.spp = 1.0f; c.tonemap = 0;
    if (!ctx)
    {
        filt::temporal_host(c, hdr_rgba, albedo_rgba, nz.data(), pnz.data(), hist_color, hist_moments, hist_color_out, hist_moments_out, out_hdr_rgba,
            motion ? prev_position_rgba : nullptr, motion ? prev_pose_normal_rgba : nullptr);
        return RT_OK;
    }
    // with motion images: hdr, albedo, nz, prev nz, hist in, moments in, prev position, prev pose normal, a, b, out, hist out, moments out
    if (motion)
        return debug_on_device(ctx, who, n, 13, {hdr_rgba, albedo_rgba, nz.data(), pnz.data(), hist_color, hist_moments, prev_position_rgba, prev_pose_normal_rgba},
                               {out_hdr_rgba, hist_color_out, hist_moments_out},
                               [&](float4** b) { return filt::temporal(ctx->stream, c, b[0], b[1], b[2], b[3], b[4], b[5], b[11], b[12], b[8], b[9], b[10], b[6], b[7]); });
    // images: hdr, albedo, nz, prev nz, hist in, moments in, a, b, out, hist out, moments out
    return debug_on_device(ctx, who, n, 11, {hdr_rgba, albedo_rgba, nz.data(), pnz.data(), hist_color, hist_moments},
                           {out_hdr_rgba, hist_color_out, hist_moments_out},
                           [&](float4** b) { return filt::temporal(ctx->stream, c, b[0], b[1], b[2], b[3], b[4], b[5], b[9], b[10], b[6], b[7], b[8]); });
}

} // extern "C"
