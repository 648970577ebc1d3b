// scene_queries.cpp -- the C entry points of the eight query families on an uploaded scene, the bookkeeping around the kernels and launch drivers of
// query.hip, bake.hip, nearest.hip, all_hits.hip, within.hip, region.hip, cross.hip and separation.hip (DESIGN.md sections 7h - 7o): rt_scene_trace*, rt_scene_bake*,
// rt_scene_nearest*, rt_scene_trace_all*, rt_scene_within*, rt_scene_overlap*, rt_scene_select*, rt_scene_cross*, rt_scene_separation* and their rt_debug_* forms.  Host code only, on context.h:
// a query reads the scene and writes the caller's arrays, it launches on the context's stream -- behind every refit, pose and upload, which end there --
// and touches no frame.  (The three picks read a frame's camera and tile: they are frame_layout.cpp's and call the entries here.)  The stack spill area, the
// status word and the staging arrays of every family but the bakes are the ray queries' (ctx->query), so rt_scene_tree_report's "ray queries" line
// counts them; the bakes have a scratch of their own (ctx->bake).  The tree-less UV atlas (atlas.hip, section 7r: rt_scene_atlas*, rt_scene_atlas_surfaces*,
// rt_scene_atlas_bake, rt_debug_atlas) has its entry points here too and works in the bakes' scratch, and so do the light bakes (light_bake.hip, section 7s:
// rt_scene_light_bake*, rt_scene_atlas_bake_light, rt_debug_light_bake_*).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <functional>
#include <initializer_list>
#include <string>
#include "rt_hip.h"
#include "context.h"
#include "query_host.h"
#include "bake_host.h"
#include "light_bake_host.h"
#include "light_bake.h"
#include "nearest_host.h"
#include "all_hits_host.h"
#include "within_host.h"
#include "region_host.h"
#include "cross_host.h"
#include "cross.h"
#include "separation_host.h"
#include "separation.h"
#include "atlas_host.h"
#include "atlas.h"
#include "device_memory.h"
using namespace context;

// ---- what the families share ---------------------------------------------------------------------------------------------------------------------------

// How every scene form opens: a context, the arrays it asks for before it looks at the scene, a scene, the arrays it asks for after.  (Which array comes
// before the scene differs by family and is part of each one's contract: a caller sees the first refusal only.)
struct Needed { const char* what; bool given; };
static int opening_refused(rt_ctx* ctx, const std::string& name, std::initializer_list<Needed> before_scene, std::initializer_list<Needed> after_scene)
{
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    for (const Needed& a : before_scene) if (!a.given) return fail(ctx, name + ": " + a.what + " is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    for (const Needed& a : after_scene) if (!a.given) return fail(ctx, name + ": " + a.what + " is NULL");
    return RT_OK;
}

// One array of a host form's call: `host` is the caller's (NULL: not asked for), staged through stage[stage] of the scratch, up before the launch or down after it.
struct StagedArray { void* host; size_t record; int stage; bool up; };

// A host form's loop, shared by every family's: at most `chunk` records at a time are staged -- reserve, copy up, launch(first, m) on the staged arrays,
// copy down, wait for the stream, read the walk's status word.
static int staged_call(rt_ctx* ctx, const char* who, query::Scratch& s, std::initializer_list<StagedArray> arrays, uint32_t n, uint32_t chunk,
    const std::function<int(uint32_t first, uint32_t m)>& launch)
{
    for (uint32_t first = 0; first < n; )
    {
        const uint32_t m = n - first < chunk ? n - first : chunk;
        for (const StagedArray& a : arrays)
            if (a.host && !query::reserve(ctx->stream, s, a.stage, (size_t)m * a.record)) return fail(ctx, std::string(who) + ": out of device memory for the staging arrays");
        for (const StagedArray& a : arrays)
            if (a.host && a.up) HIPCHK(ctx, hipMemcpyAsync(s.stage[a.stage], (const char*)a.host + (size_t)first * a.record, (size_t)m * a.record, hipMemcpyHostToDevice, ctx->stream));
        if (launch(first, m) != RT_OK) return RT_ERROR;
        for (const StagedArray& a : arrays)
            if (a.host && !a.up) HIPCHK(ctx, hipMemcpyAsync((char*)a.host + (size_t)first * a.record, s.stage[a.stage], (size_t)m * a.record, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (query_check_status(ctx, who) != RT_OK) return RT_ERROR;
        first += m;
    }
    return RT_OK;
}

// what a buffer form refuses of its buffers (NULL: not passed)
struct BufferArg { rt_buffer* b; size_t record; const char* what; };
static int buffers_refused(rt_ctx* ctx, const char* who, std::initializer_list<BufferArg> bufs, uint32_t n)
{
    for (const BufferArg& b : bufs)
    {
        if (!b.b) continue;
        if (b.b->ctx != ctx) return fail(ctx, std::string(who) + ": the " + b.what + " buffer belongs to another context");
        if (b.b->bytes < (size_t)n * b.record) return fail(ctx, std::string(who) + ": the " + b.what + " buffer is smaller than n records");
    }
    return RT_OK;
}

// a driver's launch() said `ok`; why_not: the message behind `who` when it did not
static int launch_result(rt_ctx* ctx, const char* who, bool ok, const char* why_not)
{
    if (ok) return RT_OK;
    (void)hipGetLastError();
    return fail(ctx, std::string(who) + why_not);
}
static const char QUERY_NOT_LAUNCHED[] = ": the query could not be launched (the stack spill area could not be allocated, or a launch failed)";

// A brute-force debug form's two ways, once its arguments have passed: without a context on_host() computes, with one on_device(stream) does on its device.
template <class Host, class Device> static int host_or_device(rt_ctx* ctx, const char* who, Host on_host, Device on_device)
{
    if (!ctx) { on_host(); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!on_device(ctx->stream)) return fail(ctx, std::string(who) + ": the device path failed (allocation, copy or launch)");
    return RT_OK;
}

// what a walk form says of a `wide` that is neither
static const char WIDE_REFUSED[] = ": wide must be 0 (the child-pair form) or 1 (the 4-wide records)";

extern "C" {

// ---- rays: rt_scene_trace / rt_scene_trace_buffer / rt_debug_query_surface (query.hip) ---------------------------------------------

// everything both forms refuse before anything is launched
static int query_refused(rt_ctx* ctx, const char* who, bool rays, uint32_t n, uint32_t mode, bool hits, bool occluded, bool surfaces)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"rays", rays || n == 0u}}, {}) != RT_OK) return RT_ERROR;
    if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_ANY_HIT) return fail(ctx, name + ": unknown mode (RT_QUERY_CLOSEST or RT_QUERY_ANY_HIT)");
    if (mode == RT_QUERY_CLOSEST && !hits && !occluded && !surfaces) return fail(ctx, name + ": no output (hits, occluded and surfaces are all NULL)");
    if (mode == RT_QUERY_ANY_HIT && (hits || surfaces)) return fail(ctx, name + ": RT_QUERY_ANY_HIT reports no hits or surfaces (which triangle occludes depends on the tree): pass NULL");
    if (mode == RT_QUERY_ANY_HIT && !occluded) return fail(ctx, name + ": no output (occluded is NULL)");
    return RT_OK;
}

static int query_launch(rt_ctx* ctx, const char* who, const rt_ray* d_rays, uint32_t n, uint32_t mode, rt_hit* d_hits, uint32_t* d_occluded, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, query::launch(ctx->stream, ctx->query, s.d, s.wide_ok, s.n_tris, s.pose ? s.pose->ids : nullptr, ctx->prop.multiProcessorCount, d_rays, n,
        mode, d_hits, d_occluded, d_surfaces), QUERY_NOT_LAUNCHED);
}

int rt_scene_trace(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t mode, rt_hit* hits, uint32_t* occluded, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (query_refused(ctx, "rt_scene_trace", rays != nullptr, n, mode, hits != nullptr, occluded != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    return staged_call(ctx, "rt_scene_trace", q, {{(void*)rays, sizeof(rt_ray), 0, true}, {hits, sizeof(rt_hit), 1, false}, {occluded, sizeof(uint32_t), 2, false},
        {surfaces, sizeof(rt_surface), 3, false}}, n, (uint32_t)query::CHUNK_RAYS, [&](uint32_t, uint32_t m)
        {
            return query_launch(ctx, "rt_scene_trace", (const rt_ray*)q.stage[0], m, mode, hits ? (rt_hit*)q.stage[1] : nullptr, occluded ? (uint32_t*)q.stage[2] : nullptr,
                surfaces ? (rt_surface*)q.stage[3] : nullptr);
        });
}

int rt_scene_trace_buffer(rt_ctx* ctx, rt_buffer* rays, uint32_t n, uint32_t mode, rt_buffer* hits, rt_buffer* occluded, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (query_refused(ctx, "rt_scene_trace_buffer", rays != nullptr, n, mode, hits != nullptr, occluded != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_trace_buffer", {{rays, sizeof(rt_ray), "rays"}, {hits, sizeof(rt_hit), "hits"}, {occluded, sizeof(uint32_t), "occluded"},
            {surfaces, sizeof(rt_surface), "surfaces"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return query_launch(ctx, "rt_scene_trace_buffer", (const rt_ray*)rays->ptr, n, mode, hits ? (rt_hit*)hits->ptr : nullptr, occluded ? (uint32_t*)occluded->ptr : nullptr,
        surfaces ? (rt_surface*)surfaces->ptr : nullptr);
}

int rt_debug_query_surface(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits,
    uint32_t n, rt_surface* out)
{
    if (n == 0u) return RT_OK;
    if (!rays || !hits || !out || (!triangles && num_triangles > 0u)) return fail(ctx, "rt_debug_query_surface: NULL argument");
    return host_or_device(ctx, "rt_debug_query_surface", [&] { query::debug_surface_host(triangles, num_triangles, object_of_triangle, rays, hits, n, out); },
        [&](hipStream_t st) { return query::debug_surface_device(st, triangles, num_triangles, object_of_triangle, rays, hits, n, out); });
}

// ---- bakes: rt_scene_bake / rt_scene_bake_buffer / rt_debug_bake_rays / rt_debug_bake_reduce (bake.hip) ----------------------------

// everything both forms refuse before anything is launched
static int bake_refused(rt_ctx* ctx, const char* who, bool points, uint32_t n, const rt_bake_desc* desc, bool out)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"points", points}, {"desc", desc != nullptr}, {"out", out}}, {}) != RT_OK) return RT_ERROR;
    if (const char* why = bake::desc_refusal(*desc)) return fail(ctx, name + ": " + why);
    return RT_OK;
}

static int bake_launch(rt_ctx* ctx, const char* who, const void* d_points, uint32_t n, uint32_t first_index, const rt_bake_desc& desc, rt_bake_result* d_out)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, bake::launch(ctx->stream, ctx->bake, &ctx->query.status, s.d, s.wide_ok, ctx->prop.multiProcessorCount, d_points, n, first_index, desc, d_out),
        ": the bake could not be launched (the stack spill area could not be allocated, or the launch failed)");
}

int rt_scene_bake(rt_ctx* ctx, const void* points, uint32_t n, const rt_bake_desc* desc, rt_bake_result* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (bake_refused(ctx, "rt_scene_bake", points != nullptr, n, desc, out != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& b = ctx->bake;
    return staged_call(ctx, "rt_scene_bake", b, {{(void*)points, bake::point_bytes(*desc), 0, true}, {out, sizeof(rt_bake_result), 1, false}}, n, ctx->bake_chunk_points,
        [&](uint32_t first, uint32_t m) { return bake_launch(ctx, "rt_scene_bake", b.stage[0], m, first, *desc, (rt_bake_result*)b.stage[1]); });
}

int rt_scene_bake_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, const rt_bake_desc* desc, rt_buffer* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (bake_refused(ctx, "rt_scene_bake_buffer", points != nullptr, n, desc, out != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_bake_buffer", {{points, bake::point_bytes(*desc), "points"}, {out, sizeof(rt_bake_result), "out"}}, n) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return bake_launch(ctx, "rt_scene_bake_buffer", points->ptr, n, 0u, *desc, (rt_bake_result*)out->ptr);
}

int rt_debug_bake_rays(rt_ctx* ctx, const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc* desc, rt_ray* rays_out)
{
    if (n == 0u) return RT_OK;
    if (!points || !desc || !rays_out) return fail(ctx, "rt_debug_bake_rays: NULL argument");
    if (const char* why = bake::desc_refusal(*desc)) return fail(ctx, std::string("rt_debug_bake_rays: ") + why);
    if ((uint64_t)n * desc->samples > (1ull << 28)) return fail(ctx, "rt_debug_bake_rays: more than 2^28 rays");
    return host_or_device(ctx, "rt_debug_bake_rays", [&] { bake::debug_rays_host(points, n, first_index, *desc, rays_out); },
        [&](hipStream_t st) { return bake::debug_rays_device(st, points, n, first_index, *desc, rays_out); });
}

int rt_debug_bake_reduce(const rt_ray* rays, const uint32_t* occluded, uint32_t n, uint32_t samples, rt_bake_result* out)
{
    if (n == 0u) return RT_OK;
    if (!rays || !occluded || !out) return fail(nullptr, "rt_debug_bake_reduce: NULL argument");
    if (samples < 16u || samples > 4096u || (samples & (samples - 1u)) != 0u) return fail(nullptr, "rt_debug_bake_reduce: samples must be a power of two in 16 .. 4096");
    bake::debug_reduce_host(rays, occluded, n, samples, out);
    return RT_OK;
}

// ---- light bakes: rt_scene_light_bake / rt_scene_light_bake_buffer / rt_debug_light_bake_rays / rt_debug_light_bake_reduce (light_bake.hip, DESIGN.md
// section 7s; rt_scene_atlas_bake_light is with the atlas below).  They work in the bakes' scratch, as the occlusion bakes do ----------------------------

// everything both forms refuse before anything is launched
static int light_bake_refused(rt_ctx* ctx, const char* who, bool points, const rt_light_bake_desc* desc, bool out)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"points", points}, {"desc", desc != nullptr}, {"out", out}}, {}) != RT_OK) return RT_ERROR;
    if (const char* why = light_bake::desc_refusal(*desc)) return fail(ctx, name + ": " + why);
    return RT_OK;
}

static int light_bake_launch(rt_ctx* ctx, const char* who, const void* d_points, uint32_t n, uint32_t first_index, const rt_light_bake_desc& desc, rt_light_bake_result* d_out)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, light_bake::launch(ctx->stream, ctx->bake, &ctx->query.status, s.d, s.wide_ok, ctx->prop.multiProcessorCount, d_points, n, first_index,
        desc, d_out), ": the bake could not be launched (the stack spill area could not be allocated, or the launch failed)");
}

int rt_scene_light_bake(rt_ctx* ctx, const void* points, uint32_t n, const rt_light_bake_desc* desc, rt_light_bake_result* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (light_bake_refused(ctx, "rt_scene_light_bake", points != nullptr, desc, out != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& b = ctx->bake;
    return staged_call(ctx, "rt_scene_light_bake", b, {{(void*)points, light_bake::point_bytes(*desc), 0, true}, {out, sizeof(rt_light_bake_result), 1, false}}, n,
        ctx->bake_chunk_points, [&](uint32_t first, uint32_t m) { return light_bake_launch(ctx, "rt_scene_light_bake", b.stage[0], m, first, *desc, (rt_light_bake_result*)b.stage[1]); });
}

int rt_scene_light_bake_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, const rt_light_bake_desc* desc, rt_buffer* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (light_bake_refused(ctx, "rt_scene_light_bake_buffer", points != nullptr, desc, out != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_light_bake_buffer", {{points, light_bake::point_bytes(*desc), "points"}, {out, sizeof(rt_light_bake_result), "out"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return light_bake_launch(ctx, "rt_scene_light_bake_buffer", points->ptr, n, 0u, *desc, (rt_light_bake_result*)out->ptr);
}

int rt_debug_light_bake_rays(rt_ctx* ctx, const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc* desc, const rt_light* lights,
    uint32_t num_lights, rt_ray* rays_out)
{
    if (n == 0u) return RT_OK;
    if (!points || !desc || !rays_out || (!lights && num_lights > 0u)) return fail(ctx, "rt_debug_light_bake_rays: NULL argument");
    if (const char* why = light_bake::desc_refusal(*desc)) return fail(ctx, std::string("rt_debug_light_bake_rays: ") + why);
    if ((uint64_t)n * ((uint64_t)desc->samples + num_lights) > (1ull << 28)) return fail(ctx, "rt_debug_light_bake_rays: more than 2^28 rays");
    return host_or_device(ctx, "rt_debug_light_bake_rays", [&] { light_bake::debug_rays_host(points, n, first_index, *desc, lights, num_lights, rays_out); },
        [&](hipStream_t st) { return light_bake::debug_rays_device(st, points, n, first_index, *desc, lights, num_lights, rays_out); });
}

int rt_debug_light_bake_reduce(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc* desc, const rt_light* lights, uint32_t num_lights,
    const float* env_rgba, uint32_t env_w, uint32_t env_h, const uint32_t* occluded, rt_light_bake_result* out)
{
    if (n == 0u) return RT_OK;
    if (!points || !desc || !occluded || !out || (!lights && num_lights > 0u)) return fail(nullptr, "rt_debug_light_bake_reduce: NULL argument");
    if (const char* why = light_bake::desc_refusal(*desc)) return fail(nullptr, std::string("rt_debug_light_bake_reduce: ") + why);
    if (!(desc->flags & RT_LIGHT_BAKE_NO_SKY) && (!env_rgba || env_w == 0u || env_h == 0u || env_w > 0x7FFFFFFFu || env_h > 0x7FFFFFFFu))
        return fail(nullptr, "rt_debug_light_bake_reduce: no environment image (env_rgba NULL or a size of 0) and RT_LIGHT_BAKE_NO_SKY is not set");
    if ((uint64_t)n * ((uint64_t)desc->samples + num_lights) > (1ull << 28)) return fail(nullptr, "rt_debug_light_bake_reduce: more than 2^28 rays");
    light_bake::debug_reduce_host(points, n, first_index, *desc, lights, num_lights, env_rgba, env_w, env_h, occluded, out);
    return RT_OK;
}

// ---- the nearest surface point: rt_scene_nearest / rt_scene_nearest_buffer / rt_debug_nearest / rt_debug_nearest_walk (nearest.hip) --

// everything both forms refuse before anything is launched
static int nearest_refused(rt_ctx* ctx, const char* who, bool points, uint32_t n, bool out, bool surfaces)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"points", points || n == 0u}}, {}) != RT_OK) return RT_ERROR;
    if (!out && !surfaces) return fail(ctx, name + ": no output (out and surfaces are both NULL)");
    return RT_OK;
}

static int nearest_launch(rt_ctx* ctx, const char* who, const rt_point* d_points, uint32_t n, rt_nearest* d_out, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, nearest::launch(ctx->stream, ctx->query, s.d, s.wide_ok, s.n_tris, s.pose ? s.pose->ids : nullptr, ctx->prop.multiProcessorCount, d_points, n,
        d_out, d_surfaces), QUERY_NOT_LAUNCHED);
}

int rt_scene_nearest(rt_ctx* ctx, const rt_point* points, uint32_t n, rt_nearest* out, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (nearest_refused(ctx, "rt_scene_nearest", points != nullptr, n, out != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the points, [1] the records, [3] the surfaces
    return staged_call(ctx, "rt_scene_nearest", q, {{(void*)points, sizeof(rt_point), 0, true}, {out, sizeof(rt_nearest), 1, false}, {surfaces, sizeof(rt_surface), 3, false}}, n,
        (uint32_t)query::CHUNK_RAYS, [&](uint32_t, uint32_t m)
        {
            return nearest_launch(ctx, "rt_scene_nearest", (const rt_point*)q.stage[0], m, out ? (rt_nearest*)q.stage[1] : nullptr, surfaces ? (rt_surface*)q.stage[3] : nullptr);
        });
}

int rt_scene_nearest_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, rt_buffer* out, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (nearest_refused(ctx, "rt_scene_nearest_buffer", points != nullptr, n, out != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_nearest_buffer", {{points, sizeof(rt_point), "points"}, {out, sizeof(rt_nearest), "out"}, {surfaces, sizeof(rt_surface), "surfaces"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return nearest_launch(ctx, "rt_scene_nearest_buffer", (const rt_point*)points->ptr, n, out ? (rt_nearest*)out->ptr : nullptr, surfaces ? (rt_surface*)surfaces->ptr : nullptr);
}

int rt_debug_nearest(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_point* points, uint32_t n, rt_nearest* out)
{
    if (n == 0u) return RT_OK;
    if (!points || !out || (!triangles && num_triangles > 0u)) return fail(ctx, "rt_debug_nearest: NULL argument");
    return host_or_device(ctx, "rt_debug_nearest", [&] { nearest::brute_host(triangles, num_triangles, points, n, out); },
        [&](hipStream_t st) { return nearest::brute_device(st, triangles, num_triangles, points, n, out); });
}

int rt_debug_nearest_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_point* points,
    uint32_t n, rt_nearest* out, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (!nodes || num_nodes == 0u || !triangles || !points || !out) return fail(nullptr, "rt_debug_nearest_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, std::string("rt_debug_nearest_walk") + WIDE_REFUSED);
    if (const char* why = nearest::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, points, n, out, triangles_tested))
        return fail(nullptr, std::string("rt_debug_nearest_walk: ") + why);
    return RT_OK;
}

// ---- every surface a ray crosses: rt_scene_trace_all / rt_scene_trace_all_buffer / rt_debug_trace_all (all_hits.hip) ---------------

// everything both forms refuse before anything is launched
static int all_hits_refused(rt_ctx* ctx, const char* who, bool rays, uint32_t n, uint32_t max_hits, bool out, bool hits, bool surfaces)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"rays", rays || n == 0u}}, {{"out", out}}) != RT_OK) return RT_ERROR;
    if (max_hits > RT_ALL_HITS_MAX) return fail(ctx, name + ": max_hits is above RT_ALL_HITS_MAX");
    if (max_hits == 0u && (hits || surfaces)) return fail(ctx, name + ": hits or surfaces given with max_hits == 0: pass NULL");
    return RT_OK;
}

static int all_hits_launch(rt_ctx* ctx, const char* who, const rt_ray* d_rays, uint32_t n, uint32_t max_hits, rt_ray_hits* d_out, rt_hit* d_hits, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, all_hits::launch(ctx->stream, ctx->query, s.d, s.wide_ok, s.n_tris, s.pose ? s.pose->ids : nullptr, ctx->prop.multiProcessorCount, d_rays, n,
        max_hits, d_out, d_hits, d_surfaces), QUERY_NOT_LAUNCHED);
}

int rt_scene_trace_all(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (all_hits_refused(ctx, "rt_scene_trace_all", rays != nullptr, n, max_hits, out != nullptr, hits != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the rays, [1] the hits, [2] the records, [3] the surfaces; a chunk's rays times max_hits stay within a ray query's chunk
    const uint32_t per_ray = max_hits > 0u ? max_hits : 1u;
    return staged_call(ctx, "rt_scene_trace_all", q, {{(void*)rays, sizeof(rt_ray), 0, true}, {hits, sizeof(rt_hit) * per_ray, 1, false}, {out, sizeof(rt_ray_hits), 2, false},
        {surfaces, sizeof(rt_surface) * per_ray, 3, false}}, n, (uint32_t)query::CHUNK_RAYS / per_ray, [&](uint32_t, uint32_t m)
        {
            return all_hits_launch(ctx, "rt_scene_trace_all", (const rt_ray*)q.stage[0], m, max_hits, (rt_ray_hits*)q.stage[2], hits ? (rt_hit*)q.stage[1] : nullptr,
                surfaces ? (rt_surface*)q.stage[3] : nullptr);
        });
}

int rt_scene_trace_all_buffer(rt_ctx* ctx, rt_buffer* rays, uint32_t n, uint32_t max_hits, rt_buffer* out, rt_buffer* hits, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (all_hits_refused(ctx, "rt_scene_trace_all_buffer", rays != nullptr, n, max_hits, out != nullptr, hits != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_trace_all_buffer", {{rays, sizeof(rt_ray), "rays"}, {out, sizeof(rt_ray_hits), "out"}, {hits, sizeof(rt_hit) * max_hits, "hits"},
            {surfaces, sizeof(rt_surface) * max_hits, "surfaces"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return all_hits_launch(ctx, "rt_scene_trace_all_buffer", (const rt_ray*)rays->ptr, n, max_hits, (rt_ray_hits*)out->ptr, hits ? (rt_hit*)hits->ptr : nullptr,
        surfaces ? (rt_surface*)surfaces->ptr : nullptr);
}

int rt_debug_trace_all(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, const rt_ray* rays, uint32_t n,
    uint32_t max_hits, rt_ray_hits* out, rt_hit* hits)
{
    if (n == 0u) return RT_OK;
    if (!nodes || num_nodes == 0u || !rays || !out || (!triangles && num_triangles > 0u) || (!hits && max_hits > 0u)) return fail(ctx, "rt_debug_trace_all: NULL argument");
    if (max_hits > RT_ALL_HITS_MAX) return fail(ctx, "rt_debug_trace_all: max_hits is above RT_ALL_HITS_MAX");
    if (const char* why = all_hits::leaves_refused(nodes, num_nodes, num_triangles)) return fail(ctx, std::string("rt_debug_trace_all: ") + why);
    return host_or_device(ctx, "rt_debug_trace_all", [&] { all_hits::brute_host(nodes, num_nodes, triangles, rays, n, max_hits, out, hits); },
        [&](hipStream_t st) { return all_hits::brute_device(st, nodes, num_nodes, triangles, num_triangles, rays, n, max_hits, out, hits); });
}

// ---- every triangle within a radius: rt_scene_within / rt_scene_within_buffer / rt_debug_within / rt_debug_within_walk (within.hip) --

// what every entry refuses of max_near and options
static const char* within_shape_refused(uint32_t max_near, uint32_t options)
{
    if (max_near > RT_WITHIN_MAX) return "max_near is above RT_WITHIN_MAX";
    if (options & ~RT_WITHIN_K_NEAREST) return "unknown option bits";
    if ((options & RT_WITHIN_K_NEAREST) && max_near == 0u) return "RT_WITHIN_K_NEAREST needs max_near >= 1";
    return nullptr;
}

// everything both scene forms refuse before anything is launched
static int within_refused(rt_ctx* ctx, const char* who, bool points, uint32_t n, uint32_t max_near, uint32_t options, bool out, bool near, bool surfaces)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {}, {{"points", points || n == 0u}, {"out", out}}) != RT_OK) return RT_ERROR;
    if (const char* why = within_shape_refused(max_near, options)) return fail(ctx, name + ": " + why);
    if (max_near == 0u && (near || surfaces)) return fail(ctx, name + ": near or surfaces given with max_near == 0: pass NULL");
    return RT_OK;
}

static int within_launch(rt_ctx* ctx, const char* who, const rt_point* d_points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* d_out,
    rt_nearest* d_near, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, within::launch(ctx->stream, ctx->query, s.d, s.wide_ok, s.n_tris, s.pose ? s.pose->ids : nullptr, ctx->prop.multiProcessorCount, d_points, n,
        max_near, options, d_out, d_near, d_surfaces), QUERY_NOT_LAUNCHED);
}

int rt_scene_within(rt_ctx* ctx, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (within_refused(ctx, "rt_scene_within", points != nullptr, n, max_near, options, out != nullptr, near != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the points, [1] the members' records, [2] the points' records, [3] the surfaces; a chunk's points times max_near
    // stay within a ray query's chunk
    const uint32_t per_point = max_near > 0u ? max_near : 1u;
    return staged_call(ctx, "rt_scene_within", q, {{(void*)points, sizeof(rt_point), 0, true}, {near, sizeof(rt_nearest) * per_point, 1, false},
        {out, sizeof(rt_point_hits), 2, false}, {surfaces, sizeof(rt_surface) * per_point, 3, false}}, n, (uint32_t)query::CHUNK_RAYS / per_point, [&](uint32_t, uint32_t m)
        {
            return within_launch(ctx, "rt_scene_within", (const rt_point*)q.stage[0], m, max_near, options, (rt_point_hits*)q.stage[2], near ? (rt_nearest*)q.stage[1] : nullptr,
                surfaces ? (rt_surface*)q.stage[3] : nullptr);
        });
}

int rt_scene_within_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, uint32_t max_near, uint32_t options, rt_buffer* out, rt_buffer* near, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (within_refused(ctx, "rt_scene_within_buffer", points != nullptr, n, max_near, options, out != nullptr, near != nullptr, surfaces != nullptr) != RT_OK)
        return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_within_buffer", {{points, sizeof(rt_point), "points"}, {out, sizeof(rt_point_hits), "out"}, {near, sizeof(rt_nearest) * max_near, "near"},
            {surfaces, sizeof(rt_surface) * max_near, "surfaces"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return within_launch(ctx, "rt_scene_within_buffer", (const rt_point*)points->ptr, n, max_near, options, (rt_point_hits*)out->ptr, near ? (rt_nearest*)near->ptr : nullptr,
        surfaces ? (rt_surface*)surfaces->ptr : nullptr);
}

int rt_debug_within(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options,
    rt_point_hits* out, rt_nearest* near)
{
    if (n == 0u) return RT_OK;
    if (const char* why = within_shape_refused(max_near, options)) return fail(ctx, std::string("rt_debug_within: ") + why);
    if (!points || !out || (!triangles && num_triangles > 0u) || (!near && max_near > 0u)) return fail(ctx, "rt_debug_within: NULL argument");
    return host_or_device(ctx, "rt_debug_within", [&] { within::brute_host(triangles, num_triangles, points, n, max_near, options, out, near); },
        [&](hipStream_t st) { return within::brute_device(st, triangles, num_triangles, points, n, max_near, options, out, near); });
}

int rt_debug_within_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_point* points,
    uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (const char* why = within_shape_refused(max_near, options)) return fail(nullptr, std::string("rt_debug_within_walk: ") + why);
    if (!nodes || num_nodes == 0u || !triangles || !points || !out || (!near && max_near > 0u)) return fail(nullptr, "rt_debug_within_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, std::string("rt_debug_within_walk") + WIDE_REFUSED);
    if (const char* why = within::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, points, n, max_near, options, out, near, triangles_tested))
        return fail(nullptr, std::string("rt_debug_within_walk: ") + why);
    return RT_OK;
}

// ---- the triangles of a convex region, and the select: rt_scene_overlap / rt_scene_overlap_buffer / rt_scene_select / rt_scene_select_buffer /
// rt_debug_overlap / rt_debug_overlap_walk / rt_debug_select / rt_debug_rect_region (region.hip) ------------------------------------

// everything both overlap forms refuse before anything is launched
static int overlap_refused(rt_ctx* ctx, const char* who, bool regions, uint32_t n, uint32_t max_list, bool out, bool members)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {}, {{"regions", regions || n == 0u}, {"out", out}}) != RT_OK) return RT_ERROR;
    if (max_list > RT_REGION_LIST_MAX) return fail(ctx, name + ": max_list is above RT_REGION_LIST_MAX");
    if (max_list == 0u && members) return fail(ctx, name + ": members given with max_list == 0: pass NULL");
    return RT_OK;
}

static int overlap_launch(rt_ctx* ctx, const char* who, const rt_region* d_regions, uint32_t n, uint32_t max_list, rt_region_hits* d_out, rt_region_member* d_members)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, region::launch(ctx->stream, ctx->query, s.d, s.wide_ok, ctx->prop.multiProcessorCount, d_regions, n, max_list, d_out, d_members),
        QUERY_NOT_LAUNCHED);
}

int rt_scene_overlap(rt_ctx* ctx, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (overlap_refused(ctx, "rt_scene_overlap", regions != nullptr, n, max_list, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the regions, [1] the members, [2] the regions' records; a chunk's regions times max_list stay within a ray query's chunk
    const uint32_t per_region = max_list > 0u ? max_list : 1u;
    return staged_call(ctx, "rt_scene_overlap", q, {{(void*)regions, sizeof(rt_region), 0, true}, {members, sizeof(rt_region_member) * per_region, 1, false},
        {out, sizeof(rt_region_hits), 2, false}}, n, (uint32_t)query::CHUNK_RAYS / per_region, [&](uint32_t, uint32_t m)
        {
            return overlap_launch(ctx, "rt_scene_overlap", (const rt_region*)q.stage[0], m, max_list, (rt_region_hits*)q.stage[2], members ? (rt_region_member*)q.stage[1] : nullptr);
        });
}

int rt_scene_overlap_buffer(rt_ctx* ctx, rt_buffer* regions, uint32_t n, uint32_t max_list, rt_buffer* out, rt_buffer* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (overlap_refused(ctx, "rt_scene_overlap_buffer", regions != nullptr, n, max_list, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_overlap_buffer", {{regions, sizeof(rt_region), "regions"}, {out, sizeof(rt_region_hits), "out"},
            {members, sizeof(rt_region_member) * max_list, "members"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return overlap_launch(ctx, "rt_scene_overlap_buffer", (const rt_region*)regions->ptr, n, max_list, (rt_region_hits*)out->ptr, members ? (rt_region_member*)members->ptr : nullptr);
}

int rt_debug_overlap(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out,
    rt_region_member* members)
{
    if (n == 0u) return RT_OK;
    if (max_list > RT_REGION_LIST_MAX) return fail(ctx, "rt_debug_overlap: max_list is above RT_REGION_LIST_MAX");
    if (!regions || !out || (!triangles && num_triangles > 0u) || (!members && max_list > 0u)) return fail(ctx, "rt_debug_overlap: NULL argument");
    return host_or_device(ctx, "rt_debug_overlap", [&] { region::brute_host(triangles, num_triangles, regions, n, max_list, out, members); },
        [&](hipStream_t st) { return region::brute_device(st, triangles, num_triangles, regions, n, max_list, out, members); });
}

int rt_debug_overlap_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_region* regions,
    uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (max_list > RT_REGION_LIST_MAX) return fail(nullptr, "rt_debug_overlap_walk: max_list is above RT_REGION_LIST_MAX");
    if (!nodes || num_nodes == 0u || !triangles || !regions || !out || (!members && max_list > 0u)) return fail(nullptr, "rt_debug_overlap_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, std::string("rt_debug_overlap_walk") + WIDE_REFUSED);
    if (const char* why = region::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, regions, n, max_list, out, members, triangles_tested))
        return fail(nullptr, std::string("rt_debug_overlap_walk: ") + why);
    return RT_OK;
}

// everything both select forms refuse before anything is launched
static int select_refused(rt_ctx* ctx, const char* who, bool regions, uint32_t n, bool per_triangle, bool per_object)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {}, {{"regions", regions}}) != RT_OK) return RT_ERROR;
    if (n == 0u || n > RT_SELECT_MAX_REGIONS) return fail(ctx, name + ": n must be 1 .. RT_SELECT_MAX_REGIONS (a bit per region in a 32-bit word)");
    if (!per_triangle && !per_object) return fail(ctx, name + ": no output (every output is NULL)");
    if (per_object && !ctx->scene.pose) return fail(ctx, name + ": the per-object outputs need rt_scene_set_objects");
    return RT_OK;
}

static int select_launch(rt_ctx* ctx, const char* who, const rt_region* d_regions, uint32_t n, uint32_t* d_touching, uint32_t* d_inside, uint32_t* d_object_touching,
    uint32_t* d_object_inside)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, region::select(ctx->stream, ctx->query, s.d, s.n_tris, s.pose ? s.pose->ids : nullptr, s.pose ? s.pose->n_objects : 0u, d_regions, n,
        d_touching, d_inside, d_object_touching, d_object_inside), ": the select could not be launched (out of device memory, or a launch failed)");
}

int rt_scene_select(rt_ctx* ctx, const rt_region* regions, uint32_t n, uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    if (select_refused(ctx, "rt_scene_select", regions != nullptr, n, touching || inside, object_touching || object_inside) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    const Scene& s = ctx->scene;
    const size_t tri_bytes = (size_t)s.n_tris * 4u, obj_bytes = (size_t)(s.pose ? s.pose->n_objects : 0u) * 4u;
    dev::Temps tmp(ctx->stream);
    void* const d_regions = tmp.get(regions, (size_t)n * sizeof(rt_region));
    uint32_t* const d_t = touching ? (uint32_t*)tmp.get(nullptr, tri_bytes) : nullptr;
    uint32_t* const d_i = inside ? (uint32_t*)tmp.get(nullptr, tri_bytes) : nullptr;
    uint32_t* const d_ot = object_touching ? (uint32_t*)tmp.get(nullptr, obj_bytes) : nullptr;
    uint32_t* const d_oi = object_inside ? (uint32_t*)tmp.get(nullptr, obj_bytes) : nullptr;
    if (!d_regions || (touching && !d_t) || (inside && !d_i) || (object_touching && !d_ot) || (object_inside && !d_oi))
        return fail(ctx, "rt_scene_select: out of device memory");
    if (select_launch(ctx, "rt_scene_select", (const rt_region*)d_regions, n, d_t, d_i, d_ot, d_oi) != RT_OK) return RT_ERROR;
    if (touching) HIPCHK(ctx, hipMemcpyAsync(touching, d_t, tri_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (inside) HIPCHK(ctx, hipMemcpyAsync(inside, d_i, tri_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (object_touching) HIPCHK(ctx, hipMemcpyAsync(object_touching, d_ot, obj_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (object_inside) HIPCHK(ctx, hipMemcpyAsync(object_inside, d_oi, obj_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_scene_select_buffer(rt_ctx* ctx, rt_buffer* regions, uint32_t n, rt_buffer* touching, rt_buffer* inside, rt_buffer* object_touching, rt_buffer* object_inside)
{
    if (select_refused(ctx, "rt_scene_select_buffer", regions != nullptr, n, touching || inside, object_touching || object_inside) != RT_OK) return RT_ERROR;
    const Scene& s = ctx->scene;
    if (buffers_refused(ctx, "rt_scene_select_buffer", {{regions, sizeof(rt_region), "regions"}}, n) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_select_buffer", {{touching, 4u, "touching"}, {inside, 4u, "inside"}}, s.n_tris) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_select_buffer", {{object_touching, 4u, "object_touching"}, {object_inside, 4u, "object_inside"}}, s.pose ? s.pose->n_objects : 0u) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    auto p = [](rt_buffer* b) { return b ? (uint32_t*)b->ptr : nullptr; };
    return select_launch(ctx, "rt_scene_select_buffer", (const rt_region*)regions->ptr, n, p(touching), p(inside), p(object_touching), p(object_inside));
}

int rt_debug_select(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, uint32_t num_objects, const rt_region* regions,
    uint32_t n, uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    if (n == 0u || n > RT_SELECT_MAX_REGIONS) return fail(ctx, "rt_debug_select: n must be 1 .. RT_SELECT_MAX_REGIONS (a bit per region in a 32-bit word)");
    if (!regions || ((!triangles || !touching || !inside) && num_triangles > 0u)) return fail(ctx, "rt_debug_select: NULL argument");
    if (object_of_triangle && (num_objects == 0u || !pose::ids_in_range(object_of_triangle, num_triangles, num_objects)))
        return fail(ctx, "rt_debug_select: an object index is not below num_objects");
    return host_or_device(ctx, "rt_debug_select",
        [&] { region::select_host(triangles, num_triangles, object_of_triangle, num_objects, regions, n, touching, inside, object_touching, object_inside); },
        [&](hipStream_t st) { return region::select_device(st, triangles, num_triangles, object_of_triangle, num_objects, regions, n, touching, inside, object_touching, object_inside); });
}

int rt_debug_rect_region(const rt_camera* camera, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far,
    rt_region* out)
{
    if (!camera || !out) return fail(nullptr, "rt_debug_rect_region: NULL argument");
    if (const char* why = region::rect_refused(width, height, x0, y0, x1, y1)) return fail(nullptr, std::string("rt_debug_rect_region: ") + why);
    *out = region::rect_region(*camera, width, height, x0, y0, x1, y1, t_near, t_far);
    return RT_OK;
}

// ---- the triangles a caller's triangle crosses, and a scene's self-crossings: rt_scene_cross / rt_scene_cross_buffer / rt_scene_cross_self /
// rt_scene_cross_self_buffer / rt_debug_cross / rt_debug_cross_walk / rt_debug_cross_self (cross.hip) -------------------------------

// everything the four scene forms refuse before anything is launched; self: probes are the scene's triangles first .. first + n - 1
static int cross_refused(rt_ctx* ctx, const char* who, bool self, bool probes, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, bool out, bool members)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {}, {{"probes", self || probes || n == 0u}, {"out", out}}) != RT_OK) return RT_ERROR;
    if (const char* why = cross_shape_refused(max_list, options, self, members)) return fail(ctx, name + ": " + why);
    if (self && (uint64_t)first + n > ctx->scene.n_tris) return fail(ctx, name + ": first + n is beyond the scene's triangles");
    if ((options & RT_CROSS_OTHER_OBJECTS) && !ctx->scene.pose) return fail(ctx, name + ": RT_CROSS_OTHER_OBJECTS needs rt_scene_set_objects");
    return RT_OK;
}

static int cross_launch(rt_ctx* ctx, const char* who, const rt_probe* d_probes, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* d_out,
    rt_cross_member* d_members)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, cross::launch(ctx->stream, ctx->query, s.d, s.wide_ok, ctx->prop.multiProcessorCount, d_probes, n, max_list, options, d_out, d_members),
        QUERY_NOT_LAUNCHED);
}

static int cross_self_launch(rt_ctx* ctx, const char* who, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* d_out, rt_cross_member* d_members)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, cross::launch_self(ctx->stream, ctx->query, s.d, s.wide_ok, ctx->prop.multiProcessorCount, s.pose ? s.pose->ids : nullptr, first, n,
        max_list, options, d_out, d_members), QUERY_NOT_LAUNCHED);
}

int rt_scene_cross(rt_ctx* ctx, const rt_probe* probes, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (cross_refused(ctx, "rt_scene_cross", false, probes != nullptr, 0u, n, max_list, options, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the probes, [1] the members, [2] the probes' records; a chunk's probes times max_list stay within a ray query's chunk
    const uint32_t per_probe = max_list > 0u ? max_list : 1u;
    return staged_call(ctx, "rt_scene_cross", q, {{(void*)probes, sizeof(rt_probe), 0, true}, {members, sizeof(rt_cross_member) * per_probe, 1, false},
        {out, sizeof(rt_probe_hits), 2, false}}, n, (uint32_t)query::CHUNK_RAYS / per_probe, [&](uint32_t, uint32_t m)
        {
            return cross_launch(ctx, "rt_scene_cross", (const rt_probe*)q.stage[0], m, max_list, options, (rt_probe_hits*)q.stage[2], members ? (rt_cross_member*)q.stage[1] : nullptr);
        });
}

int rt_scene_cross_buffer(rt_ctx* ctx, rt_buffer* probes, uint32_t n, uint32_t max_list, uint32_t options, rt_buffer* out, rt_buffer* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (cross_refused(ctx, "rt_scene_cross_buffer", false, probes != nullptr, 0u, n, max_list, options, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_cross_buffer", {{probes, sizeof(rt_probe), "probes"}, {out, sizeof(rt_probe_hits), "out"},
            {members, sizeof(rt_cross_member) * max_list, "members"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return cross_launch(ctx, "rt_scene_cross_buffer", (const rt_probe*)probes->ptr, n, max_list, options, (rt_probe_hits*)out->ptr, members ? (rt_cross_member*)members->ptr : nullptr);
}

int rt_scene_cross_self(rt_ctx* ctx, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (cross_refused(ctx, "rt_scene_cross_self", true, true, first, n, max_list, options, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [1] the members, [2] the probes' records; nothing goes up
    const uint32_t per_probe = max_list > 0u ? max_list : 1u;
    return staged_call(ctx, "rt_scene_cross_self", q, {{members, sizeof(rt_cross_member) * per_probe, 1, false}, {out, sizeof(rt_probe_hits), 2, false}}, n,
        (uint32_t)query::CHUNK_RAYS / per_probe, [&](uint32_t done, uint32_t m)
        {
            return cross_self_launch(ctx, "rt_scene_cross_self", first + done, m, max_list, options, (rt_probe_hits*)q.stage[2], members ? (rt_cross_member*)q.stage[1] : nullptr);
        });
}

int rt_scene_cross_self_buffer(rt_ctx* ctx, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_buffer* out, rt_buffer* members)
{
    if (ctx && n == 0u) return RT_OK;
    if (cross_refused(ctx, "rt_scene_cross_self_buffer", true, true, first, n, max_list, options, out != nullptr, members != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_cross_self_buffer", {{out, sizeof(rt_probe_hits), "out"}, {members, sizeof(rt_cross_member) * max_list, "members"}}, n) != RT_OK)
        return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return cross_self_launch(ctx, "rt_scene_cross_self_buffer", first, n, max_list, options, (rt_probe_hits*)out->ptr, members ? (rt_cross_member*)members->ptr : nullptr);
}

// what the debug forms refuse of their shape: the scene forms' rule (members with max_list == 0 or with RT_CROSS_ANY are refused there too); beyond it a
// debug form REQUIRES members exactly when it is listed into (max_list > 0 and no RT_CROSS_ANY), which its NULL-argument check says
static const char* debug_cross_refused(bool self, uint32_t max_list, uint32_t options, bool members)
{
    return cross_shape_refused(max_list, options, self, members);
}

int rt_debug_cross(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_probe* probes, uint32_t n, uint32_t max_list, uint32_t options,
    rt_probe_hits* out, rt_cross_member* members)
{
    if (n == 0u) return RT_OK;
    if (const char* why = debug_cross_refused(false, max_list, options, members != nullptr)) return fail(ctx, std::string("rt_debug_cross: ") + why);
    const bool any = (options & RT_CROSS_ANY) != 0u;
    if (!probes || !out || (!triangles && num_triangles > 0u) || (!members && max_list > 0u && !any)) return fail(ctx, "rt_debug_cross: NULL argument");
    return host_or_device(ctx, "rt_debug_cross", [&] { cross::brute_host(triangles, num_triangles, probes, nullptr, 0u, n, max_list, options, out, members); },
        [&](hipStream_t st) { return cross::brute_device(st, triangles, num_triangles, probes, nullptr, 0u, n, max_list, options, out, members); });
}

int rt_debug_cross_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_probe* probes,
    uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (const char* why = debug_cross_refused(false, max_list, options, members != nullptr)) return fail(nullptr, std::string("rt_debug_cross_walk: ") + why);
    const bool any = (options & RT_CROSS_ANY) != 0u;
    if (!nodes || num_nodes == 0u || !triangles || !probes || !out || (!members && max_list > 0u && !any)) return fail(nullptr, "rt_debug_cross_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, std::string("rt_debug_cross_walk") + WIDE_REFUSED);
    if (const char* why = cross::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, probes, n, max_list, options, out, members, triangles_tested))
        return fail(nullptr, std::string("rt_debug_cross_walk: ") + why);
    return RT_OK;
}

int rt_debug_cross_self(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, uint32_t first, uint32_t n,
    uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (n == 0u) return RT_OK;
    if (const char* why = debug_cross_refused(true, max_list, options, members != nullptr)) return fail(ctx, std::string("rt_debug_cross_self: ") + why);
    const bool any = (options & RT_CROSS_ANY) != 0u;
    if (!triangles || !out || (!members && max_list > 0u && !any)) return fail(ctx, "rt_debug_cross_self: NULL argument");
    if ((uint64_t)first + n > num_triangles) return fail(ctx, "rt_debug_cross_self: first + n is beyond the triangles");
    if ((options & RT_CROSS_OTHER_OBJECTS) && !object_of_triangle) return fail(ctx, "rt_debug_cross_self: RT_CROSS_OTHER_OBJECTS needs object_of_triangle");
    return host_or_device(ctx, "rt_debug_cross_self",
        [&] { cross::brute_host(triangles, num_triangles, nullptr, object_of_triangle, first, n, max_list, options, out, members); },
        [&](hipStream_t st) { return cross::brute_device(st, triangles, num_triangles, nullptr, object_of_triangle, first, n, max_list, options, out, members); });
}

// ---- the nearest scene triangle to a caller's triangle, and a scene's clearances: rt_scene_separation / rt_scene_separation_buffer /
// rt_scene_separation_self / rt_scene_separation_self_buffer / rt_debug_separation / rt_debug_separation_walk / rt_debug_separation_self (separation.hip,
// DESIGN.md section 7o) ---------------------------------------------------------------------------------------------------------------------------------

// everything the four scene forms refuse before anything is launched; self: probes are the scene's triangles first .. first + n - 1
static int separation_refused(rt_ctx* ctx, const char* who, bool self, bool probes, uint32_t first, uint32_t n, uint32_t options, bool out)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {}, {{"probes", self || probes || n == 0u}, {"out", out}}) != RT_OK) return RT_ERROR;
    if (const char* why = sep_shape_refused(options, self)) return fail(ctx, name + ": " + why);
    if (self && (uint64_t)first + n > ctx->scene.n_tris) return fail(ctx, name + ": first + n is beyond the scene's triangles");
    if ((options & RT_SEPARATION_OTHER_OBJECTS) && !ctx->scene.pose) return fail(ctx, name + ": RT_SEPARATION_OTHER_OBJECTS needs rt_scene_set_objects");
    return RT_OK;
}

static int separation_launch(rt_ctx* ctx, const char* who, const rt_probe* d_probes, uint32_t n, float max_distance, rt_separation* d_out)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, separation::launch(ctx->stream, ctx->query, s.d, s.wide_ok, ctx->prop.multiProcessorCount, d_probes, n, max_distance, d_out),
        QUERY_NOT_LAUNCHED);
}

static int separation_self_launch(rt_ctx* ctx, const char* who, uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_separation* d_out)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, separation::launch_self(ctx->stream, ctx->query, s.d, s.wide_ok, ctx->prop.multiProcessorCount, s.pose ? s.pose->ids : nullptr, first, n,
        max_distance, options, d_out), QUERY_NOT_LAUNCHED);
}

int rt_scene_separation(rt_ctx* ctx, const rt_probe* probes, uint32_t n, float max_distance, uint32_t options, rt_separation* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (separation_refused(ctx, "rt_scene_separation", false, probes != nullptr, 0u, n, options, out != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the probes, [2] the records
    return staged_call(ctx, "rt_scene_separation", q, {{(void*)probes, sizeof(rt_probe), 0, true}, {out, sizeof(rt_separation), 2, false}}, n, (uint32_t)query::CHUNK_RAYS,
        [&](uint32_t, uint32_t m) { return separation_launch(ctx, "rt_scene_separation", (const rt_probe*)q.stage[0], m, max_distance, (rt_separation*)q.stage[2]); });
}

int rt_scene_separation_buffer(rt_ctx* ctx, rt_buffer* probes, uint32_t n, float max_distance, uint32_t options, rt_buffer* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (separation_refused(ctx, "rt_scene_separation_buffer", false, probes != nullptr, 0u, n, options, out != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_separation_buffer", {{probes, sizeof(rt_probe), "probes"}, {out, sizeof(rt_separation), "out"}}, n) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return separation_launch(ctx, "rt_scene_separation_buffer", (const rt_probe*)probes->ptr, n, max_distance, (rt_separation*)out->ptr);
}

int rt_scene_separation_self(rt_ctx* ctx, uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_separation* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (separation_refused(ctx, "rt_scene_separation_self", true, true, first, n, options, out != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [2] the records; nothing goes up
    return staged_call(ctx, "rt_scene_separation_self", q, {{out, sizeof(rt_separation), 2, false}}, n, (uint32_t)query::CHUNK_RAYS, [&](uint32_t done, uint32_t m)
        {
            return separation_self_launch(ctx, "rt_scene_separation_self", first + done, m, max_distance, options, (rt_separation*)q.stage[2]);
        });
}

int rt_scene_separation_self_buffer(rt_ctx* ctx, uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_buffer* out)
{
    if (ctx && n == 0u) return RT_OK;
    if (separation_refused(ctx, "rt_scene_separation_self_buffer", true, true, first, n, options, out != nullptr) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_separation_self_buffer", {{out, sizeof(rt_separation), "out"}}, n) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return separation_self_launch(ctx, "rt_scene_separation_self_buffer", first, n, max_distance, options, (rt_separation*)out->ptr);
}

int rt_debug_separation(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_probe* probes, uint32_t n, float max_distance, rt_separation* out)
{
    if (n == 0u) return RT_OK;
    if (!probes || !out || (!triangles && num_triangles > 0u)) return fail(ctx, "rt_debug_separation: NULL argument");
    return host_or_device(ctx, "rt_debug_separation", [&] { separation::brute_host(triangles, num_triangles, probes, nullptr, 0u, n, max_distance, 0u, out); },
        [&](hipStream_t st) { return separation::brute_device(st, triangles, num_triangles, probes, nullptr, 0u, n, max_distance, 0u, out); });
}

int rt_debug_separation_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_probe* probes,
    uint32_t n, float max_distance, rt_separation* out, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (!nodes || num_nodes == 0u || !triangles || !probes || !out) return fail(nullptr, "rt_debug_separation_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, std::string("rt_debug_separation_walk") + WIDE_REFUSED);
    if (const char* why = separation::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, probes, n, max_distance, out, triangles_tested))
        return fail(nullptr, std::string("rt_debug_separation_walk: ") + why);
    return RT_OK;
}

int rt_debug_separation_self(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, uint32_t first, uint32_t n,
    float max_distance, uint32_t options, rt_separation* out)
{
    if (n == 0u) return RT_OK;
    if (const char* why = sep_shape_refused(options, true)) return fail(ctx, std::string("rt_debug_separation_self: ") + why);
    if (!triangles || !out) return fail(ctx, "rt_debug_separation_self: NULL argument");
    if ((uint64_t)first + n > num_triangles) return fail(ctx, "rt_debug_separation_self: first + n is beyond the triangles");
    if ((options & RT_SEPARATION_OTHER_OBJECTS) && !object_of_triangle) return fail(ctx, "rt_debug_separation_self: RT_SEPARATION_OTHER_OBJECTS needs object_of_triangle");
    return host_or_device(ctx, "rt_debug_separation_self",
        [&] { separation::brute_host(triangles, num_triangles, nullptr, object_of_triangle, first, n, max_distance, options, out); },
        [&](hipStream_t st) { return separation::brute_device(st, triangles, num_triangles, nullptr, object_of_triangle, first, n, max_distance, options, out); });
}

// ---- the UV atlas: rt_scene_atlas / rt_scene_atlas_buffer / rt_scene_atlas_surfaces / rt_scene_atlas_surfaces_buffer / rt_scene_atlas_bake / rt_debug_atlas
// (atlas.hip).  No tree is walked.  The work area and the host forms' arrays are the bakes' scratch (ctx->bake): [0] the UVs, then a
// bake's surfaces, [1] a bake's results, [2] the cover's work area, [3] the texels ------------------------------------------------------------------------

// everything the cover's forms refuse before anything is launched
static int atlas_refused(rt_ctx* ctx, const char* who, const rt_atlas_desc* desc, std::initializer_list<Needed> outputs)
{
    const std::string name(who);
    if (opening_refused(ctx, name, {{"desc", desc != nullptr}}, {}) != RT_OK) return RT_ERROR;
    for (const Needed& a : outputs) if (!a.given) return fail(ctx, name + ": " + a.what + " is NULL");
    if (const char* why = atlas_desc_refusal(*desc)) return fail(ctx, name + ": " + why);
    if (desc->object != RT_INVALID_ID)
    {
        if (!ctx->scene.pose) return fail(ctx, name + ": desc.object needs rt_scene_set_objects");
        if (desc->object >= ctx->scene.pose->n_objects) return fail(ctx, name + ": desc.object is not below the object count");
    }
    return RT_OK;
}

static int atlas_launch(rt_ctx* ctx, const char* who, void* d_work, const rt_atlas_desc& desc, const float* d_uv, rt_texel* d_texels)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, atlas::launch(ctx->stream, d_work, desc, d_uv, s.d.tris_sh, s.n_tris, s.pose ? s.pose->ids : nullptr, d_texels),
        ": the cover could not be launched (a launch failed)");
}

// the host forms' cover: afterwards, in stream order, the texels are the bakes' stage [3] and the statistics the head of stage [2]
static int atlas_on_scratch(rt_ctx* ctx, const char* who, const rt_atlas_desc& desc, const float* uv)
{
    query::Scratch& b = ctx->bake;
    const size_t n = (size_t)desc.width * desc.height, uv_bytes = (size_t)ctx->scene.n_tris * 24u;
    if ((uv && !query::reserve(ctx->stream, b, 0, uv_bytes)) || !query::reserve(ctx->stream, b, 2, atlas::work_bytes(desc)) || !query::reserve(ctx->stream, b, 3, n * sizeof(rt_texel)))
        return fail(ctx, std::string(who) + ": out of device memory for the atlas");
    if (uv && uv_bytes) HIPCHK(ctx, hipMemcpyAsync(b.stage[0], uv, uv_bytes, hipMemcpyHostToDevice, ctx->stream));
    return atlas_launch(ctx, who, b.stage[2], desc, uv ? (const float*)b.stage[0] : nullptr, (rt_texel*)b.stage[3]);
}

int rt_scene_atlas(rt_ctx* ctx, const rt_atlas_desc* desc, const float* uv, rt_texel* texels, rt_atlas_stats* stats)
{
    if (atlas_refused(ctx, "rt_scene_atlas", desc, {{"texels", texels != nullptr}}) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    if (atlas_on_scratch(ctx, "rt_scene_atlas", *desc, uv) != RT_OK) return RT_ERROR;
    HIPCHK(ctx, hipMemcpyAsync(texels, ctx->bake.stage[3], (size_t)desc->width * desc->height * sizeof(rt_texel), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, ctx->bake.stage[2], sizeof(rt_atlas_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_scene_atlas_buffer(rt_ctx* ctx, const rt_atlas_desc* desc, rt_buffer* uv, rt_buffer* texels, rt_buffer* stats)
{
    if (atlas_refused(ctx, "rt_scene_atlas_buffer", desc, {{"texels", texels != nullptr}}) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_atlas_buffer", {{uv, 24u, "uv"}}, ctx->scene.n_tris) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_atlas_buffer", {{texels, sizeof(rt_texel), "texels"}}, desc->width * desc->height) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_atlas_buffer", {{stats, sizeof(rt_atlas_stats), "stats"}}, 1u) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    if (!query::reserve(ctx->stream, ctx->bake, 2, atlas::work_bytes(*desc))) return fail(ctx, "rt_scene_atlas_buffer: out of device memory for the atlas");
    if (atlas_launch(ctx, "rt_scene_atlas_buffer", ctx->bake.stage[2], *desc, uv ? (const float*)uv->ptr : nullptr, (rt_texel*)texels->ptr) != RT_OK) return RT_ERROR;
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats->ptr, ctx->bake.stage[2], sizeof(rt_atlas_stats), hipMemcpyDeviceToDevice, ctx->stream));
    return RT_OK;
}

static int atlas_surfaces_launch(rt_ctx* ctx, const char* who, const rt_texel* d_texels, uint32_t n, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    return launch_result(ctx, who, atlas::launch_surfaces(ctx->stream, s.d.tris_sh, s.n_tris, s.pose ? s.pose->ids : nullptr, d_texels, n, d_surfaces),
        ": the surfaces could not be launched (the launch failed)");
}

int rt_scene_atlas_surfaces(rt_ctx* ctx, const rt_texel* texels, uint32_t n, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (opening_refused(ctx, "rt_scene_atlas_surfaces", {{"texels", texels != nullptr}, {"surfaces", surfaces != nullptr}}, {}) != RT_OK) return RT_ERROR;
    for (uint32_t i = 0; i < n; ++i)
        if (texels[i].primitive_id != RT_INVALID_ID && texels[i].primitive_id >= ctx->scene.n_tris)
            return fail(ctx, "rt_scene_atlas_surfaces: a record's primitive_id is not below the scene's triangle count");
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the texels, [3] the surfaces
    return staged_call(ctx, "rt_scene_atlas_surfaces", q, {{(void*)texels, sizeof(rt_texel), 0, true}, {surfaces, sizeof(rt_surface), 3, false}}, n, (uint32_t)query::CHUNK_RAYS,
        [&](uint32_t, uint32_t m) { return atlas_surfaces_launch(ctx, "rt_scene_atlas_surfaces", (const rt_texel*)q.stage[0], m, (rt_surface*)q.stage[3]); });
}

int rt_scene_atlas_surfaces_buffer(rt_ctx* ctx, rt_buffer* texels, uint32_t n, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (opening_refused(ctx, "rt_scene_atlas_surfaces_buffer", {{"texels", texels != nullptr}, {"surfaces", surfaces != nullptr}}, {}) != RT_OK) return RT_ERROR;
    if (buffers_refused(ctx, "rt_scene_atlas_surfaces_buffer", {{texels, sizeof(rt_texel), "texels"}, {surfaces, sizeof(rt_surface), "surfaces"}}, n) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return atlas_surfaces_launch(ctx, "rt_scene_atlas_surfaces_buffer", (const rt_texel*)texels->ptr, n, (rt_surface*)surfaces->ptr);
}

int rt_scene_atlas_bake(rt_ctx* ctx, const rt_atlas_desc* atlas_desc, const float* uv, const rt_bake_desc* bake_desc, rt_bake_result* out, rt_texel* texels,
    rt_atlas_stats* stats)
{
    static const char who[] = "rt_scene_atlas_bake";
    if (atlas_refused(ctx, who, atlas_desc, {{"bake_desc", bake_desc != nullptr}, {"out", out != nullptr}}) != RT_OK) return RT_ERROR;
    if (bake_desc->flags != 0u) return fail(ctx, std::string(who) + ": bake_desc->flags must be 0 (the records are the atlas's own surfaces)");
    rt_bake_desc bd = *bake_desc;
    bd.flags = RT_BAKE_FROM_SURFACES;
    if (const char* why = bake::desc_refusal(bd)) return fail(ctx, std::string(who) + ": " + why);
    (void)hipSetDevice(ctx->device);
    if (atlas_on_scratch(ctx, who, *atlas_desc, uv) != RT_OK) return RT_ERROR;
    query::Scratch& b = ctx->bake;
    const uint32_t n = atlas_desc->width * atlas_desc->height;
    if (texels) HIPCHK(ctx, hipMemcpyAsync(texels, b.stage[3], (size_t)n * sizeof(rt_texel), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, b.stage[2], sizeof(rt_atlas_stats), hipMemcpyDeviceToHost, ctx->stream));
    // the bake's chunks: a chunk's surfaces are made in stage [0] from the resident texels (the UVs there have been read: a stage is re-allocated only after
    // the stream has been waited for), baked into stage [1] with the chunk's first index, and only the results come down
    return staged_call(ctx, who, b, {{out, sizeof(rt_bake_result), 1, false}}, n, ctx->bake_chunk_points, [&](uint32_t first, uint32_t m)
        {
            if (!query::reserve(ctx->stream, b, 0, (size_t)m * sizeof(rt_surface))) return fail(ctx, std::string(who) + ": out of device memory for the staging arrays");
            if (atlas_surfaces_launch(ctx, who, (const rt_texel*)b.stage[3] + first, m, (rt_surface*)b.stage[0]) != RT_OK) return (int)RT_ERROR;
            return bake_launch(ctx, who, b.stage[0], m, first, bd, (rt_bake_result*)b.stage[1]);
        });
}

// rt_scene_atlas_bake with the light bake in the occlusion bake's place (light_bake.hip): the same cover, the same chunks
int rt_scene_atlas_bake_light(rt_ctx* ctx, const rt_atlas_desc* atlas_desc, const float* uv, const rt_light_bake_desc* desc, rt_light_bake_result* out, rt_texel* texels,
    rt_atlas_stats* stats)
{
    static const char who[] = "rt_scene_atlas_bake_light";
    if (atlas_refused(ctx, who, atlas_desc, {{"desc", desc != nullptr}, {"out", out != nullptr}}) != RT_OK) return RT_ERROR;
    if (desc->flags != 0u) return fail(ctx, std::string(who) + ": desc->flags must be 0 (the records are the atlas's own surfaces)");
    rt_light_bake_desc bd = *desc;
    bd.flags = RT_BAKE_FROM_SURFACES;
    if (const char* why = light_bake::desc_refusal(bd)) return fail(ctx, std::string(who) + ": " + why);
    (void)hipSetDevice(ctx->device);
    if (atlas_on_scratch(ctx, who, *atlas_desc, uv) != RT_OK) return RT_ERROR;
    query::Scratch& b = ctx->bake;
    const uint32_t n = atlas_desc->width * atlas_desc->height;
    if (texels) HIPCHK(ctx, hipMemcpyAsync(texels, b.stage[3], (size_t)n * sizeof(rt_texel), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, b.stage[2], sizeof(rt_atlas_stats), hipMemcpyDeviceToHost, ctx->stream));
    return staged_call(ctx, who, b, {{out, sizeof(rt_light_bake_result), 1, false}}, n, ctx->bake_chunk_points, [&](uint32_t first, uint32_t m)
        {
            if (!query::reserve(ctx->stream, b, 0, (size_t)m * sizeof(rt_surface))) return fail(ctx, std::string(who) + ": out of device memory for the staging arrays");
            if (atlas_surfaces_launch(ctx, who, (const rt_texel*)b.stage[3] + first, m, (rt_surface*)b.stage[0]) != RT_OK) return (int)RT_ERROR;
            return light_bake_launch(ctx, who, b.stage[0], m, first, bd, (rt_light_bake_result*)b.stage[1]);
        });
}

int rt_debug_atlas(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, const float* uv, const rt_atlas_desc* desc,
    rt_texel* texels, rt_atlas_stats* stats)
{
    if (!desc || !texels || (!triangles && !uv && num_triangles > 0u)) return fail(ctx, "rt_debug_atlas: NULL argument");
    if (const char* why = atlas_desc_refusal(*desc)) return fail(ctx, std::string("rt_debug_atlas: ") + why);
    if (desc->object != RT_INVALID_ID && !object_of_triangle && num_triangles > 0u) return fail(ctx, "rt_debug_atlas: desc.object needs object_of_triangle");
    return host_or_device(ctx, "rt_debug_atlas", [&] { atlas::cover_host(triangles, num_triangles, object_of_triangle, uv, *desc, texels, stats); },
        [&](hipStream_t st) { return atlas::cover_device(st, triangles, num_triangles, object_of_triangle, uv, *desc, texels, stats); });
}

} // extern "C"
