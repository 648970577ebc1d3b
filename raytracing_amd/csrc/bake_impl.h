// bake_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after query_impl.h): rt_scene_bake / rt_scene_bake_buffer /
// rt_debug_bake_rays / rt_debug_bake_reduce, the bookkeeping around bake.hip's kernels.  Like a query, a bake reads the scene and writes
// the caller's arrays: it launches on the context's stream -- behind every refit, pose and upload, which end there -- and touches no frame.

// everything both forms refuse before anything is launched
static int bake_refused(rt_ctx* ctx, const char* who, bool points, uint32_t n, const rt_bake_desc* desc, bool out)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!points) return fail(ctx, name + ": points is NULL");
    if (!desc) return fail(ctx, name + ": desc is NULL");
    if (!out) return fail(ctx, name + ": out is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
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
    if (!ctx) { bake::debug_rays_host(points, n, first_index, *desc, rays_out); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!bake::debug_rays_device(ctx->stream, points, n, first_index, *desc, rays_out))
        return fail(ctx, "rt_debug_bake_rays: the device path failed (allocation, copy or launch)");
    return RT_OK;
}

int rt_debug_bake_reduce(const rt_ray* rays, const uint32_t* occluded, uint32_t n, uint32_t samples, rt_bake_result* out)
{
    if (n == 0u) return RT_OK;
    if (!rays || !occluded || !out) return fail(nullptr, "rt_debug_bake_reduce: NULL argument");
    if (samples < 16u || samples > 4096u || (samples & (samples - 1u)) != 0u) return fail(nullptr, "rt_debug_bake_reduce: samples must be a power of two in 16 .. 4096");
    bake::debug_reduce_host(rays, occluded, n, samples, out);
    return RT_OK;
}
