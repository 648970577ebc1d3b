// nearest_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after bake_impl.h): rt_scene_nearest / rt_scene_nearest_buffer /
// rt_debug_nearest / rt_debug_nearest_walk, the bookkeeping around nearest.hip's kernels.  Like a ray query, a nearest query reads the
// scene and writes the caller's arrays: it launches on the context's stream -- behind every refit, pose and upload, which end there -- and touches no frame.
// Its stack spill area, status word and staging arrays are the ray queries' (ctx->query), so rt_scene_tree_report's "ray queries" line counts them.

// everything both forms refuse before anything is launched
static int nearest_refused(rt_ctx* ctx, const char* who, bool points, uint32_t n, bool out, bool surfaces)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!points && n > 0u) return fail(ctx, name + ": points is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (!out && !surfaces) return fail(ctx, name + ": no output (out and surfaces are both NULL)");
    return RT_OK;
}

static int nearest_launch(rt_ctx* ctx, const char* who, const rt_point* d_points, uint32_t n, rt_nearest* d_out, rt_surface* d_surfaces)
{
    const Scene& s = ctx->scene;
    if (!nearest::launch(ctx->stream, ctx->query, s.d, s.wide_ok, s.n_tris, s.pose ? s.pose->ids : nullptr, ctx->prop.multiProcessorCount, d_points, n, d_out, d_surfaces))
    {
        (void)hipGetLastError();
        return fail(ctx, std::string(who) + ": the query could not be launched (the stack spill area could not be allocated, or a launch failed)");
    }
    return RT_OK;
}

int rt_scene_nearest(rt_ctx* ctx, const rt_point* points, uint32_t n, rt_nearest* out, rt_surface* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (nearest_refused(ctx, "rt_scene_nearest", points != nullptr, n, out != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    query::Scratch& q = ctx->query;
    // the ray queries' staging arrays: [0] the points, [1] the records, [3] the surfaces
    for (uint32_t first = 0; first < n; )
    {
        const uint32_t m = n - first < (uint32_t)query::CHUNK_RAYS ? n - first : (uint32_t)query::CHUNK_RAYS;
        if (!query::reserve(ctx->stream, q, 0, (size_t)m * sizeof(rt_point)) || (out && !query::reserve(ctx->stream, q, 1, (size_t)m * sizeof(rt_nearest))) ||
            (surfaces && !query::reserve(ctx->stream, q, 3, (size_t)m * sizeof(rt_surface))))
            return fail(ctx, "rt_scene_nearest: out of device memory for the staging arrays");
        HIPCHK(ctx, hipMemcpyAsync(q.stage[0], points + first, (size_t)m * sizeof(rt_point), hipMemcpyHostToDevice, ctx->stream));
        if (nearest_launch(ctx, "rt_scene_nearest", (const rt_point*)q.stage[0], m, out ? (rt_nearest*)q.stage[1] : nullptr, surfaces ? (rt_surface*)q.stage[3] : nullptr) != RT_OK)
            return RT_ERROR;
        if (out) HIPCHK(ctx, hipMemcpyAsync(out + first, q.stage[1], (size_t)m * sizeof(rt_nearest), hipMemcpyDeviceToHost, ctx->stream));
        if (surfaces) HIPCHK(ctx, hipMemcpyAsync(surfaces + first, q.stage[3], (size_t)m * sizeof(rt_surface), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (query_check_status(ctx, "rt_scene_nearest") != RT_OK) return RT_ERROR;
        first += m;
    }
    return RT_OK;
}

int rt_scene_nearest_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, rt_buffer* out, rt_buffer* surfaces)
{
    if (ctx && n == 0u) return RT_OK;
    if (nearest_refused(ctx, "rt_scene_nearest_buffer", points != nullptr, n, out != nullptr, surfaces != nullptr) != RT_OK) return RT_ERROR;
    const struct { rt_buffer* b; size_t record; const char* what; } bufs[3] = {{points, sizeof(rt_point), "points"}, {out, sizeof(rt_nearest), "out"},
        {surfaces, sizeof(rt_surface), "surfaces"}};
    for (const auto& b : bufs)
    {
        if (!b.b) continue;
        if (b.b->ctx != ctx) return fail(ctx, std::string("rt_scene_nearest_buffer: the ") + b.what + " buffer belongs to another context");
        if (b.b->bytes < (size_t)n * b.record) return fail(ctx, std::string("rt_scene_nearest_buffer: the ") + b.what + " buffer is smaller than n records");
    }
    (void)hipSetDevice(ctx->device);
    return nearest_launch(ctx, "rt_scene_nearest_buffer", (const rt_point*)points->ptr, n, out ? (rt_nearest*)out->ptr : nullptr, surfaces ? (rt_surface*)surfaces->ptr : nullptr);
}

int rt_debug_nearest(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const rt_point* points, uint32_t n, rt_nearest* out)
{
    if (n == 0u) return RT_OK;
    if (!points || !out || (!triangles && num_triangles > 0u)) return fail(ctx, "rt_debug_nearest: NULL argument");
    if (!ctx) { nearest::brute_host(triangles, num_triangles, points, n, out); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!nearest::brute_device(ctx->stream, triangles, num_triangles, points, n, out))
        return fail(ctx, "rt_debug_nearest: the device path failed (allocation, copy or launch)");
    return RT_OK;
}

int rt_debug_nearest_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_point* points,
    uint32_t n, rt_nearest* out, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (!nodes || num_nodes == 0u || !triangles || !points || !out) return fail(nullptr, "rt_debug_nearest_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, "rt_debug_nearest_walk: wide must be 0 (the child-pair form) or 1 (the 4-wide records)");
    if (const char* why = nearest::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, points, n, out, triangles_tested))
        return fail(nullptr, std::string("rt_debug_nearest_walk: ") + why);
    return RT_OK;
}
