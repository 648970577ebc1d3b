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
