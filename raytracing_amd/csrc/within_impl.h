// within_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after all_hits_impl.h): rt_scene_within /
// rt_scene_within_buffer / rt_debug_within / rt_debug_within_walk, the bookkeeping around within.hip's kernels.  Like a nearest query,
// a within query reads the scene and writes the caller's arrays: it launches on the context's stream -- behind every refit, pose and upload, which end
// there -- and touches no frame.  Its stack spill area, status word and staging arrays are the ray queries' (ctx->query), so rt_scene_tree_report's "ray
// queries" line counts them.

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
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (!points && n > 0u) return fail(ctx, name + ": points is NULL");
    if (!out) return fail(ctx, name + ": out is NULL");
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
    if (!ctx) { within::brute_host(triangles, num_triangles, points, n, max_near, options, out, near); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!within::brute_device(ctx->stream, triangles, num_triangles, points, n, max_near, options, out, near))
        return fail(ctx, "rt_debug_within: the device path failed (allocation, copy or launch)");
    return RT_OK;
}

int rt_debug_within_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_point* points,
    uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (const char* why = within_shape_refused(max_near, options)) return fail(nullptr, std::string("rt_debug_within_walk: ") + why);
    if (!nodes || num_nodes == 0u || !triangles || !points || !out || (!near && max_near > 0u)) return fail(nullptr, "rt_debug_within_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, "rt_debug_within_walk: wide must be 0 (the child-pair form) or 1 (the 4-wide records)");
    if (const char* why = within::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, points, n, max_near, options, out, near, triangles_tested))
        return fail(nullptr, std::string("rt_debug_within_walk: ") + why);
    return RT_OK;
}
