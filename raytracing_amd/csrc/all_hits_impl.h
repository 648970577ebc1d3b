// all_hits_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after nearest_impl.h): rt_scene_trace_all /
// rt_scene_trace_all_buffer / rt_frame_pick_all / rt_debug_trace_all, the bookkeeping around all_hits.hip's kernels.  Like a ray query,
// an all-hits query reads the scene and writes the caller's arrays: it launches on the context's stream -- behind every refit, pose and upload, which end
// there -- and touches no frame.  Its stack spill area, status word and staging arrays are the ray queries' (ctx->query), so rt_scene_tree_report's "ray
// queries" line counts them.

// everything both forms refuse before anything is launched
static int all_hits_refused(rt_ctx* ctx, const char* who, bool rays, uint32_t n, uint32_t max_hits, bool out, bool hits, bool surfaces)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!rays && n > 0u) return fail(ctx, name + ": rays is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (!out) return fail(ctx, name + ": out is NULL");
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

int rt_frame_pick_all(rt_frame* f, uint32_t x, uint32_t y, uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    if (!f) return fail(nullptr, "rt_frame_pick_all: frame is NULL");
    rt_ctx* ctx = f->ctx;
    if (!ctx->scene.valid) return fail(ctx, "rt_frame_pick_all: no scene uploaded");
    if (f->tile.nranks > 1) return fail(ctx, "rt_frame_pick_all: a tile frame (tile_count > 1): pick on a frame of the whole image");
    if (x >= f->tile.width || y >= f->tile.height) return fail(ctx, "rt_frame_pick_all: the pixel is outside the image");
    const rt_ray r = query::pick_ray(f->camera, f->tile.width, f->tile.height, x, y);
    if (rt_scene_trace_all(ctx, &r, 1u, max_hits, out, hits, surfaces) != RT_OK) return RT_ERROR;
    if (ray) *ray = r;
    return RT_OK;
}

int rt_debug_trace_all(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, const rt_ray* rays, uint32_t n,
    uint32_t max_hits, rt_ray_hits* out, rt_hit* hits)
{
    if (n == 0u) return RT_OK;
    if (!nodes || num_nodes == 0u || !rays || !out || (!triangles && num_triangles > 0u) || (!hits && max_hits > 0u)) return fail(ctx, "rt_debug_trace_all: NULL argument");
    if (max_hits > RT_ALL_HITS_MAX) return fail(ctx, "rt_debug_trace_all: max_hits is above RT_ALL_HITS_MAX");
    if (const char* why = all_hits::leaves_refused(nodes, num_nodes, num_triangles)) return fail(ctx, std::string("rt_debug_trace_all: ") + why);
    if (!ctx) { all_hits::brute_host(nodes, num_nodes, triangles, rays, n, max_hits, out, hits); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!all_hits::brute_device(ctx->stream, nodes, num_nodes, triangles, num_triangles, rays, n, max_hits, out, hits))
        return fail(ctx, "rt_debug_trace_all: the device path failed (allocation, copy or launch)");
    return RT_OK;
}
