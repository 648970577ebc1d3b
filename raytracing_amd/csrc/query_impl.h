// query_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after pose_impl.h): rt_scene_trace / rt_scene_trace_buffer /
// rt_frame_pick / rt_debug_query_surface, the bookkeeping around query.hip's kernels.  A query reads the scene and writes the caller's
// arrays: it launches on the context's stream -- behind every refit, pose and upload, which end there -- and touches no frame.

// everything both forms refuse before anything is launched
static int query_refused(rt_ctx* ctx, const char* who, bool rays, uint32_t n, uint32_t mode, bool hits, bool occluded, bool surfaces)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!rays && n > 0u) return fail(ctx, name + ": rays is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_ANY_HIT) return fail(ctx, name + ": unknown mode (RT_QUERY_CLOSEST or RT_QUERY_ANY_HIT)");
    if (mode == RT_QUERY_CLOSEST && !hits && !occluded && !surfaces) return fail(ctx, name + ": no output (hits, occluded and surfaces are all NULL)");
    if (mode == RT_QUERY_ANY_HIT && (hits || surfaces)) return fail(ctx, name + ": RT_QUERY_ANY_HIT reports no hits or surfaces (which triangle occludes depends on the tree): pass NULL");
    if (mode == RT_QUERY_ANY_HIT && !occluded) return fail(ctx, name + ": no output (occluded is NULL)");
    return RT_OK;
}

// One array of a host form's call: `host` is the caller's (NULL: not asked for), staged through stage[stage] of the scratch, up before the launch or down after it.
struct StagedArray { void* host; size_t record; int stage; bool up; };

// A host form's loop, shared by rt_scene_trace, rt_scene_bake and rt_scene_nearest: at most `chunk` records at a time are staged -- reserve, copy up,
// launch(first, m) on the staged arrays, copy down, wait for the stream, read the walk's status word.
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

int rt_frame_pick(rt_frame* f, uint32_t x, uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface)
{
    if (!f) return fail(nullptr, "rt_frame_pick: frame is NULL");
    rt_ctx* ctx = f->ctx;
    if (!ctx->scene.valid) return fail(ctx, "rt_frame_pick: no scene uploaded");
    if (f->tile.nranks > 1) return fail(ctx, "rt_frame_pick: a tile frame (tile_count > 1): pick on a frame of the whole image");
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

int rt_debug_query_surface(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle, const rt_ray* rays, const rt_hit* hits,
    uint32_t n, rt_surface* out)
{
    if (n == 0u) return RT_OK;
    if (!rays || !hits || !out || (!triangles && num_triangles > 0u)) return fail(ctx, "rt_debug_query_surface: NULL argument");
    if (!ctx) { query::debug_surface_host(triangles, num_triangles, object_of_triangle, rays, hits, n, out); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!query::debug_surface_device(ctx->stream, triangles, num_triangles, object_of_triangle, rays, hits, n, out))
        return fail(ctx, "rt_debug_query_surface: the device path failed (allocation, copy or launch)");
    return RT_OK;
}
