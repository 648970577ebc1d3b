// region_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after within_impl.h): rt_scene_overlap /
// rt_scene_overlap_buffer / rt_scene_select / rt_scene_select_buffer / rt_frame_pick_rect / rt_debug_overlap / rt_debug_overlap_walk / rt_debug_select /
// rt_debug_rect_region, the bookkeeping around region.hip's kernels.  Like a within query, an overlap query reads the scene and writes
// the caller's arrays: it launches on the context's stream -- behind every refit, pose and upload, which end there -- and touches no frame.  Its stack spill
// area, status word and staging arrays are the ray queries' (ctx->query).

// everything both overlap forms refuse before anything is launched
static int overlap_refused(rt_ctx* ctx, const char* who, bool regions, uint32_t n, uint32_t max_list, bool out, bool members)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (!regions && n > 0u) return fail(ctx, name + ": regions is NULL");
    if (!out) return fail(ctx, name + ": out is NULL");
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
    if (!ctx) { region::brute_host(triangles, num_triangles, regions, n, max_list, out, members); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!region::brute_device(ctx->stream, triangles, num_triangles, regions, n, max_list, out, members))
        return fail(ctx, "rt_debug_overlap: the device path failed (allocation, copy or launch)");
    return RT_OK;
}

int rt_debug_overlap_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_region* regions,
    uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members, uint32_t* triangles_tested)
{
    if (n == 0u) return RT_OK;
    if (max_list > RT_REGION_LIST_MAX) return fail(nullptr, "rt_debug_overlap_walk: max_list is above RT_REGION_LIST_MAX");
    if (!nodes || num_nodes == 0u || !triangles || !regions || !out || (!members && max_list > 0u)) return fail(nullptr, "rt_debug_overlap_walk: NULL argument");
    if (wide != 0 && wide != 1) return fail(nullptr, "rt_debug_overlap_walk: wide must be 0 (the child-pair form) or 1 (the 4-wide records)");
    if (const char* why = region::walk_host(nodes, num_nodes, triangles, num_triangles, wide != 0, regions, n, max_list, out, members, triangles_tested))
        return fail(nullptr, std::string("rt_debug_overlap_walk: ") + why);
    return RT_OK;
}

// everything both select forms refuse before anything is launched
static int select_refused(rt_ctx* ctx, const char* who, bool regions, uint32_t n, bool per_triangle, bool per_object)
{
    const std::string name(who);
    if (!ctx) return fail(nullptr, name + ": ctx is NULL");
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene uploaded");
    if (!regions) return fail(ctx, name + ": regions is NULL");
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
    if (!ctx) { region::select_host(triangles, num_triangles, object_of_triangle, num_objects, regions, n, touching, inside, object_touching, object_inside); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!region::select_device(ctx->stream, triangles, num_triangles, object_of_triangle, num_objects, regions, n, touching, inside, object_touching, object_inside))
        return fail(ctx, "rt_debug_select: the device path failed (allocation, copy or launch)");
    return RT_OK;
}

static const char* rect_refused(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (x1 < x0 || y1 < y0) return "an empty rectangle (x1 < x0 or y1 < y0)";
    if (x1 >= width || y1 >= height) return "the rectangle is outside the image";
    return nullptr;
}

int rt_debug_rect_region(const rt_camera* camera, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far,
    rt_region* out)
{
    if (!camera || !out) return fail(nullptr, "rt_debug_rect_region: NULL argument");
    if (const char* why = rect_refused(width, height, x0, y0, x1, y1)) return fail(nullptr, std::string("rt_debug_rect_region: ") + why);
    *out = region::rect_region(*camera, width, height, x0, y0, x1, y1, t_near, t_far);
    return RT_OK;
}

int rt_frame_pick_rect(rt_frame* f, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far, rt_region* region, uint32_t* touching,
    uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    if (!f) return fail(nullptr, "rt_frame_pick_rect: frame is NULL");
    rt_ctx* ctx = f->ctx;
    if (!ctx->scene.valid) return fail(ctx, "rt_frame_pick_rect: no scene uploaded");
    if (f->tile.nranks > 1) return fail(ctx, "rt_frame_pick_rect: a tile frame (tile_count > 1): pick on a frame of the whole image");
    if (const char* why = rect_refused(f->tile.width, f->tile.height, x0, y0, x1, y1)) return fail(ctx, std::string("rt_frame_pick_rect: ") + why);
    if ((object_touching || object_inside) && !ctx->scene.pose) return fail(ctx, "rt_frame_pick_rect: the per-object outputs need rt_scene_set_objects");
    const rt_region g = region::rect_region(f->camera, f->tile.width, f->tile.height, x0, y0, x1, y1, t_near, t_far);
    if ((touching || inside || object_touching || object_inside) && rt_scene_select(ctx, &g, 1u, touching, inside, object_touching, object_inside) != RT_OK) return RT_ERROR;
    if (region) *region = g;
    return RT_OK;
}
