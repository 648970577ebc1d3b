// pose_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block, after refit_impl.h): rt_scene_set_objects / rt_scene_pose /
// rt_debug_pose, the bookkeeping around pose.hip's kernels.  A pose IS a refit: rt_scene_pose writes the posed triangles into the staging
// area rt_scene_set_objects allocated and hands it to refit_device() unchanged.

int rt_scene_set_objects(rt_ctx* ctx, const uint32_t* object_of_triangle, uint32_t num_triangles, uint32_t num_objects)
{
    if (!ctx || !object_of_triangle) return fail(ctx, "rt_scene_set_objects: NULL argument");
    if (refit_refused(ctx, "rt_scene_set_objects", num_triangles, false) != RT_OK) return RT_ERROR;
    if (num_objects == 0u) return fail(ctx, "rt_scene_set_objects: no objects");
    if (!pose::ids_in_range(object_of_triangle, num_triangles, num_objects)) return fail(ctx, "rt_scene_set_objects: an object index is not below num_objects");
    (void)hipSetDevice(ctx->device);
    Scene& s = ctx->scene;
    pose::State* st = new pose::State();
    if (!pose::arm(ctx->stream, *st, (const float4*)s.tris_sh, object_of_triangle, num_triangles, num_objects))
    {
        delete st;
        return fail(ctx, "rt_scene_set_objects: the rest pose and the staging area could not be allocated");
    }
    if (s.pose) { pose::release(*s.pose); delete s.pose; }
    s.pose = st;
    // the report keeps one such line, before the refit's own (which is replaced, with all that follows it, by every refit)
    char line[300];
    snprintf(line, sizeof(line), "posed objects: %u objects, %u bytes per triangle kept (%.1f MB): rest pose %u + object index %u + staging area %u\n", num_objects,
        (unsigned)pose::BYTES_PER_TRIANGLE, (double)s.n_tris * pose::BYTES_PER_TRIANGLE / 1e6, (unsigned)pose::REST_BYTES, (unsigned)pose::ID_BYTES, (unsigned)pose::STAGED_BYTES);
    std::string& r = s.tree_report;
    auto line_that_begins = [&r](const char* prefix)                 // only at the start of a line: another line may hold the word
    {
        size_t at = r.find(prefix);
        while (at != std::string::npos && at != 0 && r[at - 1] != '\n') at = r.find(prefix, at + 1);
        return at;
    };
    const size_t old = line_that_begins("posed objects: ");
    if (old != std::string::npos) r.erase(old, r.find('\n', old) == std::string::npos ? std::string::npos : r.find('\n', old) - old + 1);
    const size_t at = line_that_begins("refit ");
    r.insert(at == std::string::npos ? r.size() : at, line);
    return RT_OK;
}

int rt_scene_pose(rt_ctx* ctx, const float* matrices3x4, uint32_t num_objects)
{
    if (!ctx || !matrices3x4) return fail(ctx, "rt_scene_pose: NULL argument");
    Scene& s = ctx->scene;
    if (refit_refused(ctx, "rt_scene_pose", s.n_tris, false) != RT_OK) return RT_ERROR;
    if (!s.pose) return fail(ctx, "rt_scene_pose: no objects (rt_scene_set_objects has not been called for this scene)");
    if (num_objects != s.pose->n_objects) return fail(ctx, "rt_scene_pose: the object count differs from rt_scene_set_objects'");
    if (!pose::matrices_finite(matrices3x4, num_objects)) return fail(ctx, "rt_scene_pose: a matrix entry is not finite");
    (void)hipSetDevice(ctx->device);
    if (!pose::run(ctx->stream, *s.pose, matrices3x4))
    {
        (void)hipGetLastError();
        return fail(ctx, "rt_scene_pose: the pose kernel could not be launched");
    }
    return refit_device(ctx, s.pose->staged, "rt_scene_pose");
}

int rt_debug_pose(rt_ctx* ctx, const rt_triangle* rest, const uint32_t* object_of_triangle, uint32_t num_triangles, const float* matrices3x4, uint32_t num_objects,
    rt_triangle* out)
{
    if (!rest || !object_of_triangle || !matrices3x4 || !out) return fail(ctx, "rt_debug_pose: NULL argument");
    if (num_triangles == 0u) return fail(ctx, "rt_debug_pose: no triangles");
    if (num_objects == 0u) return fail(ctx, "rt_debug_pose: no objects");
    if (!pose::ids_in_range(object_of_triangle, num_triangles, num_objects)) return fail(ctx, "rt_debug_pose: an object index is not below num_objects");
    if (!pose::matrices_finite(matrices3x4, num_objects)) return fail(ctx, "rt_debug_pose: a matrix entry is not finite");
    if (!ctx) { pose::debug_host(rest, object_of_triangle, num_triangles, matrices3x4, num_objects, out); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    if (!pose::debug_device(ctx->stream, rest, object_of_triangle, num_triangles, matrices3x4, num_objects, out))
        return fail(ctx, "rt_debug_pose: the device path failed (allocation, copy or launch)");
    return RT_OK;
}
