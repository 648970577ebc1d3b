// refit_impl.h -- part of rt_hip.hip's translation unit (included inside its extern "C" block): rt_scene_refit / rt_scene_refit_buffer / rt_debug_refit, the
// bookkeeping around refit.hip's kernels.  After a successful refit the context behaves as a fresh one would after rt_scene_upload of
// the moved triangles with the node array "same topology, same split axes, bounds refitted".

// RT_CTX_OPT_REFITTABLE at the end of rt_scene_upload: the links of the child-pair records and of the 4-wide trees the scene starts with
static bool refit_link_trees(rt_ctx* ctx);
static void refit_arm(rt_ctx* ctx, const rt_scene_desc* sd, uint32_t n_pairs)
{
    Scene& s = ctx->scene;
    s.refit_wide_built = s.wide_ok;
    s.n_materials = sd->num_materials;
    if (!refit::leaves_partition(sd->nodes, sd->num_nodes, sd->num_triangles)) { s.refit_refusal = "the leaves of the uploaded node array are not consecutive ranges that cover the triangle array"; return; }
    s.refit = new refit::State();
    if (!refit::prepare(ctx->stream, *s.refit, (const float4*)s.nodes, n_pairs) || !refit_link_trees(ctx) || hipStreamSynchronize(ctx->stream) != hipSuccess)
    {
        (void)hipGetLastError();
        refit::release(*s.refit); delete s.refit; s.refit = nullptr;
        s.refit_refusal = "the refit state could not be allocated at upload";
    }
    if (!s.refit || !ctx->refit_motion) return;
    // RT_CTX_OPT_REFIT_MOTION: room for the pose a refit replaces; without it the option is off for this scene
    char line[200];
    if (hipMalloc(&s.pose_snap, (size_t)s.n_tris * 96u) != hipSuccess)
    {
        (void)hipGetLastError();
        s.pose_snap = nullptr;
        snprintf(line, sizeof(line), "previous pose: could not be allocated at upload, RT_CTX_OPT_REFIT_MOTION is treated as off\n");
    }
    else snprintf(line, sizeof(line), "previous pose: RT_CTX_OPT_REFIT_MOTION keeps 96 bytes per triangle (%.1f MB)\n", (double)s.n_tris * 96.0 / 1e6);
    s.tree_report += line;
}

// the 4-wide trees the scene holds NOW (an adaptation or rt_scene_import_folds may have replaced the records since the links were made)
static bool refit_link_trees(rt_ctx* ctx)
{
    Scene& s = ctx->scene;
    const WideTree &ref = s.trees[TREE_REF], &sh = s.trees[TREE_SHADOW];
    const bool wide = s.refit_wide_built && ref.recs && ref.n != 0u;
    const bool own_sh = wide && s.shadow == TREE_SHADOW && sh.recs && sh.n != 0u;           // tree 1: only records of the shadow rays' own
    return refit::link_tree(ctx->stream, *s.refit, 0, wide ? (WideNode*)ref.recs : nullptr, ref.n, s.d.w_entry_ref) &&
           refit::link_tree(ctx->stream, *s.refit, 1, own_sh ? (WideNode*)sh.recs : nullptr, sh.n, s.d.w_sh_entry_ref);
}

static int refit_device(rt_ctx* ctx, const rt_triangle* d_tris, const char* who)
{
    Scene& s = ctx->scene;
    const std::string name(who);
    // read-only first: a refused refit leaves the scene untouched
    switch (refit::validate(ctx->stream, *s.refit, d_tris, s.n_tris, s.n_materials))
    {
    case refit::OK: break;
    case refit::BAD_POSITION: return fail(ctx, name + ": a triangle has a non-finite position");
    case refit::BAD_MATERIAL: return fail(ctx, name + ": material index out of range");
    default: (void)hipGetLastError(); return fail(ctx, name + ": the validation kernel failed");
    }
    if (quiesce(ctx) != RT_OK) return RT_ERROR;                            // nothing may still read what is about to be rewritten
    // an adaptation's host copies (the binary trees, the triangles' corners) are stale from here on: it is retired -- one in flight is cancelled and waited
    // for -- and the records adapted so far stay in use
    const bool had_adapt = s.adapt != nullptr;
    if (s.adapt) { drop_fold_adapt(s.adapt); s.adapt = nullptr; (void)hipSetDevice(ctx->device); }
    // RT_CTX_OPT_REFIT_MOTION: the pose about to be replaced, while the shading records still hold it
    if (s.pose_snap)
    {
        s.pose_valid = false;
        HIPCHK(ctx, filt::snapshot_pose(ctx->stream, (const float4*)s.tris_sh, s.n_tris, (float4*)s.pose_snap));
    }
    const auto t0 = std::chrono::steady_clock::now();
    refit::Result res;
    if (!refit_link_trees(ctx) ||
        !refit::run(ctx->stream, *s.refit, d_tris, s.n_tris, (float4*)s.tris_rt, (float4*)s.tris_sh, (float4*)s.nodes, s.d.entry_ref, res) || res.error != refit::OK)
    {
        (void)hipGetLastError();
        s.valid = false;                                                   // half-written records: upload again
        return fail(ctx, name + ": the refit kernels failed; the scene is no longer valid, upload it again");
    }
    for (int k = 0; k < 3; ++k) { s.d.root_min[k] = res.root_min[k]; s.d.root_max[k] = res.root_max[k]; }
    // a record that no longer qualifies for k_trace_w4: the BVH2 kernels, as upload does for such trees; a later refit that qualifies switches back
    const bool fallback = s.refit_wide_built && (res.wide_bad[0] || res.wide_bad[1]);
    s.wide_ok = s.refit_wide_built && !fallback;
    ++ctx->scene_uploads;                                                  // guide caches, temporal histories, measured choices: dropped as on upload
    ++s.refits;
    ++ctx->refit_index;
    s.pose_valid = s.pose_snap != nullptr;
    {
        char pose[96] = "";
        if (s.pose_snap) snprintf(pose, sizeof(pose), " + %.1f MB for the previous pose, 96 bytes per triangle", (double)s.n_tris * 96.0 / 1e6);
        char line[500];
        snprintf(line, sizeof(line), "refit %llu: %.3f ms on the device (%u triangles, %u child-pair records, %u + %u wide records, %.1f MB kept for it%s); %s; %s\n",
            (unsigned long long)s.refits, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), s.n_tris, s.refit->n_pairs,
            s.refit->trees[0].n, s.refit->trees[1].n, (double)s.refit->bytes / 1e6, pose,
            fallback ? "a 4-wide record no longer qualifies -> the BVH2 kernels until a refit qualifies again" : (s.refit_wide_built ? "the 4-wide trees qualify" : "no 4-wide tree"),
            had_adapt || s.adapt_retired ? "the fold adaptation is retired (the records adapted so far stay)" : "no fold adaptation");
        s.adapt_retired = s.adapt_retired || had_adapt;
        replace_report_line(s.tree_report, "refit ", line);
    }
    return RT_OK;
}

static int refit_refused(rt_ctx* ctx, const char* who, uint64_t count_or_bytes, bool bytes)
{
    const std::string name(who);
    Scene& s = ctx->scene;
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene");
    if (!s.refit) return fail(ctx, name + (s.refit_refusal.empty() ? ": RT_CTX_OPT_REFITTABLE was off when the scene was uploaded" : ": " + s.refit_refusal));
    if (ctx->closest_tree != 0u || s.trees[TREE_CLOSEST].recs) return fail(ctx, name + ": not in the tolerance mode (RT_CTX_OPT_CLOSEST_TREE != 0)");
    if (bytes ? count_or_bytes != (uint64_t)s.n_tris * sizeof(rt_triangle) : count_or_bytes != s.n_tris)
        return fail(ctx, name + ": the triangle count differs from the uploaded scene's");
    return RT_OK;
}

int rt_scene_refit_buffer(rt_ctx* ctx, rt_buffer* triangles)
{
    if (!ctx || !triangles) return fail(ctx, "rt_scene_refit_buffer: NULL argument");
    if (triangles->ctx != ctx) return fail(ctx, "rt_scene_refit_buffer: the buffer belongs to another context");
    if (refit_refused(ctx, "rt_scene_refit_buffer", triangles->bytes, true) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return refit_device(ctx, (const rt_triangle*)triangles->ptr, "rt_scene_refit_buffer");
}

int rt_scene_refit(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles)
{
    if (!ctx || !triangles) return fail(ctx, "rt_scene_refit: NULL argument");
    if (refit_refused(ctx, "rt_scene_refit", num_triangles, false) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    dev::Mem d_tris;
    if (dev_fill(ctx, "rt_scene_refit", d_tris, triangles, (size_t)num_triangles * sizeof(rt_triangle)) != RT_OK) return RT_ERROR;
    const int rc = refit_device(ctx, d_tris.get<const rt_triangle>(), "rt_scene_refit");
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int rt_debug_refit(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, const void* records, uint32_t num_records,
    uint32_t entry_ref, rt_bvh_node* out_nodes, void* out_records)
{
    std::string error;
    bool bad = false;
    if (ctx) (void)hipSetDevice(ctx->device);
    const bool ok = ctx ? refit::debug_device(ctx->stream, nodes, num_nodes, triangles, num_triangles, (const WideNode*)records, num_records, entry_ref, out_nodes, (WideNode*)out_records, &bad, error)
                        : refit::debug_host(nodes, num_nodes, triangles, num_triangles, (const WideNode*)records, num_records, entry_ref, out_nodes, (WideNode*)out_records, &bad, error);
    if (!ok) return fail(ctx, "rt_debug_refit: " + error);
    return bad ? RT_REFIT_DISQUALIFIED : RT_OK;
}
