// scene_moved.cpp -- the C entry points of the three producers of moved triangles, the bookkeeping around the kernels and host drivers of pose.hip, skin.hip and
// morph.hip (DESIGN.md sections 7g, 7p, 7q): rt_scene_set_objects .. rt_scene_morph_skin and their rt_debug_* forms.  Host code only, on context.h.  A pose, a
// skin and a morph ARE refits: each writes its state's staging area and hands it to refit_device() (scene_upload.cpp) unchanged.  The three states are
// independent, and the fused rt_scene_morph_skin reads the skin's influences and palette, never its rest pose.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <memory>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "context.h"
#include "pose_host.h"       // the scene's objects posed from one matrix per object (pose.hip)
#include "skin_host.h"       // the scene's triangles skinned from a palette of bone matrices (skin.hip)
#include "morph.h"           // morph::Record
#include "morph_host.h"      // the scene's triangles morphed from one weight per target, alone or fused with the skin (morph.hip)
using namespace context;

// ---- what the producers share ------------------------------------------------------------------------------------------------------------------------
// the report keeps one line that begins with `prefix`, before the refit's own (which is replaced, with all that follows it, by every refit)
static void keep_one_line_before_refit(std::string& r, const char* prefix, const char* line)
{
    auto line_that_begins = [&r](const char* word)                   // only at the start of a line: another line may hold the word
    {
        size_t at = r.find(word);
        while (at != std::string::npos && at != 0 && r[at - 1] != '\n') at = r.find(word, at + 1);
        return at;
    };
    const size_t old = line_that_begins(prefix);
    if (old != std::string::npos) r.erase(old, r.find('\n', old) == std::string::npos ? std::string::npos : r.find('\n', old) - old + 1);
    const size_t at = line_that_begins("refit ");
    r.insert(at == std::string::npos ? r.size() : at, line);
}

// how every rt_scene_set_* ends: the armed state is the scene's, the one it replaces is released, the report says what is kept (`line` begins with `prefix`)
template <class State> static int install(rt_ctx* ctx, State*& slot, std::unique_ptr<State>& armed, const char* prefix, const char* line)
{
    if (slot) { release(*slot); delete slot; }
    slot = armed.release();
    keep_one_line_before_refit(ctx->scene.tree_report, prefix, line);
    return RT_OK;
}

// how every rt_scene_pose / _skin / _morph / _morph_skin ends, once nothing is left to refuse: launch() writes `staged` on ctx's stream, the refit takes it
template <class Launch> static int run_and_refit(rt_ctx* ctx, const char* who, const char* kernel, Launch launch, const rt_triangle* staged)
{
    (void)hipSetDevice(ctx->device);
    if (launch()) return refit_device(ctx, staged, who);
    (void)hipGetLastError();
    return fail(ctx, std::string(who) + ": the " + kernel + " kernel could not be launched");
}

// ---- posed objects -------------------------------------------------------------------------------------------------------------
extern "C" {

int rt_scene_set_objects(rt_ctx* ctx, const uint32_t* object_of_triangle, uint32_t num_triangles, uint32_t num_objects)
{
    if (!ctx || !object_of_triangle) return fail(ctx, "rt_scene_set_objects: NULL argument");
    if (refit_refused(ctx, "rt_scene_set_objects", num_triangles, false) != RT_OK) return RT_ERROR;
    if (num_objects == 0u) return fail(ctx, "rt_scene_set_objects: no objects");
    if (!pose::ids_in_range(object_of_triangle, num_triangles, num_objects)) return fail(ctx, "rt_scene_set_objects: an object index is not below num_objects");
    (void)hipSetDevice(ctx->device);
    Scene& s = ctx->scene;
    std::unique_ptr<pose::State> st(new pose::State());
    if (!pose::arm(ctx->stream, *st, (const float4*)s.tris_sh, object_of_triangle, num_triangles, num_objects))
        return fail(ctx, "rt_scene_set_objects: the rest pose and the staging area could not be allocated");
    char line[300];
    snprintf(line, sizeof(line), "posed objects: %u objects, %u bytes per triangle kept (%.1f MB): rest pose %u + object index %u + staging area %u\n", num_objects,
        (unsigned)pose::BYTES_PER_TRIANGLE, (double)s.n_tris * pose::BYTES_PER_TRIANGLE / 1e6, (unsigned)pose::REST_BYTES, (unsigned)pose::ID_BYTES, (unsigned)pose::STAGED_BYTES);
    return install(ctx, s.pose, st, "posed objects: ", line);
}

int rt_scene_pose(rt_ctx* ctx, const float* matrices3x4, uint32_t num_objects)
{
    if (!ctx || !matrices3x4) return fail(ctx, "rt_scene_pose: NULL argument");
    Scene& s = ctx->scene;
    if (refit_refused(ctx, "rt_scene_pose", s.n_tris, false) != RT_OK) return RT_ERROR;
    if (!s.pose) return fail(ctx, "rt_scene_pose: no objects (rt_scene_set_objects has not been called for this scene)");
    if (num_objects != s.pose->n_objects) return fail(ctx, "rt_scene_pose: the object count differs from rt_scene_set_objects'");
    if (!pose::matrices_finite(matrices3x4, num_objects)) return fail(ctx, "rt_scene_pose: a matrix entry is not finite");
    return run_and_refit(ctx, "rt_scene_pose", "pose", [&] { return pose::run(ctx->stream, *s.pose, matrices3x4); }, s.pose->stage.staged);
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
    return pose::debug_device(ctx->stream, rest, object_of_triangle, num_triangles, matrices3x4, num_objects, out) ? RT_OK
        : fail(ctx, "rt_debug_pose: the device path failed (allocation, copy or launch)");
}

// ---- skinned triangles ---------------------------------------------------------------------------------------------------------

static int skin_table_refused(rt_ctx* ctx, const char* who, const rt_skin_influence* per_corner, uint32_t num_triangles, uint32_t num_bones)
{
    const std::string name(who);
    if (num_bones == 0u) return fail(ctx, name + ": no bones");
    if (num_bones > (uint32_t)skin::MAX_BONES) return fail(ctx, name + ": more than 65536 bones (a bone index is 16 bits)");
    switch (skin::influences_fault(per_corner, num_triangles, num_bones))
    {
    case 0: return RT_OK;
    case 1: return fail(ctx, name + ": a bone index is not below num_bones");
    default: return fail(ctx, name + ": a weight is not finite");
    }
}

// what rt_scene_skin and rt_scene_morph_skin refuse of a palette, before any launch
static int palette_refused(rt_ctx* ctx, const char* who, const float* matrices3x4, uint32_t num_bones)
{
    const std::string name(who);
    const Scene& s = ctx->scene;
    if (!s.skin) return fail(ctx, name + ": no skin (rt_scene_set_skin has not been called for this scene)");
    if (num_bones != s.skin->n_bones) return fail(ctx, name + ": the bone count differs from rt_scene_set_skin's");
    if (!skin::matrices_finite(matrices3x4, num_bones)) return fail(ctx, name + ": a matrix entry is not finite");
    return RT_OK;
}

int rt_scene_set_skin(rt_ctx* ctx, const rt_skin_influence* per_corner, uint32_t num_triangles, uint32_t num_bones)
{
    if (!ctx || !per_corner) return fail(ctx, "rt_scene_set_skin: NULL argument");
    if (refit_refused(ctx, "rt_scene_set_skin", num_triangles, false) != RT_OK) return RT_ERROR;
    if (skin_table_refused(ctx, "rt_scene_set_skin", per_corner, num_triangles, num_bones) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    Scene& s = ctx->scene;
    std::unique_ptr<skin::State> st(new skin::State());
    if (!skin::arm(ctx->stream, *st, (const float4*)s.tris_sh, per_corner, num_triangles, num_bones))
        return fail(ctx, "rt_scene_set_skin: the rest pose, the influences and the staging area could not be allocated");
    char line[300];
    snprintf(line, sizeof(line), "skinned triangles: %u bones, %u bytes per triangle kept (%.1f MB): rest pose %u + influences %u + staging area %u; the palette %u bytes per bone\n",
        num_bones, (unsigned)skin::BYTES_PER_TRIANGLE, (double)s.n_tris * skin::BYTES_PER_TRIANGLE / 1e6, (unsigned)skin::REST_BYTES, (unsigned)skin::INFLUENCE_BYTES,
        (unsigned)skin::STAGED_BYTES, (unsigned)skin::MATRIX_BYTES);
    return install(ctx, s.skin, st, "skinned triangles: ", line);
}

int rt_scene_skin(rt_ctx* ctx, const float* matrices3x4, uint32_t num_bones)
{
    if (!ctx || !matrices3x4) return fail(ctx, "rt_scene_skin: NULL argument");
    Scene& s = ctx->scene;
    if (refit_refused(ctx, "rt_scene_skin", s.n_tris, false) != RT_OK) return RT_ERROR;
    if (palette_refused(ctx, "rt_scene_skin", matrices3x4, num_bones) != RT_OK) return RT_ERROR;
    return run_and_refit(ctx, "rt_scene_skin", "skin", [&] { return skin::run(ctx->stream, *s.skin, matrices3x4); }, s.skin->stage.staged);
}

int rt_debug_skin(rt_ctx* ctx, const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t num_triangles, const float* matrices3x4, uint32_t num_bones,
    rt_triangle* out)
{
    if (!rest || !per_corner || !matrices3x4 || !out) return fail(ctx, "rt_debug_skin: NULL argument");
    if (num_triangles == 0u) return fail(ctx, "rt_debug_skin: no triangles");
    if (skin_table_refused(ctx, "rt_debug_skin", per_corner, num_triangles, num_bones) != RT_OK) return RT_ERROR;
    if (!skin::matrices_finite(matrices3x4, num_bones)) return fail(ctx, "rt_debug_skin: a matrix entry is not finite");
    if (!ctx) { skin::debug_host(rest, per_corner, num_triangles, matrices3x4, num_bones, out); return RT_OK; }
    (void)hipSetDevice(ctx->device);
    return skin::debug_device(ctx->stream, rest, per_corner, num_triangles, matrices3x4, num_bones, out) ? RT_OK
        : fail(ctx, "rt_debug_skin: the device path failed (allocation, copy or launch)");
}

// ---- morphed triangles ---------------------------------------------------------------------------------------------------------

static int morph_table_refused(rt_ctx* ctx, const char* who, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles)
{
    const std::string name(who);
    if (num_targets == 0u) return fail(ctx, name + ": no targets");
    if (num_targets > (uint32_t)morph::MAX_TARGETS) return fail(ctx, name + ": more than 65536 targets");
    if (num_triangles > morph::MAX_TRIANGLES) return fail(ctx, name + ": more than 1431655765 triangles (a corner index is 32 bits)");
    switch (morph::table_fault(deltas, target_offsets, num_targets, num_triangles))
    {
    case morph::TABLE_OK: return RT_OK;
    case morph::FIRST_OFFSET: return fail(ctx, name + ": target_offsets[0] is not 0");
    case morph::DECREASING_OFFSET: return fail(ctx, name + ": target_offsets decrease");
    case morph::BAD_CORNER: return fail(ctx, name + ": a corner is not below 3 * num_triangles");
    case morph::NOT_FINITE: return fail(ctx, name + ": a delta is not finite");
    case morph::BAD_PAD: return fail(ctx, name + ": a delta's pad is not 0");
    case morph::NO_MEMORY: return fail(ctx, name + ": no host memory to check the table");
    default: return fail(ctx, name + ": a target moves the same corner twice");
    }
}

int rt_scene_set_morph(rt_ctx* ctx, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles)
{
    if (!ctx || !deltas || !target_offsets) return fail(ctx, "rt_scene_set_morph: NULL argument");
    if (refit_refused(ctx, "rt_scene_set_morph", num_triangles, false) != RT_OK) return RT_ERROR;
    if (morph_table_refused(ctx, "rt_scene_set_morph", deltas, target_offsets, num_targets, num_triangles) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    Scene& s = ctx->scene;
    std::vector<uint32_t> row;
    std::vector<morph::Record> records;
    if (!morph::transpose(deltas, target_offsets, num_targets, num_triangles, row, records)) return fail(ctx, "rt_scene_set_morph: no host memory for the rows");
    std::unique_ptr<morph::State> st(new morph::State());
    if (!morph::arm(ctx->stream, *st, (const float4*)s.tris_sh, row, records, num_triangles, num_targets))
        return fail(ctx, "rt_scene_set_morph: the rest pose, the records and the staging area could not be allocated");
    char line[300];
    snprintf(line, sizeof(line), "morph targets: %u targets, %u deltas, %.1f MB kept: rest pose %u + staging area %u + row %u bytes per triangle, %u per delta, %u per target\n",
        num_targets, st->n_deltas, (double)st->bytes / 1e6, (unsigned)morph::REST_BYTES, (unsigned)morph::STAGED_BYTES, (unsigned)morph::ROW_BYTES,
        (unsigned)morph::RECORD_BYTES, (unsigned)morph::WEIGHT_BYTES);
    return install(ctx, s.morph, st, "morph targets: ", line);
}

// what rt_scene_morph and rt_scene_morph_skin refuse in common, before any launch
static int morph_refused(rt_ctx* ctx, const char* who, const float* weights, uint32_t num_targets)
{
    const std::string name(who);
    Scene& s = ctx->scene;
    if (refit_refused(ctx, who, s.n_tris, false) != RT_OK) return RT_ERROR;
    if (!s.morph) return fail(ctx, name + ": no morph (rt_scene_set_morph has not been called for this scene)");
    if (num_targets != s.morph->n_targets) return fail(ctx, name + ": the target count differs from rt_scene_set_morph's");
    if (!morph::weights_finite(weights, num_targets)) return fail(ctx, name + ": a weight is not finite");
    return RT_OK;
}

int rt_scene_morph(rt_ctx* ctx, const float* weights, uint32_t num_targets)
{
    if (!ctx || !weights) return fail(ctx, "rt_scene_morph: NULL argument");
    if (morph_refused(ctx, "rt_scene_morph", weights, num_targets) != RT_OK) return RT_ERROR;
    Scene& s = ctx->scene;
    return run_and_refit(ctx, "rt_scene_morph", "morph", [&] { return morph::run(ctx->stream, *s.morph, weights); }, s.morph->stage.staged);
}

int rt_scene_morph_skin(rt_ctx* ctx, const float* weights, uint32_t num_targets, const float* matrices3x4, uint32_t num_bones)
{
    if (!ctx || !weights || !matrices3x4) return fail(ctx, "rt_scene_morph_skin: NULL argument");
    if (morph_refused(ctx, "rt_scene_morph_skin", weights, num_targets) != RT_OK) return RT_ERROR;
    if (palette_refused(ctx, "rt_scene_morph_skin", matrices3x4, num_bones) != RT_OK) return RT_ERROR;
    Scene& s = ctx->scene;
    return run_and_refit(ctx, "rt_scene_morph_skin", "morph-and-skin", [&]
        {
            return skin::upload_palette(ctx->stream, *s.skin, matrices3x4) &&
                   morph::run_skin(ctx->stream, *s.morph, weights, s.skin->influences, s.skin->palette, num_bones);
        }, s.morph->stage.staged);
}

static int debug_morph_refused(rt_ctx* ctx, const char* who, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles,
    const float* weights)
{
    const std::string name(who);
    if (num_triangles == 0u) return fail(ctx, name + ": no triangles");
    if (morph_table_refused(ctx, who, deltas, target_offsets, num_targets, num_triangles) != RT_OK) return RT_ERROR;
    if (!morph::weights_finite(weights, num_targets)) return fail(ctx, name + ": a weight is not finite");
    return RT_OK;
}

int rt_debug_morph(rt_ctx* ctx, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles,
    const float* weights, rt_triangle* out)
{
    if (!rest || !deltas || !target_offsets || !weights || !out) return fail(ctx, "rt_debug_morph: NULL argument");
    if (debug_morph_refused(ctx, "rt_debug_morph", deltas, target_offsets, num_targets, num_triangles, weights) != RT_OK) return RT_ERROR;
    if (!ctx) return morph::debug_host(rest, deltas, target_offsets, num_targets, num_triangles, weights, out) ? RT_OK : fail(ctx, "rt_debug_morph: no host memory for the rows");
    (void)hipSetDevice(ctx->device);
    return morph::debug_device(ctx->stream, rest, deltas, target_offsets, num_targets, num_triangles, weights, out) ? RT_OK
        : fail(ctx, "rt_debug_morph: the device path failed (allocation, copy or launch)");
}

int rt_debug_morph_skin(rt_ctx* ctx, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles,
    const float* weights, const rt_skin_influence* per_corner, const float* matrices3x4, uint32_t num_bones, rt_triangle* out)
{
    if (!rest || !deltas || !target_offsets || !weights || !per_corner || !matrices3x4 || !out) return fail(ctx, "rt_debug_morph_skin: NULL argument");
    if (debug_morph_refused(ctx, "rt_debug_morph_skin", deltas, target_offsets, num_targets, num_triangles, weights) != RT_OK) return RT_ERROR;
    if (skin_table_refused(ctx, "rt_debug_morph_skin", per_corner, num_triangles, num_bones) != RT_OK) return RT_ERROR;
    if (!skin::matrices_finite(matrices3x4, num_bones)) return fail(ctx, "rt_debug_morph_skin: a matrix entry is not finite");
    if (!ctx)
    {
        if (!morph::debug_host(rest, deltas, target_offsets, num_targets, num_triangles, weights, out)) return fail(ctx, "rt_debug_morph_skin: no host memory for the rows");
        skin::debug_host(out, per_corner, num_triangles, matrices3x4, num_bones, out);           // (triangle by triangle, each read before it is written)
        return RT_OK;
    }
    (void)hipSetDevice(ctx->device);
    return morph::debug_skin_device(ctx->stream, rest, deltas, target_offsets, num_targets, num_triangles, weights, per_corner, matrices3x4, num_bones, out) ? RT_OK
        : fail(ctx, "rt_debug_morph_skin: the device path failed (allocation, copy or launch)");
}

} // extern "C"
