/* rt_hip.h -- C-ABI of the MI355X (gfx950) wavefront path-tracing backend.
 *
 * This library is the drop-in replacement for the reference's OpenCL wrapper
 * layer src/gpu_wrappers/cl_context.{hpp,cpp} (CLContext / CLKernel) together
 * with the device half of src/integrator/cl_pt_integrator.{hpp,cpp} (the
 * buffers it owns and the 11 kernels it launches).  A reference-side
 * `HIPPathTraceIntegrator : Integrator` binds these entry points one to one
 * (this repo ships that class in raytracing_amd/host/).
 *
 * Conventions: every function returns 0 on success, non-zero on failure; the
 * message is available from rt_last_error() (replaces the thrown CLException,
 * src/utils/cl_exception.hpp:109-123 -- the C++ host shim rethrows).  Plain
 * pointers and sizes only; records are the PODs of rt_types.h.  One HIP stream
 * per context with in-order semantics, like the reference's single in-order
 * command queue (cl_context.cpp:89).  No call synchronises with the host
 * except rt_finish, rt_buffer_read, rt_frame_read_* and rt_frame_get_stats.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERROR 1
#define RT_MAX_BOUNCES_LIMIT 62u

typedef struct rt_ctx rt_ctx;        /* CLContext, cl_context.hpp:37-65 */
typedef struct rt_buffer rt_buffer;  /* cl::Buffer */
typedef struct rt_frame rt_frame;    /* per-integrator device state, cl_pt_integrator.hpp:80-120 */

/* ---- context: CLContext::CLContext / Finish (cl_context.cpp:47-94, hpp:49) */
int rt_ctx_create(int device_ordinal, rt_ctx** out);
int rt_ctx_destroy(rt_ctx* ctx);
int rt_finish(rt_ctx* ctx);
/* last error message of `ctx`, or of the calling thread when ctx == NULL */
const char* rt_last_error(rt_ctx* ctx);
/* device name / CU count (the device info dump of cl_context.cpp:70-83) */
int rt_ctx_device_info(rt_ctx* ctx, char* name, size_t name_len, int* compute_units, size_t* hbm_bytes);
/* the hipStream_t of this context (for interop with other HIP libraries) */
void* rt_ctx_stream(rt_ctx* ctx);
/* Page-lock a caller-owned host buffer (and release it): read-backs into it -- rt_frame_resolve every frame in the
 * reference's call pattern (cl_pt_integrator.cpp:677-684 has the GL image for that; headless there is only the host) --
 * then run at the PCIe rate instead of through the runtime's staging copies.  Optional: every entry point works with
 * pageable memory. */
int rt_host_register(rt_ctx* ctx, void* host_ptr, size_t bytes);
int rt_host_unregister(rt_ctx* ctx, void* host_ptr);
/* context options, effective at the next rt_scene_upload */
enum rt_ctx_option
{
    RT_CTX_OPT_TREELET_NODES = 0   /* BVH record layout: interior nodes per contiguous breadth-first cluster
                                      (default 7; 1 = the reference's depth-first order).  Layout only. */
    , RT_CTX_OPT_WIDE_BVH = 1      /* 1 (default): also build the 4-wide quantized tree of k_trace_w4, each 64-byte record
                                      folding the SAH-optimal frontier of up to four BVH2 nodes; 2: two BVH2 levels per
                                      record (round 2's rule); 0: BVH2 records only */
    , RT_CTX_OPT_SHADOW_TREE = 2   /* 1 (default): shadow rays walk a 4-wide tree of the backend's own where that is cheaper --
                                      built over the reference's LEAVES (src/bvh.cpp:67-221 fixes only those for an any-hit
                                      query) by a full-sweep SAH on the projected area along the scene's directional lights
                                      (+ 50 % isotropic; surface area when there are only point lights); rt_scene_upload
                                      walks it and the reference's topology with proxy shadow rays and keeps the own tree if it
                                      saves more than 10 % of the steps (rt_scene_tree_report).  Verdicts equal TraceBvh
                                      -DSHADOW_RAYS bit for bit on either (trace_bvh.cl:107-109,164-167).  2: the own tree
                                      unconditionally; 3: the own tree with the surface-area metric (A/B); 0: shadow rays share
                                      the closest-hit tree */
    , RT_CTX_OPT_CLOSEST_TREE = 3  /* 0 (default): closest-hit rays walk the reference's topology in the reference's order
                                      (bit-identical radiance).  1 (measured like the shadow tree) / 2 (unconditionally):
                                      TOLERANCE MODE -- they walk an own surface-area tree, near child first on ITS split axes:
                                      the hit differs from TraceBvh's where two candidate hits tie within the rounding of
                                      RayTriangle (trace_bvh.cl:157-162); validated by rel-L2 < 1e-4 and a differing-pixel
                                      count against oracle/_ref, never the default */
    , RT_CTX_OPT_ADAPTIVE_FOLD = 4 /* The 4-wide trees start with the fold rt_scene_upload makes (optimal for the surface-area visit
                                      probability).  Default 25 = bits 0 + 3 + 4.  Bit 0: the first rt_integrate of an uploaded scene
                                      traces a small probe frame through the stage API (same camera, 1/k of the resolution, ~32 K paths),
                                      the host counts how often those rays pass each box of the binary tree, and a worker thread folds both
                                      4-wide trees again to be optimal for THOSE frequencies; the new records replace the old ones
                                      between two rt_integrate calls once they are ready, and again when a frame's camera has
                                      left the view they were made for (3 % of the scene's diagonal, 20 degrees, a tenth of the
                                      field of view) -- at most once per RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS.  EXACT: a fold decides
                                      which interior boxes are tested, never a hit or a verdict.  Bit 1:
                                      rt_integrate waits for the new fold (reproducible timing: bench.py, tests).  Bit 2: also for
                                      trees of fewer than 8192 nodes (tests).  Bit 3: the shadow rays' BINARY tree is first rotated for
                                      the probe rays' measured crossings (tree_rotate.h) -- any tree over the reference's leaves gives
                                      an any-hit query the reference's verdict.  Bit 4: the slots of every shadow record are stored
                                      likeliest occluder first -- k_trace_w4<shadow> looks at them in stored order, an any-hit
                                      verdict is an OR, an occluded ray stops at its first hit; the host finds the probe rays' nearest
                                      occluders itself and keeps the triangles' positions for that (36 bytes each).  Measured on the
                                      device in round 5 (profiles/r05_call01_*): bits 3 + 4 take the shadow trace of the headline scene
                                      from 0.314 to 0.258 ms per sample (6711 -> 6917 Mrays/s), every config's frame bit-identical.
                                      0: off.
                                      Takes effect at the next rt_scene_upload; rt_scene_tree_report carries the latest
                                      adaptation's line.  Costs: a host copy of the binary tree(s), 48 bytes per node, for as long
                                      as the scene lives; per adaptation a probe frame's launches on the context's stream (nothing
                                      waits for them: the queues come back through pinned memory, the worker uploads the new
                                      records itself and rt_integrate only exchanges pointers); the worker gives up within
                                      milliseconds when the scene is uploaded again. */
    , RT_CTX_OPT_ADAPT_MIN_INTERVAL_MS = 5 /* default 500: a camera that keeps leaving the adapted view (an orbit) starts at most one
                                      fold adaptation per this many milliseconds (bit 1 of RT_CTX_OPT_ADAPTIVE_FOLD -- wait for every
                                      adaptation: tests, bench.py -- is not rate-limited).  Takes effect at once. */
    , RT_CTX_OPT_DEVICE_FOLD = 7   /* 1 (default): the collapse of a binary tree into the 4-wide records of k_trace_w4 -- the dynamic programme over node x slots,
                                      the record roots, the slots' placement, the quantised boxes -- runs on the DEVICE (raytracing_amd/csrc/fold_kernels.h:
                                      five kernels; the reference's tree at rt_scene_upload, the shadow rays' own tree, and every re-fold of an
                                      adaptation, whose crossing counts are a device kernel too); 0: on host threads (build_wide_bvh, the same algorithm:
                                      the two are compared record for record in tests/test_gpu_device_fold.py, and the host's is the fallback when the device
                                      path fails).  Results do not depend on it.  Takes effect at the next rt_scene_upload. */
    , RT_CTX_OPT_TREE_BUILDER = 9  /* who builds the shadow rays' own binary tree (RT_CTX_OPT_SHADOW_TREE).  0: own_bvh.h's full-sweep SAH on host threads (rounds 4 - 5).  1: the DEVICE --
                                      PLOC (parallel locally-ordered clustering, Meister & Bittner 2017) over the reference's leaves in Morton order, the tree's own metric (projected
                                      area along the directional lights + an isotropic share) as the merge cost, then the same fold where the tree lies (raytracing_amd/csrc/ploc_kernels.h):
                                      0.38 -> 0.09 s for 2.45 M leaves, 1.7 -> 0.26 s for 8.7 M.  2 (default): both start; the device's candidate is ready first and is measured first
                                      (proxy rays, rt_scene_tree_report); if it wins that measurement the host's build is abandoned, otherwise the host's candidate is waited for and
                                      measured as before -- never a worse tree than rounds 4 - 5 chose, and the upload of the headline scene 0.54 -> 0.24 s.  Any binary tree over the
                                      reference's leaves gives an any-hit query the reference's verdict.  Takes effect at the next rt_scene_upload. */
    , RT_CTX_OPT_WIDE_LAYOUT = 8   /* 0: the 4-wide records in the fold's own (depth-first) order; 1: in PAIRS -- every record with interior slots at an even index,
                                      the child it hands most rays on to right behind it, i.e. in the same 128-byte line (the L2 of gfx950 fetches whole lines:
                                      a 64-byte record that misses pays for its line-mate anyway).  A permutation of the records: no result depends on it.
                                      Takes effect at the next rt_scene_upload. */
    , RT_CTX_OPT_REFITTABLE = 10   /* 0 (default): a scene's triangles move only by rt_scene_upload again; nothing is kept, rt_scene_refit* is refused.
                                      1: rt_scene_upload keeps what a refit needs on the device -- who holds each child-pair record and each 4-wide record,
                                      the exact box of every 4-wide record, arrival counters: 8 bytes per child-pair record + 40 per 4-wide record, about 34 bytes
                                      per triangle.  Upload's results, trees and report are the same either way.  Takes effect at the
                                      next rt_scene_upload. */
    , RT_CTX_OPT_REFIT_MOTION = 11 /* 0 (default): a refit drops every temporal filter history, as an upload does; nothing is kept or allocated.
                                      1 (needs RT_CTX_OPT_REFITTABLE = 1; without it nothing is allocated and the refit calls stay refused): rt_scene_upload
                                      allocates room for ONE previous pose -- three positions and three shading normals per triangle, the first six float4 of
                                      the shading record, 96 bytes per triangle -- and every successful refit first copies the pose it is about to replace
                                      there.  rt_frame_filter_temporal then follows the moved surfaces instead of dropping its history (see there; DESIGN.md
                                      section 7f).  If the room cannot be allocated the option is treated as off and rt_scene_tree_report says so.  Every
                                      other result is the same either way.  Takes effect at the next rt_scene_upload. */
    , RT_CTX_OPT_ADAPT_WAIT = 6    /* 1 / 0: sets / clears bit 1 of RT_CTX_OPT_ADAPTIVE_FOLD (rt_integrate waits for an adaptation it has
                                      started) for the scene IN PLACE, at once; the context's option, which the next upload reads, stays
                                      (bench.py: the headline waits for its fold, the moving-camera leg runs as the library ships) */
    , RT_CTX_OPT_BAKE_CHUNK_POINTS = 12 /* rt_scene_bake stages at most this many points at a time (default and upper bound 1 Mi; 0 = the default).  No result
                                      depends on it (tests force it small).  Takes effect at once. */
};
int rt_ctx_set_option(rt_ctx* ctx, int option, uint32_t value);
/* The blue-noise sampler tables (src/utils/blue_noise_sampler.hpp: sobol_256spp_256d[256*256],
 * scramblingTile[128*128*8], rankingTile[128*128*8], values 0..255) that CLPathTraceIntegrator
 * uploads in its ctor (cl_pt_integrator.cpp:222-235).  Required before RT_OPT_SAMPLER = 1. */
int rt_upload_blue_noise_tables(rt_ctx* ctx, const int* sobol_256spp_256d, const int* scramblingTile,
    const int* rankingTile);

/* ---- buffers: cl::Buffer(ctx, flags, size, host_ptr) (cl_pt_integrator.cpp:178-186)
 *      WriteBuffer / ReadBuffer / CopyBuffer (cl_context.cpp:96-113).
 *      rt_buffer_read is BLOCKING (the reference's ReadBuffer is non-blocking
 *      and never waited on, a latent race this ABI does not reproduce). */
int rt_buffer_create(rt_ctx* ctx, size_t bytes, const void* init_or_null, rt_buffer** out);
int rt_buffer_destroy(rt_buffer* buf);
int rt_buffer_write(rt_buffer* buf, size_t offset, const void* src, size_t bytes);
int rt_buffer_read(rt_buffer* buf, size_t offset, void* dst, size_t bytes);
int rt_buffer_copy(rt_buffer* src, rt_buffer* dst, size_t src_offset, size_t dst_offset, size_t bytes);
void* rt_buffer_device_ptr(rt_buffer* buf);
size_t rt_buffer_size(rt_buffer* buf);

/* ---- scene: CLPathTraceIntegrator::UploadGPUData (cl_pt_integrator.cpp:373-456)
 * Host arrays in the reference's layouts; the device re-layout (child-pair BVH
 * nodes, pre-differenced trace triangles, 128-byte shading records) happens
 * behind this call.  Arrays are copied; the caller keeps ownership. */
typedef struct rt_scene_desc
{
    const rt_triangle* triangles;         uint32_t num_triangles;   /* Scene::GetTriangles(), BVH order */
    const rt_bvh_node* nodes;             uint32_t num_nodes;       /* AccelerationStructure::GetNodes() */
    const rt_packed_material* materials;  uint32_t num_materials;
    const rt_texture* textures;           uint32_t num_textures;
    const uint32_t* texture_data;         uint32_t num_texture_data;
    const rt_light* lights;               uint32_t num_lights;
    const uint32_t* emissive_indices;     uint32_t num_emissive;    /* uploaded, unused (hit_surface.cl:39) */
    const float* env_rgba;                uint32_t env_width, env_height;  /* Scene::GetEnvImage(), float RGBA */
    /* ---- opt-in extensions.  NULL / 0 = the reference's behaviour, bit for bit. ---- */
    const uint16_t* material_texture_indices;   /* 6 per material -- diffuse, specular, roughness, metalness, emission,
                                                   transparency; 0xFFFF = none.  When given, these replace the 8-bit texture
                                                   indices packed into rt_packed_material and with them the 255-texture limit
                                                   (INVALID_TEXTURE_IDX 0xFF, constants.h:35; PackAlbedo's assert, scene.cpp:55) */
    uint32_t flags;                             /* RT_SCENE_* */
} rt_scene_desc;
/* rt_scene_desc::flags */
#define RT_SCENE_EMISSIVE_NEE 1u   /* next-event estimation also samples the emissive triangles of emissive_indices (which the
                                      reference collects, scene.cpp:324-339, and passes to a kernel that ignores them,
                                      hit_surface.cl:39).  Changes the estimator, not the expected image: DESIGN.md section 7b */

int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene);

/* The scene's triangles MOVED (a door opens, a character deforms): topology, split axes and every fold stay, all bounds are made again on the device from the
 * new vertices -- a leaf's = min / max over its vertices, an interior node's = min / max of its two children -- in the triangle records, the child-pair records
 * and every 4-wide tree the scene holds (the reference fold, an adapted or imported fold, the shadow rays' own tree, the pair layout alike), then the frames and
 * 8-bit planes of the 4-wide records by the builder's own quantisation.  Milliseconds where rt_scene_upload takes a third of a second or more.
 *   triangles: the reference layout, the SAME count and the same (BVH) order as the upload; positions, normals, texture coordinates and mtl_index may change.
 *   rt_scene_refit takes a host array, rt_scene_refit_buffer an rt_buffer of num_triangles * sizeof(rt_triangle) bytes of this context (no PCIe copy: the per-frame path).
 * Afterwards the context behaves, for every entry point and option, exactly as a fresh one would after rt_scene_upload of the moved triangles with the node array
 * "same topology, same split axes, bounds refitted": radiance, resolved image, counters, AOVs, guides and filter outputs are bit-identical (the trees WALKED may differ
 * from what a fresh upload would choose, which never changes a result; a refitted tree is a worse tree after a large deformation -- upload again then).
 * Refused with the scene untouched: RT_CTX_OPT_REFITTABLE off at upload, no scene, another count or size, the tolerance mode (RT_CTX_OPT_CLOSEST_TREE != 0), a
 * non-finite position or mtl_index >= num_materials (checked by a read-only kernel first), or node arrays whose leaves are not consecutive ranges covering the
 * triangle array.  Otherwise: quiesces as rt_scene_upload does (samples traced ahead are dropped); a fold adaptation is retired -- one in flight is cancelled --
 * and the records adapted so far stay in use; guide caches and temporal histories drop as on upload (RT_CTX_OPT_REFIT_MOTION = 1: the histories follow the move); frames keep their accumulation: rt_reset them.
 * A record that no longer qualifies for k_trace_w4 after the move (cell above 2^20, coordinates beyond 2^28) does not fail the call: the scene is traced by the
 * BVH2 kernels, as after an upload of such a tree, until a later refit qualifies again; rt_scene_tree_report's "refit" line says which. */
int rt_scene_refit(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles);
int rt_scene_refit_buffer(rt_ctx* ctx, rt_buffer* triangles);

/* The scene's OBJECTS moved, each by one 3x4 matrix (the door that opens): 12 floats per object instead of 160 bytes per triangle.
 *   rt_scene_set_objects, after rt_scene_upload on a context with RT_CTX_OPT_REFITTABLE = 1: object_of_triangle[num_triangles] (the upload's BVH order), every
 *     entry < num_objects, is copied to the device; the scene's CURRENT pose becomes the rest pose (made from the shading records: positions, normals, texture
 *     coordinates, mtl_index -- every field a refit reads); the staging area of a pose is allocated, so rt_scene_pose allocates nothing.  324 bytes per triangle
 *     (rest pose 160, object index 4, staging area 160; rt_scene_tree_report's "posed objects" line).  Refused, with what an earlier call set left in place: a NULL
 *     argument, no scene, a scene that is not refittable, another triangle count, num_objects == 0, an index >= num_objects.  Calling it again replaces indices
 *     and rest pose; rt_scene_upload drops both; rt_scene_refit* leaves both alone (the rest pose is what set_objects saw, not the last refit).
 *   rt_scene_pose: matrices3x4[num_objects * 12], row-major, m[0..3] = row x (three linear terms, then the translation).  Poses are ABSOLUTE: every call poses
 *     the rest pose, so M1 then M2 equals M2 alone.  position' = ((m0 x + m1 y) + m2 z) + m3 per row; normal' = the cofactor matrix of the 3x3 part times the
 *     normal, times -1 if det < 0, normalised if its squared length is positive and finite; texture coordinates and mtl_index are copied; an object whose matrix is
 *     bit for bit the identity's is copied, so posing everything by the identity gives the rest pose back byte for byte.  k_pose_triangles writes the staging
 *     area and the refit above runs on it unchanged: afterwards the context is, for every entry point and option, bit for bit what rt_scene_refit of
 *     rt_debug_pose(NULL, ...)'s output would have left (validation first, so an overflowing pose is refused with the scene untouched; quiescence; the kept
 *     previous pose of RT_CTX_OPT_REFIT_MOTION; the report's "refit" line).  Refused before any launch: a NULL argument, no objects set, another num_objects, a
 *     non-finite matrix entry, everything rt_scene_refit refuses. */
int rt_scene_set_objects(rt_ctx* ctx, const uint32_t* object_of_triangle, uint32_t num_triangles, uint32_t num_objects);
int rt_scene_pose(rt_ctx* ctx, const float* matrices3x4, uint32_t num_objects);

/* The scene's triangles SKINNED from a palette of bone matrices (the character that deforms): 48 bytes per bone and frame instead of 160 bytes per triangle
 * (linear blend skinning).  One rt_skin_influence per triangle CORNER, 3 * num_triangles of them in the upload's BVH order: v1, v2, v3 of
 * triangle 0, then triangle 1, ...  An unused slot has weight 0 and any valid bone.  The library does not normalise weights.
 *   rt_scene_set_skin, after rt_scene_upload on a context with RT_CTX_OPT_REFITTABLE = 1: per_corner[3 * num_triangles], every bone < num_bones and every weight
 *     finite, is copied to the device; the scene's CURRENT pose becomes the rest pose (made from the shading records as rt_scene_set_objects makes it); the
 *     staging area of a skin and the palette's room are allocated, so rt_scene_skin allocates nothing.  392 bytes per triangle (rest pose 160, influences 72,
 *     staging area 160; rt_scene_tree_report's "skinned triangles" line).  Refused, with what an earlier call set left in place: a NULL argument, no scene, a
 *     scene that is not refittable, another triangle count, num_bones == 0 or above 65536, a bone index >= num_bones, a non-finite weight.  Calling it again
 *     replaces influences and rest pose; rt_scene_upload drops both; rt_scene_refit*, rt_scene_set_objects and rt_scene_pose leave both alone, as this leaves
 *     the objects alone: the two states are independent, each works from its own rest pose, and whichever of pose / skin / refit ran last is the scene.
 *   rt_scene_skin: matrices3x4[num_bones * 12], rt_scene_pose's layout.  Skins are ABSOLUTE: every call skins the rest pose, so M1 then M2 equals M2 alone.
 *     Per corner B[k] = ((w0 M[b0][k] + w1 M[b1][k]) + w2 M[b2][k]) + w3 M[b3][k] for the 12 entries, in that order, no slot skipped; a corner whose B is bit for
 *     bit the identity is copied; otherwise position and normal go through rt_scene_pose's arithmetic with B (cofactors, det and sign made from B per corner);
 *     the .w lanes, texture coordinates, mtl_index and padding are copied.  So with every bone the identity, weights that blend to exactly the identity --
 *     (1,0,0,0), (0.5,0.5,0,0) -- give the rest pose back byte for byte; weights that sum to 0 collapse a corner to the origin with a zero normal (finite:
 *     accepted).  k_skin_triangles writes the staging area and the refit above runs on it unchanged: afterwards the context is, for every entry point and
 *     option, bit for bit what rt_scene_refit of rt_debug_skin(NULL, ...)'s output would have left (validation first, so an overflowing skin is refused with
 *     the scene untouched; quiescence; the kept previous pose of RT_CTX_OPT_REFIT_MOTION; the report's "refit" line).  Refused before any launch: a NULL
 *     argument, no skin set, another num_bones, a non-finite matrix entry, everything rt_scene_refit refuses. */
typedef struct rt_skin_influence { uint16_t bone[4]; float weight[4]; } rt_skin_influence;
int rt_scene_set_skin(rt_ctx* ctx, const rt_skin_influence* per_corner, uint32_t num_triangles, uint32_t num_bones);
int rt_scene_skin(rt_ctx* ctx, const float* matrices3x4, uint32_t num_bones);

/* The scene's triangles MORPHED from one weight per morph target (blend shapes: faces, muscle correctives, cloth caches): 4 bytes per target and frame instead of
 * 160 bytes per triangle, alone or fused with the skin above -- morph the rest pose first, then skin the result, as glTF, FBX and Alembic do.
 * A target is SPARSE: one rt_morph_delta per triangle corner it moves, corner = 3 * triangle + c in the upload's BVH order (c = 0, 1, 2 for v1, v2, v3), a
 * position delta, a normal delta (three +0.0 words: the target leaves that normal alone) and pad = 0.  A vertex several triangles share is given once per
 * corner, with the same delta, or the mesh cracks.
 *   rt_scene_set_morph, after rt_scene_upload on a context with RT_CTX_OPT_REFITTABLE = 1: target t owns deltas[target_offsets[t] .. target_offsets[t + 1]),
 *     in any order inside the target; target_offsets has num_targets + 1 entries.  The library keeps the deltas on the device as one row of 32-byte records per
 *     triangle (sorted by triangle, then target, then corner); the scene's CURRENT pose becomes the morph's rest pose (made from the shading records as
 *     rt_scene_set_skin makes its own); the staging area and the weights' device and pinned host memory are allocated, so a morph allocates nothing.  Kept:
 *     320 bytes per triangle (rest pose 160, staging area 160), 4 per row, 32 per delta, 4 per target (rt_scene_tree_report's "morph targets" line).  Refused,
 *     with what an earlier call set left in place: a NULL argument, no scene, a scene that is not refittable, another triangle count, num_targets == 0 or above
 *     65536, target_offsets[0] != 0, decreasing offsets, a corner >= 3 * num_triangles, a non-finite delta word, pad != 0, the same (target, corner) twice --
 *     the offsets are checked first, then the deltas in array order, and the first offence decides the message.  A set with no deltas at all is legal: every
 *     morph returns the rest pose.  Calling it again replaces the targets and the rest pose; rt_scene_upload drops them; rt_scene_refit*, rt_scene_set_objects,
 *     rt_scene_pose, rt_scene_set_skin and rt_scene_skin leave them alone, as this leaves theirs alone: the three states are independent and whichever of
 *     pose / skin / morph / refit ran last is the scene.
 *   rt_scene_morph: weights[num_targets], used as given (nothing normalises them).  Morphs are ABSOLUTE: every call morphs the rest pose, so w1 then w2 equals
 *     w2 alone.  Per corner, its records in ascending target order: a record whose weight is +0 or -0 is skipped entirely; otherwise p.x = p.x + w * dp.x,
 *     likewise y and z; if a word of dn is not zero, n.x = n.x + w * dn.x, likewise y and z, and the corner's normal is renormalised once after its last record
 *     by rt_scene_pose's rule (l = (x^2 + y^2) + z^2, divided by sqrtf(l) if l > 0 and finite, else left as summed); a corner with no applied record is copied
 *     byte for byte; the .w lanes, texture coordinates, mtl_index and padding are copied.  So all-zero weights give the rest pose back byte for byte and a
 *     position-only target never touches a normal.  k_morph_triangles writes the staging area and the refit above runs on it unchanged: afterwards the context
 *     is, for every entry point and option, bit for bit what rt_scene_refit of rt_debug_morph(NULL, ...)'s output would have left (validation first, so an
 *     overflowing morph is refused with the scene untouched).  Refused before any launch: a NULL argument, no morph set, another num_targets, a non-finite
 *     weight, everything rt_scene_refit refuses.
 *   rt_scene_morph_skin, after both rt_scene_set_morph and rt_scene_set_skin: the morph above, then rt_scene_skin's arithmetic on its result, in ONE kernel
 *     (k_morph_skin_triangles).  It uses THE MORPH'S REST POSE; from the skin it takes the influences and the palette's room and nothing else -- the skin's own
 *     rest pose is not read, and the two can differ when a refit, pose, skin or morph ran between the two set calls.  Afterwards the context is bit for bit what
 *     rt_scene_refit of rt_debug_skin(NULL, rt_debug_morph(NULL, rest, ..., weights), influences, matrices) would have left.  It refuses whatever either
 *     single call refuses. */
typedef struct rt_morph_delta { uint32_t corner; float position[3]; float normal[3]; uint32_t pad; } rt_morph_delta;
int rt_scene_set_morph(rt_ctx* ctx, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles);
int rt_scene_morph(rt_ctx* ctx, const float* weights, uint32_t num_targets);
int rt_scene_morph_skin(rt_ctx* ctx, const float* weights, uint32_t num_targets, const float* matrices3x4, uint32_t num_bones);

/* ---- ray queries: the CALLER's rays against the uploaded scene (opt-in extension).  Every other ray this library traces is one a frame
 * generated; these are a host program's own: which object lies under a pixel, visibility and probe rays, baking over the uploaded trees, collision rays against
 * a posed scene.
 *   rays: rt_ray as the reference means it (trace_bvh.cl:148,28-73): origin.w = t_min, direction.w = t_max; a candidate hit is rejected when t < t_min ||
 *     t > t_max, a box's entry distance is max(..., t_min).  t_min > t_max is therefore a miss.  A ray with a non-finite component in origin, direction, t_min
 *     or t_max, and a ray whose direction is all zeros, is not walked: a miss (not occluded).
 *   RT_QUERY_CLOSEST: hits[i] = bc, primitive_id (BVH order, as everywhere in this ABI) and t, bit for bit what the reference's IntersectRays gives that ray on
 *     the scene's current triangles (its topology and near / far order decide ties); on a miss only primitive_id = RT_INVALID_ID is specified.  surfaces[i]:
 *     the hit's surface (rt_surface).  At least one of hits / surfaces; occluded[i] (optional) = 1 on a hit.
 *   RT_QUERY_ANY_HIT: occluded[i] = 1 when anything lies within [t_min, t_max], else 0 -- exact; WHICH triangle is not reported (the shadow rays' own tree visits
 *     leaves in its own order: only the OR over all leaves is tree-independent).  hits and surfaces must be NULL.
 * Closest-hit queries walk what a frame's closest-hit rays walk at the moment (the current 4-wide records, adapted folds included; the child-pair records with
 * RT_CTX_OPT_WIDE_BVH = 0 or a tree that does not qualify), any-hit queries the shadow rays' tree.  A query runs on the context's stream, after every refit,
 * pose or upload before it, and touches no frame: accumulation, samples traced ahead, guide caches, filter histories and rt_stats are as if it had not happened.
 *   rt_scene_trace: host arrays, staged through device scratch the context keeps (grown on demand, chunks of at most 4 Mi rays: any n needs bounded memory;
 *     rt_scene_tree_report's "ray queries" line has its size); returns when the outputs are written.
 *   rt_scene_trace_buffer: rt_buffers of this context holding n records each (rt_ray / rt_hit / uint32_t / rt_surface); only enqueues -- rt_finish or
 *     rt_buffer_read waits; allocates at most the walk's stack spill area.
 * A traversal stack that ran over its bound (excluded by the bound's argument; checked all the same) is never silent: the query's kernel raises a
 * flag, and the next call that waits for the context's stream -- rt_scene_trace itself, rt_finish, rt_buffer_read -- fails with that message and clears it.
 * Refused with nothing launched: a NULL context, NULL rays with n > 0, no scene, an unknown mode, closest mode without hits and surfaces, any-hit mode with
 * hits or surfaces or without occluded, a buffer of another context or smaller than n records.  n == 0 is RT_OK and does nothing. */
#define RT_QUERY_CLOSEST 0u
#define RT_QUERY_ANY_HIT 1u
typedef struct rt_surface
{
    float position[3];         uint32_t primitive_id;   /* RT_INVALID_ID on a miss: every other field 0 then */
    float geometric_normal[3]; uint32_t mtl_index;      /* normalize(cross(p2 - p1, p3 - p1)); zeros for a degenerate triangle */
    float shading_normal[3];   uint32_t object;         /* rt_scene_set_objects' index of the triangle, RT_INVALID_ID if none set */
    float texcoord[2];         float t;  uint32_t flags; /* bit 0: hit; bit 1: dot(direction, geometric_normal) > 0 (back face) */
} rt_surface;
int rt_scene_trace(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t mode, rt_hit* hits_or_null, uint32_t* occluded_or_null, rt_surface* surfaces_or_null);
int rt_scene_trace_buffer(rt_ctx* ctx, rt_buffer* rays, uint32_t n, uint32_t mode, rt_buffer* hits_or_null, rt_buffer* occluded_or_null, rt_buffer* surfaces_or_null);
/* The closest hit of the ray through the CENTRE of pixel (x, y) -- image coordinates -- of the frame's current camera: the guide pass's ray (origin = the camera
 * position, direction = the filters' pixel-centre direction, t_min 0, t_max RT_MAX_RENDER_DIST), so surface.shading_normal and |origin - position| are bit for
 * bit rt_frame_read_guides' normal and depth of that pixel.  Any output may be NULL.  Refused: a NULL frame, no scene, x >= width or y >= height, a tile frame. */
int rt_frame_pick(rt_frame* frame, uint32_t x, uint32_t y, rt_ray* ray_or_null, rt_hit* hit_or_null, rt_surface* surface_or_null);
/* the surface records on their own: out[i] of rays[i] and hits[i] over caller triangles (object_of_triangle NULL: object = RT_INVALID_ID); a hit whose
 * primitive_id is not below num_triangles counts as a miss.  ctx == NULL: the host restatement (query.h); otherwise k_query_surface on uploaded copies.  The
 * two agree bit for bit. */
int rt_debug_query_surface(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle_or_null,
                           const rt_ray* rays, const rt_hit* hits, uint32_t n, rt_surface* out);

/* ---- occlusion bakes: ambient occlusion and bent normals at the CALLER's points (opt-in extension).  Per point a cosine-weighted
 * hemisphere of `samples` any-hit rays about the point's normal is generated, walked and reduced on the device: 32 bytes per point in, 16 out, no ray or verdict
 * ever crosses PCIe.  raytracing_amd/csrc/bake.h states every step of the arithmetic (the rays, the frame, the order of the reduction).
 *   points: eight floats each -- position xyz, w ignored, normal xyz (any length), w ignored; with RT_BAKE_FROM_SURFACES rt_surface records instead (position,
 *     shading_normal negated when flags bit 1 -- back face -- is set; a record with flags bit 0 clear, a miss, is skipped): rt_scene_trace_buffer's surfaces feed a
 *     bake without a trip to the host.
 *   a point is SKIPPED -- none of its rays walked, unoccluded = RT_INVALID_ID, bent_normal zeros -- when a position or normal component is not finite, when
 *     the normal's squared length is zero or not finite, or when it is a miss record.
 *   every other point: ray k has origin = position + unit normal * bias, t_min 0, t_max radius; unoccluded = the rays for which nothing lies within [0, radius]
 *     (exact any-hit verdicts over the shadow rays' tree, as RT_QUERY_ANY_HIT's); the sampling is cosine-weighted, so unoccluded / samples is the ambient
 *     occlusion term.  bent_normal = the normalised sum of the unoccluded rays' directions in bake.h's order, zeros when that sum's squared length is zero or
 *     not finite.  The rays of point i depend on (i, seed): i = the point's index within the call.
 * A bake runs on the context's stream, after every refit, pose or upload before it, and touches no frame and no rt_stats field, like a query; a traversal
 * stack that ran over its bound is reported as a query's is.
 *   rt_scene_bake: host arrays, staged in chunks of at most 1 Mi points (RT_CTX_OPT_BAKE_CHUNK_POINTS) through scratch the context keeps; a chunk carries the
 *     index of its first point, so chunking changes no result; returns when `out` is written.
 *   rt_scene_bake_buffer: rt_buffers of this context holding n records each; only enqueues.
 * Refused with nothing launched: a NULL context, NULL points / desc / out with n > 0, no scene, samples not a power of two in 16 .. 4096, a bias or radius that
 * is not finite, radius <= 0, unknown flag bits, a buffer of another context or smaller than n records.  n == 0 is RT_OK and does nothing. */
#define RT_BAKE_FROM_SURFACES 1u
typedef struct rt_bake_desc
{
    uint32_t samples;  /* rays per point: a power of two, 16 .. 4096 */
    uint32_t seed;
    uint32_t flags;    /* RT_BAKE_FROM_SURFACES */
    float bias;        /* origin = position + unit normal * bias */
    float radius;      /* t_max; t_min = 0 */
} rt_bake_desc;
typedef struct rt_bake_result
{
    float bent_normal[3];
    uint32_t unoccluded;
} rt_bake_result;
int rt_scene_bake(rt_ctx* ctx, const void* points, uint32_t n, const rt_bake_desc* desc, rt_bake_result* out);
int rt_scene_bake_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, const rt_bake_desc* desc, rt_buffer* out);
/* the rays of a bake on their own: rays_out[p * samples + k] = ray k of points[p], whose index is first_index + p (t_min 0 in origin.w, radius in
 * direction.w); a skipped point's rays are all zeros.  ctx == NULL: the host restatement (bake.h); otherwise k_bake_rays on an uploaded copy.  The two agree
 * bit for bit.  At most 2^28 rays per call. */
int rt_debug_bake_rays(rt_ctx* ctx_or_null, const void* points, uint32_t n, uint32_t first_index, const rt_bake_desc* desc, rt_ray* rays_out);
/* the reduction on its own (host only): out[p] from rays[p * samples ..] and their verdicts (occluded[] != 0: something lies within the ray's range), in
 * bake.h's order.  A point whose first ray has an all-zero direction is a skipped one. */
int rt_debug_bake_reduce(const rt_ray* rays, const uint32_t* occluded, uint32_t n, uint32_t samples, rt_bake_result* out);

/* ---- the UV atlas: which triangle every texel of a texture shows and where on it, and an occlusion bake into it (opt-in extension).
 * A lightmap or AO map needs, per texel, the surface point that texel shows: the scene's triangles rasterised in UV space.  That runs on the device -- no
 * tree is walked -- and is repeated for free after a pose, skin or morph.  raytracing_amd/csrc/atlas.h states the rule, in integers:
 *   the atlas: width x height texels (1 .. 16384 each, width * height <= 2^26), texel (x, y) at index y * width + x, row 0 at v = 0; the texel's centre is
 *     tested, in fixed point with 8 sub-texel bits.  No repeat or wrap: only the centres inside [0, 1) x [0, 1) exist.
 *   a triangle's corners snap to X = rintf(u * 256 width), Y = rintf(v * 256 height); it is SKIPPED (triangles_skipped) when a component is not finite, a
 *     snapped coordinate exceeds 2^24 in magnitude, or its snapped area is 0.  Every other triangle covers the centres inside it and those on the edges it owns
 *     (atlas.h's rule): two triangles that share an edge give every centre on it to exactly one of them, whatever their winding; both windings rasterise.
 *   rt_texel: count = the triangles that cover the centre (saturating at 65535), primitive_id = the lowest of them (BVH order, as everywhere in this ABI),
 *     bc = that triangle's barycentrics at the centre as rt_hit's (the weights of corners 2 and 3: one exact binary64 divide each, rounded once to binary32),
 *     flags = RT_TEXEL_COVERED.  Uncovered: RT_INVALID_ID and zeros.
 *   gutter (0 .. 4 passes): each pass gives every texel without a record that of its first neighbour with one, in the order left, right, up (y - 1), down,
 *     up-left, up-right, down-left, down-right, with flags = RT_TEXEL_GUTTER and count = 0, so a bilinear fetch at a chart's border reads no empty texel.
 *   uv_or_null: six floats per triangle in BVH order (u1 v1 u2 v2 u3 v3), a second UV set -- the usual lightmap channel; NULL: the triangles' own texcoord.xy.
 *   desc.object: only the triangles of that object of rt_scene_set_objects are rasterised (the others count in triangles_filtered and nowhere else);
 *     RT_INVALID_ID: every triangle.
 *   rt_atlas_stats: covered and overlapped (count > 1) texels before the gutter, the texels the gutter filled, and of the triangles those skipped, those
 *     filtered, and those neither skipped nor filtered that cover no centre (triangles_without_texel: too small for this atlas -- a lightmapper's warning).
 * The cover depends on the UVs alone: it stays valid across refit, pose, skin and morph.  Everything runs on the context's stream, after every upload, refit or
 * pose before it, touches no frame and no rt_stats field, and keeps nothing between calls but scratch the context grows on demand (the bakes').
 *   rt_scene_atlas: host arrays; returns when texels[width * height] (and *stats) are written.
 *   rt_scene_atlas_buffer: rt_buffers of this context (uv: 24 bytes per triangle; texels: width * height records; stats: one rt_atlas_stats); only enqueues.
 *   rt_scene_atlas_surfaces / _buffer: surfaces[i] = the rt_surface of (texels[i].primitive_id, texels[i].bc) on the scene's triangles AS POSED NOW, made as a
 *     ray query makes it (query.h) with an all-zero direction and t = 0, so flags = hit, never back face; an uncovered record gives a miss record.  A
 *     primitive_id that is neither RT_INVALID_ID nor below the scene's triangle count is refused by the host form and gives a miss record in the buffer form.
 *     The records feed rt_scene_bake_buffer(RT_BAKE_FROM_SURFACES).
 *   rt_scene_atlas_bake: the cover, its surfaces and rt_scene_bake(RT_BAKE_FROM_SURFACES) of them in one call, all on the device: out[i] of texel i is byte for
 *     byte rt_scene_bake of rt_scene_atlas_surfaces' records with the same bake_desc (point index = texel index; the bake's chunking, which changes no result);
 *     an uncovered texel is a skipped point (unoccluded = RT_INVALID_ID).  bake_desc->flags must be 0.  texels_or_null / stats_or_null: the cover itself.
 *   rt_debug_atlas: the cover over caller triangles (primitive_id = the index).  ctx == NULL: the host restatement (atlas.h); otherwise the kernels on
 *     uploaded copies.  The two agree byte for byte.
 * Refused with nothing launched: a NULL context, desc, texels, surfaces or out; no scene; a size out of range; gutter > 4; desc.object set without
 * rt_scene_set_objects (rt_debug_atlas: without object_of_triangle) or not below the object count; caller bits in bake_desc->flags, or a bake_desc that
 * rt_scene_bake refuses; a buffer of another context or one that is too small. */
#define RT_TEXEL_COVERED 1u
#define RT_TEXEL_GUTTER  2u
typedef struct rt_texel { float bc[2]; uint32_t primitive_id; uint16_t count; uint16_t flags; } rt_texel;   /* 16 bytes; count saturates at 65535; uncovered: RT_INVALID_ID, zeros */
typedef struct rt_atlas_desc { uint32_t width, height, gutter, object; } rt_atlas_desc;                     /* object: RT_INVALID_ID = every triangle */
typedef struct rt_atlas_stats { uint32_t covered, overlapped, gutter, triangles_skipped, triangles_without_texel, triangles_filtered; uint32_t reserved[2]; } rt_atlas_stats;
int rt_scene_atlas(rt_ctx* ctx, const rt_atlas_desc* desc, const float* uv_or_null, rt_texel* texels, rt_atlas_stats* stats_or_null);
int rt_scene_atlas_buffer(rt_ctx* ctx, const rt_atlas_desc* desc, rt_buffer* uv_or_null, rt_buffer* texels, rt_buffer* stats_or_null);
int rt_scene_atlas_surfaces(rt_ctx* ctx, const rt_texel* texels, uint32_t n, rt_surface* surfaces);
int rt_scene_atlas_surfaces_buffer(rt_ctx* ctx, rt_buffer* texels, uint32_t n, rt_buffer* surfaces);
int rt_scene_atlas_bake(rt_ctx* ctx, const rt_atlas_desc* atlas_desc, const float* uv_or_null, const rt_bake_desc* bake_desc, rt_bake_result* out,
                        rt_texel* texels_or_null, rt_atlas_stats* stats_or_null);
int rt_debug_atlas(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle_or_null, const float* uv_or_null,
                   const rt_atlas_desc* desc, rt_texel* texels, rt_atlas_stats* stats);

/* ---- light bakes: the irradiance the sky and the scene's analytic lights give the CALLER's points or the atlas's texels, direct terms only (opt-in
 * extension).  Per point a cosine-weighted hemisphere of `samples` any-hit rays looks the environment up where it escapes, and one
 * any-hit ray per light of the uploaded scene asks whether that light is seen: generated, walked and reduced on the device, 32 bytes per point out.
 * raytracing_amd/csrc/light_bake.h states every step of the arithmetic (the items, the environment look-up, the lights' terms, the order of the reduction).
 *   points, the skip rule, the frame, the biased origin, the rays' dependence on (i, seed): rt_scene_bake's, unchanged (RT_BAKE_FROM_SURFACES: rt_surface
 *     records).  A SKIPPED point gives zeros and both counts RT_INVALID_ID.
 *   sky = (pi / samples) * the sum of the environment (rt_scene_desc's env_rgba, the path tracer's own bilinear look-up) over the sky rays that meet nothing
 *     within [0, sky_distance]: the irradiance from the environment, in its units; sky_unoccluded = how many those are -- with radius = sky_distance,
 *     rt_scene_bake's unoccluded.
 *   lights = the sum over the scene's lights that are above the point's horizon (cosine c > 0) and unshadowed of radiance * c / distance^2 (a point light;
 *     its shadow ray is the segment to the light) or radiance * c (any other type: directional, light.origin its direction, shadowed within sky_distance);
 *     lights_unshadowed = how many those are.  No material, no indirect light, no emissive triangle enters.
 *   RT_LIGHT_BAKE_NO_SKY / RT_LIGHT_BAKE_NO_LIGHTS: that half makes no rays and stays zero.
 * Everything runs on the context's stream, after every upload, refit or pose before it, touches no frame and no rt_stats field, and a traversal stack that ran
 * over its bound is reported as a query's is.
 *   rt_scene_light_bake: host arrays, staged in chunks of at most 1 Mi points (RT_CTX_OPT_BAKE_CHUNK_POINTS); a chunk carries the index of its first point,
 *     so chunking changes no result; returns when `out` is written.
 *   rt_scene_light_bake_buffer: rt_buffers of this context holding n records each; only enqueues.
 *   rt_scene_atlas_bake_light: the cover, its surfaces and rt_scene_light_bake(RT_BAKE_FROM_SURFACES) of them in one call, all on the device: out[i] of texel i
 *     is byte for byte rt_scene_light_bake of rt_scene_atlas_surfaces' records (point index = texel index); an uncovered texel is a skipped point.
 *     desc->flags must be 0.  texels_or_null / stats_or_null: the cover itself.
 *   rt_debug_light_bake_rays: rays_out[p * (samples + num_lights) + r] = the ray of item r of points[p], whose index is first_index + p (t_min 0 in origin.w,
 *     t_max in direction.w); all zeros for an item that makes no ray and for a skipped point.  ctx == NULL: the host restatement (light_bake.h); otherwise
 *     k_light_bake_rays on uploaded copies.  The two agree bit for bit.  At most 2^28 rays per call.
 *   rt_debug_light_bake_reduce (host only): out[p] from the items of points[p] and their verdicts occluded[p * (samples + num_lights) + r] (!= 0: something
 *     lies within the ray's range; ignored for items without a ray), in light_bake.h's order.  env_rgba: env_w x env_h RGBA floats; may be NULL with
 *     RT_LIGHT_BAKE_NO_SKY.
 * (The point forms are rt_scene_light_bake*, after rt_light_bake_desc and rt_debug_light_bake_*: the rt_scene_bake* family is the occlusion bake's two forms.)
 * Refused with nothing launched: a NULL context, NULL points / desc / out with n > 0, no scene, samples not a power of two in 16 .. 4096, a bias or
 * sky_distance that is not finite, sky_distance <= 0, unknown flag bits (rt_scene_atlas_bake_light: any flag bit), a buffer of another context or smaller than
 * n records, NULL lights with num_lights > 0, more than 2^28 rays in a debug call.  n == 0 is RT_OK and does nothing. */
#define RT_LIGHT_BAKE_NO_SKY    2u     /* beside RT_BAKE_FROM_SURFACES (1u) in rt_light_bake_desc.flags */
#define RT_LIGHT_BAKE_NO_LIGHTS 4u
typedef struct rt_light_bake_desc
{
    uint32_t samples;    /* sky rays per point: a power of two, 16 .. 4096 */
    uint32_t seed;
    uint32_t flags;      /* RT_BAKE_FROM_SURFACES | RT_LIGHT_BAKE_NO_SKY | RT_LIGHT_BAKE_NO_LIGHTS */
    float bias;          /* origin = position + unit normal * bias */
    float sky_distance;  /* t_max of the sky rays and of the directional lights' shadow rays; t_min = 0 */
} rt_light_bake_desc;
typedef struct rt_light_bake_result
{
    float sky[3];     uint32_t sky_unoccluded;
    float lights[3];  uint32_t lights_unshadowed;
} rt_light_bake_result;
int rt_scene_light_bake(rt_ctx* ctx, const void* points, uint32_t n, const rt_light_bake_desc* desc, rt_light_bake_result* out);
int rt_scene_light_bake_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, const rt_light_bake_desc* desc, rt_buffer* out);
int rt_scene_atlas_bake_light(rt_ctx* ctx, const rt_atlas_desc* atlas_desc, const float* uv_or_null, const rt_light_bake_desc* desc, rt_light_bake_result* out,
                              rt_texel* texels_or_null, rt_atlas_stats* stats_or_null);
int rt_debug_light_bake_rays(rt_ctx* ctx_or_null, const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc* desc, const rt_light* lights,
                             uint32_t num_lights, rt_ray* rays_out);
int rt_debug_light_bake_reduce(const void* points, uint32_t n, uint32_t first_index, const rt_light_bake_desc* desc, const rt_light* lights, uint32_t num_lights,
                               const float* env_rgba, uint32_t env_w, uint32_t env_h, const uint32_t* occluded, rt_light_bake_result* out);

/* ---- nearest surface point: which triangle is nearest to each of the CALLER's points, where on it, and how far (opt-in extension).
 * raytracing_amd/csrc/nearest.h states every step of the arithmetic: the distance to one triangle (Ericson's region test, the blend in rt_surface's operand
 * order, the clamp to the triangle's box, d2 = |p - q|^2) and the distance to a box that prunes the walk.
 *   the answer for a point: over all triangles the one with the smallest d2 <= max_distance^2 (the square rounded once; max_distance may be +inf); a tie in d2
 *     goes to the lowest primitive_id (BVH order, rt_hit's).  That is a statement about the triangles alone: the result is bit for bit the brute-force minimum
 *     (rt_debug_nearest), whichever tree is walked, whichever fold is in place, after any refit or pose.
 *   rt_nearest: position = the closest point (inside the triangle's box), distance = sqrtf(d2), bc = (weight of p2, weight of p3) as rt_hit's, flags =
 *     RT_NEAREST_FOUND | RT_NEAREST_BACK_SIDE when dot3(p - position, cross3(p2 - p1, p3 - p1)) < 0 | the feature (0 face, 1 edge, 2 vertex) << 2.
 *     Nothing found: primitive_id = RT_INVALID_ID, zeros, flags 0.
 *   a point is NOT SEARCHED (the same record) when a position component is not finite or max_distance is NaN or negative.
 *   surfaces (optional): the rt_surface of the nearest point, made as a ray query makes it (query.h) with direction = position - p and t = distance; a miss
 *     record where nothing was found.  Its flags bit 1 (back face) agrees with RT_NEAREST_BACK_SIDE except where the normalised geometric normal degenerates
 *     (zeros: a triangle without area, or one whose squared normal overflows or underflows) or the product with it rounds to zero.  The records feed
 *     rt_scene_bake_buffer(RT_BAKE_FROM_SURFACES) without a trip to the host.
 * A nearest query runs on the context's stream, after every refit, pose or upload before it, and touches no frame and no rt_stats field, like a ray query;
 * it uses the ray queries' stack spill area and staging arrays, and a traversal stack that ran over its bound is reported as a ray query's is.
 *   rt_scene_nearest: host arrays, staged in chunks; returns when the outputs are written.
 *   rt_scene_nearest_buffer: rt_buffers of this context holding n records each; only enqueues.
 * Refused with nothing launched: a NULL context, NULL points with n > 0, no scene, both outputs NULL, a buffer of another context or smaller than n records.
 * n == 0 is RT_OK and does nothing. */
typedef struct rt_point   { float position[3]; float max_distance; } rt_point;      /* 16 bytes; max_distance may be +inf */
typedef struct rt_nearest { float position[3]; float distance; float bc[2];
                            uint32_t primitive_id; uint32_t flags; } rt_nearest;    /* 32 bytes */
#define RT_NEAREST_FOUND 1u
#define RT_NEAREST_BACK_SIDE 2u           /* the point lies behind the triangle's geometric normal */
#define RT_NEAREST_FEATURE_SHIFT 2        /* bits 2..3: 0 face, 1 edge, 2 vertex */
int rt_scene_nearest(rt_ctx* ctx, const rt_point* points, uint32_t n, rt_nearest* out_or_null, rt_surface* surfaces_or_null);
int rt_scene_nearest_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, rt_buffer* out_or_null, rt_buffer* surfaces_or_null);
/* brute force over all of `triangles` (primitive_id = the index): nearest.h on the host (ctx == NULL) or k_nearest_brute on uploaded copies.  The two agree
 * bit for bit. */
int rt_debug_nearest(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const rt_point* points, uint32_t n, rt_nearest* out);
/* the kernel's walk on the host (no device): over the child-pair form of `nodes` (wide = 0) or over build_wide_bvh's 4-wide records of them (wide = 1), pruned
 * by nearest_box_d2; triangles_tested_or_null[i] = how many triangles point i was tested against.  Refused when the tree does not qualify for the 4-wide
 * layout (wide = 1) or is deeper than the walk's stack. */
int rt_debug_nearest_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide,
                          const rt_point* points, uint32_t n, rt_nearest* out, uint32_t* triangles_tested_or_null);

/* ---- all hits: every surface a CALLER's ray crosses, counted, the nearest of them sorted (opt-in extension).  What lies behind the
 * first surface (select-through picking), whether a point is inside a closed object (entries against exits along a ray), layer order and thickness.
 * raytracing_amd/csrc/all_hits.h states the arithmetic.
 *   the HIT SET of a walked ray: of every leaf of the scene's reference tree whose box passes the reference's box test with the ray's own [t_min, t_max],
 *     every triangle that the two-sided ray-triangle test accepts with that same range.  t_max is never lowered.  The test is the reference's (ray_triangle,
 *     trace_bvh.cl:28-73) with one rule changed: it rejects |det| < 1e-8 where the reference rejects every det < 1e-8 -- the reference culls back faces, and
 *     a set without them would hold no exits.  That is a statement about leaves and triangles alone: the set is the same whichever tree or fold is walked,
 *     after any refit or pose, and rt_debug_trace_all gives it by brute force.
 *   rt_ray_hits: count = the members; entering = the members with det > 0 (the ray runs against cross(p2 - p1, p3 - p1)): exactly the triangles a ray query
 *     could report, so entering > 0 is RT_QUERY_ANY_HIT's verdict and RT_QUERY_CLOSEST's hit is the nearest entering member; count - entering = the exits;
 *     stored = min(count, max_hits); flags bit 0 = the ray was walked, bit 8 + j = stored hit j is an exit.
 *   hits (optional, max_hits records per ray, max_hits <= RT_ALL_HITS_MAX): the `stored` smallest members in ascending (t, primitive_id) order, t compared as
 *     binary32: coincident triangles are both reported, lowest primitive_id first.  bc and t of an entering member are bit for bit a ray query's.  The records
 *     from `stored` up to max_hits are primitive_id = RT_INVALID_ID and zeros.  A smaller max_hits gives a prefix of the same list.
 *   surfaces (optional, max_hits per ray): the rt_surface of each stored hit as a ray query makes it (query.h); miss records beyond `stored`.
 *   a ray that is not walked (a non-finite component, an all-zero direction) gives zeros and invalid hits; t_min > t_max gives count 0.
 * Runs on the context's stream like a ray query, touches no frame and no rt_stats field, and uses the ray queries' spill area, status word and staging arrays.
 *   rt_scene_trace_all: host arrays, staged in chunks of at most 4 Mi hit records; returns when the outputs are written.
 *   rt_scene_trace_all_buffer: rt_buffers of this context (n rt_ray, n rt_ray_hits, n * max_hits rt_hit / rt_surface); only enqueues.
 *   rt_frame_pick_all: rt_frame_pick's ray through the centre of pixel (x, y).
 * Refused with nothing launched: a NULL context, NULL rays with n > 0, no scene, out NULL, max_hits > RT_ALL_HITS_MAX, hits or surfaces with max_hits == 0, a
 * buffer of another context or too small, a pixel outside the image, a tile frame.  n == 0 is RT_OK and does nothing. */
#define RT_ALL_HITS_MAX 8
#define RT_RAY_HITS_WALKED 1u
#define RT_RAY_HITS_EXIT_SHIFT 8
typedef struct rt_ray_hits { uint32_t count; uint32_t entering; uint32_t stored; uint32_t flags; } rt_ray_hits;      /* 16 bytes */
int rt_scene_trace_all(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits_or_null, rt_surface* surfaces_or_null);
int rt_scene_trace_all_buffer(rt_ctx* ctx, rt_buffer* rays, uint32_t n, uint32_t max_hits, rt_buffer* out, rt_buffer* hits_or_null, rt_buffer* surfaces_or_null);
int rt_frame_pick_all(rt_frame* frame, uint32_t x, uint32_t y, uint32_t max_hits, rt_ray* ray_or_null, rt_ray_hits* out, rt_hit* hits_or_null,
                      rt_surface* surfaces_or_null);
/* brute force over the leaves of `nodes`, no tree walk: each leaf's box test, then the triangle test on the trace-record form of its triangles (p1,
 * fl(p2 - p1), fl(p3 - p1)); primitive_id = the index.  ctx == NULL: the host (all_hits.h); otherwise k_all_hits_brute on uploaded copies.  The two agree bit
 * for bit.  hits may be NULL when max_hits == 0.  Refused: a NULL argument, a leaf whose triangles lie outside the array, max_hits > RT_ALL_HITS_MAX. */
int rt_debug_trace_all(rt_ctx* ctx_or_null, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles,
                       const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits);

/* ---- within: every triangle within a radius of each of the CALLER's points, counted, the nearest of them sorted (opt-in extension).
 * A contact set, a selection brush, how many surfaces lie within a bias, the k nearest triangles.  raytracing_amd/csrc/within.h states the rule; the
 * distances are nearest.h's, unchanged.  rt_point is reused: max_distance is the radius and may be +inf.
 *   a point is SEARCHED under rt_scene_nearest's rule.  r2 = max_distance * max_distance, rounded once.
 *   the MEMBER SET M of a searched point: every triangle whose d2 (nearest_point_triangle on the shading record's corners, rt_scene_nearest's operands)
 *     satisfies d2 <= r2; a NaN d2 is no member.  Members are ordered by ascending (d2, primitive_id), d2 compared as binary32.
 *   without RT_WITHIN_K_NEAREST: count = |M|, stored = min(count, max_near), nearest_primitive = the first member or RT_INVALID_ID (rt_scene_nearest's
 *     primitive_id for the same point), flags bit 0 = searched; near[i * max_near + j] = rt_scene_nearest's record form of member j for j < stored, the
 *     nothing-found record beyond.  The walk's bound is r2 and is never lowered: a subtree is skipped exactly when nearest_box_d2 > r2.
 *   with RT_WITHIN_K_NEAREST (max_near >= 1): the same first min(|M|, max_near) members are listed, count == stored (nothing beyond the list is looked
 *     for), flags bit 1 is set.  The bound starts at r2 and becomes the last list entry's d2 once the list is full; the comparison stays strict, so a tie
 *     with the last entry is visited and the lower primitive_id wins.  max_near = 1 gives rt_scene_nearest's record byte for byte.  With neither near nor
 *     surfaces there is no list to shrink the search by: the counting walk runs and the record is made from its count (the same record, a full walk's cost).
 *   a smaller max_near gives a prefix of a larger one's list.  A point that is not searched gives zeros, RT_INVALID_ID and nothing-found records.
 *   surfaces (optional, max_near per point): the rt_surface of each listed member as rt_scene_nearest makes it; miss records beyond `stored`.  A call
 *     that asks for surfaces only keeps its rt_nearest records in the first 32 bytes of each surface record on the way.
 *   M is a statement about triangles and nearest.h alone -- bit for bit rt_debug_within's brute force, whichever records are walked (the 4-wide fold, an
 *     adapted or imported fold, the child-pair records), after any refit or pose: nearest_box_d2 <= d2 holds in binary32 for every box that holds a
 *     triangle's corners, so a subtree skipped at bound b holds only triangles with d2 > b; b is r2 (no member is skipped) or the k-th smallest d2 met so
 *     far, which is never below the final one (no listed member is skipped).
 * Runs on the context's stream like a nearest query, touches no frame and no rt_stats field, and uses the ray queries' spill area, status word and staging
 * arrays.
 *   rt_scene_within: host arrays, staged in chunks of at most 4 Mi member records; returns when the outputs are written.
 *   rt_scene_within_buffer: rt_buffers of this context (n rt_point, n rt_point_hits, n * max_near rt_nearest / rt_surface); only enqueues.
 * Refused with nothing launched: a NULL context, no scene, NULL points with n > 0, out NULL, max_near > RT_WITHIN_MAX, near or surfaces with max_near == 0,
 * RT_WITHIN_K_NEAREST with max_near == 0, unknown option bits, a buffer of another context or too small.  n == 0 is RT_OK and does nothing. */
#define RT_WITHIN_MAX 8
#define RT_WITHIN_K_NEAREST 1u      /* options bit: do not count, shrink the search to the max_near-th member */
#define RT_POINT_HITS_SEARCHED 1u   /* rt_point_hits.flags bit 0 */
#define RT_POINT_HITS_K_NEAREST 2u  /* rt_point_hits.flags bit 1: a k-nearest answer, count == stored */
typedef struct rt_point_hits { uint32_t count; uint32_t stored; uint32_t nearest_primitive; uint32_t flags; } rt_point_hits;      /* 16 bytes */
int rt_scene_within(rt_ctx* ctx, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near_or_null,
                    rt_surface* surfaces_or_null);
int rt_scene_within_buffer(rt_ctx* ctx, rt_buffer* points, uint32_t n, uint32_t max_near, uint32_t options, rt_buffer* out, rt_buffer* near_or_null,
                           rt_buffer* surfaces_or_null);
/* brute force over all of `triangles` (primitive_id = the index): within.h on the host (ctx == NULL) or k_within_brute on uploaded copies.  The two agree bit
 * for bit.  near may be NULL when max_near == 0.  Refused: a NULL argument, max_near > RT_WITHIN_MAX, RT_WITHIN_K_NEAREST with max_near == 0, unknown
 * option bits. */
int rt_debug_within(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const rt_point* points, uint32_t n, uint32_t max_near,
                    uint32_t options, rt_point_hits* out, rt_nearest* near);
/* the kernel's walk on the host (no device), over the child-pair form of `nodes` (wide = 0) or build_wide_bvh's 4-wide records of them (wide = 1), with the
 * bound above; triangles_tested_or_null[i] = how many triangles point i was tested against.  Refused where rt_debug_nearest_walk is, and as rt_debug_within. */
int rt_debug_within_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide,
                         const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near,
                         uint32_t* triangles_tested_or_null);

/* ---- overlap: every triangle a CALLER's convex region -- a box, a slab, a frustum, up to 8 half-spaces -- touches or encloses (opt-in extension; DESIGN.md
 * section 7m).  What lies inside a box, which cells of a grid the surface touches, which objects a trigger volume contains, what is under a dragged
 * rectangle on screen.  raytracing_amd/csrc/region.h states the rule.
 *   a region: plane k = (nx, ny, nz, d), s_k(x) = ((nx x0 + ny x1) + nz x2) + d in binary32, each product and sum rounded once; x is outside plane k exactly
 *     when s_k(x) > 0 (on the plane is inside; a NaN s is not outside).  Normals need not have unit length.  SEARCHED: 1 <= num_planes <= 8 and every one of
 *     the 4 * num_planes coefficients finite; `reserved` is ignored.
 *   a triangle, on its shading record's three corners: REJECTED when some plane has all three outside, INSIDE when no plane has any outside, CROSSING
 *     otherwise; TOUCHING = inside or crossing.  This is the usual conservative cull: a crossing triangle near an edge or a corner of the region need not
 *     intersect it; a triangle that does intersect it is never rejected.  Inside is exact for the rounded s.
 *   rt_region_hits: count = the touching triangles, inside = the inside ones, stored = min(count, max_list), flags bit 0 = searched.
 *   members (optional, max_list <= RT_REGION_LIST_MAX per region): the touching triangles with the LOWEST primitive ids, ascending -- an order no tree
 *     enters; a smaller max_list gives a prefix.  flags bit 0: inside; bit 8 + k: plane k has 1 or 2 corners outside.  Beyond `stored`: RT_INVALID_ID / 0.
 *   a region that is not searched gives zeros and invalid entries.
 *   The sets are a statement about triangles and region.h alone -- bit for bit rt_debug_overlap's brute force, whichever records are walked, after any
 *     refit or pose: a box is skipped only when one plane has the box's nearest corner outside, and then, in binary32 itself, every corner inside the box
 *     is outside that plane (region.h has the argument).
 * Runs on the context's stream like a within query, touches no frame and no rt_stats field, and uses the ray queries' spill area, status word and staging
 * arrays.
 *   rt_scene_overlap: host arrays, staged in chunks of at most 4 Mi member records; returns when the outputs are written.
 *   rt_scene_overlap_buffer: rt_buffers of this context (n rt_region, n rt_region_hits, n * max_list rt_region_member); only enqueues.
 * Refused with nothing launched: a NULL context, no scene, NULL regions with n > 0, out NULL, max_list > RT_REGION_LIST_MAX, members with max_list == 0, a
 * buffer of another context or too small.  n == 0 is RT_OK and does nothing. */
#define RT_REGION_MAX_PLANES 8
#define RT_REGION_LIST_MAX 8
#define RT_REGION_HITS_SEARCHED 1u          /* rt_region_hits.flags bit 0 */
#define RT_REGION_MEMBER_INSIDE 1u          /* rt_region_member.flags bit 0 */
#define RT_REGION_MEMBER_CROSSING_SHIFT 8   /* rt_region_member.flags bit 8 + k: plane k has 1 or 2 of the corners outside */
#define RT_SELECT_MAX_REGIONS 32
typedef struct rt_region { uint32_t num_planes; uint32_t reserved[3]; float planes[RT_REGION_MAX_PLANES][4]; } rt_region;      /* 144 bytes; plane k = (nx, ny, nz, d) */
typedef struct rt_region_hits { uint32_t count; uint32_t inside; uint32_t stored; uint32_t flags; } rt_region_hits;            /* 16 bytes */
typedef struct rt_region_member { uint32_t primitive_id; uint32_t flags; } rt_region_member;                                   /* 8 bytes */
int rt_scene_overlap(rt_ctx* ctx, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members_or_null);
int rt_scene_overlap_buffer(rt_ctx* ctx, rt_buffer* regions, uint32_t n, uint32_t max_list, rt_buffer* out, rt_buffer* members_or_null);
/* brute force over all of `triangles` (primitive_id = the index): region.h on the host (ctx == NULL) or k_region_brute on uploaded copies.  The two agree
 * bit for bit.  members may be NULL when max_list == 0.  Refused: a NULL argument, max_list > RT_REGION_LIST_MAX. */
int rt_debug_overlap(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const rt_region* regions, uint32_t n, uint32_t max_list,
                     rt_region_hits* out, rt_region_member* members);
/* the kernel's walk on the host (no device), over the child-pair form of `nodes` (wide = 0) or build_wide_bvh's 4-wide records of them (wide = 1), pruned by
 * region.h's box test; triangles_tested_or_null[i] = how many triangles region i was tested against.  Refused where rt_debug_within_walk is. */
int rt_debug_overlap_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide,
                          const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members,
                          uint32_t* triangles_tested_or_null);
/* The COMPLETE answer for a few regions (n <= RT_SELECT_MAX_REGIONS): one lane per triangle instead of one per region, no tree.  Bit r of touching[t] /
 * inside[t] (num_triangles words, BVH order) says triangle t touches / is inside region r; bit r of object_touching[o] is the OR of the object's triangles'
 * touching bits (the CAD "crossing" selection), bit r of object_inside[o] is set when the object has at least one triangle and every one of them is inside
 * (the "window" selection) -- made with atomic ORs and a finishing step, so they depend on no order.  The per-object words need rt_scene_set_objects and
 * hold its num_objects entries.  A region that is not searched sets no bit.  At least one output.
 *   rt_scene_select: host arrays; returns when the outputs are written.     rt_scene_select_buffer: rt_buffers of this context; only enqueues (the context
 *   keeps 4 bytes per object of scratch for the finishing step).
 * Refused with nothing launched: a NULL context, no scene, NULL regions, n == 0 or n > RT_SELECT_MAX_REGIONS, every output NULL, per-object outputs without
 * rt_scene_set_objects, a buffer of another context or too small. */
int rt_scene_select(rt_ctx* ctx, const rt_region* regions, uint32_t n, uint32_t* touching_or_null, uint32_t* inside_or_null, uint32_t* object_touching_or_null,
                    uint32_t* object_inside_or_null);
int rt_scene_select_buffer(rt_ctx* ctx, rt_buffer* regions, uint32_t n, rt_buffer* touching_or_null, rt_buffer* inside_or_null, rt_buffer* object_touching_or_null,
                           rt_buffer* object_inside_or_null);
/* the same over caller triangles: region.h on the host (ctx == NULL) or k_select on uploaded copies; the two agree bit for bit.  touching and inside are
 * required; the per-object outputs are written when object_of_triangle is given (every entry < num_objects). */
int rt_debug_select(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle_or_null, uint32_t num_objects,
                    const rt_region* regions, uint32_t n, uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside);
/* The marquee: the region of the INCLUSIVE pixel rectangle (x0, y0) .. (x1, y1) of the frame's current camera -- four side planes through the camera position
 * and the guide pass's directions at the rectangle's pixel corners, a near plane when t_near > 0, a far plane when t_far is finite (region.h fixes every
 * operand) -- then one rt_scene_select with that region: bit 0 of each word.  Any output may be NULL.  Refused: what rt_frame_pick refuses, x1 < x0,
 * y1 < y0, a rectangle outside the image, per-object outputs without rt_scene_set_objects. */
int rt_frame_pick_rect(rt_frame* frame, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far, rt_region* region_or_null,
                       uint32_t* touching_or_null, uint32_t* inside_or_null, uint32_t* object_touching_or_null, uint32_t* object_inside_or_null);
/* the rectangle's region on its own (host arithmetic only).  Refused: a NULL argument, an empty image, x1 < x0, y1 < y0, a rectangle outside the image. */
int rt_debug_rect_region(const rt_camera* camera, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far,
                         rt_region* out);

/* ---- cross: every triangle of the uploaded scene that a CALLER's triangle (a probe) crosses, and where (opt-in extension): contact and
 * collision work -- which scene triangles a probe mesh cuts and along which segment, which posed objects interpenetrate, whether a mesh cuts itself.
 * raytracing_amd/csrc/cross.h states the rule.
 *   a probe: three corners (every fourth component is ignored); SEARCHED when its nine coordinates are finite.
 *   CROSS(Q, T), T on its shading record's corners (rt_scene_nearest's operands): the closed boxes of the two corner triples overlap on every axis, AND the
 *     probe's plane (n = cross3(q2 - q1, q3 - q1), d = -dot(n, q1)) does not have T's three corners strictly on one side (skipped when n or d is not finite),
 *     AND one of six segment-triangle tests accepts: bits 0..2 = Q's edges q1->q2, q2->q3, q3->q1 against T, bits 3..5 = T's edges p1->p2, p2->p3, p3->p1
 *     against Q; two-sided Moeller-Trumbore, 0 <= t <= 1, a determinant that is zero or NaN rejects.  COPLANAR pairs therefore do not cross.
 *   rt_probe_hits: count = the crossing triangles, stored = min(count, max_list), first_primitive = the lowest crossing id (RT_INVALID_ID: none), flags bit 0
 *     = searched, bit 1 = an RT_CROSS_ANY answer.
 *   members (optional, max_list <= RT_CROSS_LIST_MAX per probe): the crossing triangles with the LOWEST primitive ids, ascending -- an order no tree decides;
 *     a smaller max_list gives a prefix; entries beyond `stored` hold RT_INVALID_ID and zeros.  flags = the accepting tests' bits; c0 / c1 = the point
 *     a + t * (b - a) of the lowest / second lowest set bit (one bit: c1 = c0).  In exact arithmetic a generic crossing sets exactly two bits and c0 c1 is
 *     the intersection segment; rounding may set one bit or three.
 *   RT_CROSS_ANY: the walk stops at the first member: count is 0 or 1, stored 0, first_primitive RT_INVALID_ID (which member is met first depends on the
 *     tree), flags bit 1 set; members must be NULL.
 *   a probe that is not searched gives zeros and invalid entries.
 *   The sets are a statement about triangles and cross.h alone -- bit for bit rt_debug_cross's brute force, whichever records are walked, after any refit or
 *     pose (cross.h has the argument).
 *   rt_scene_cross: host arrays, staged in chunks; returns when the outputs are written.  rt_scene_cross_buffer: rt_buffers of this context (n rt_probe,
 *     n rt_probe_hits, n * max_list rt_cross_member); only enqueues.
 *   rt_scene_cross_self / _buffer: probe i is scene triangle first + i (rt_scene_select's triangle order), nothing is uploaded.  A pair is SKIPPED (no member,
 *     not counted) when both are the same triangle or when some corner of one equals some corner of the other on all three coordinates (neighbours that share
 *     a vertex always touch).  RT_CROSS_OTHER_OBJECTS (self forms only; needs rt_scene_set_objects) also skips pairs of one object.
 * Refused with nothing launched: a NULL context, no scene, NULL probes with n > 0, out NULL, max_list > RT_CROSS_LIST_MAX, members with max_list == 0 or with
 * RT_CROSS_ANY, unknown option bits, RT_CROSS_OTHER_OBJECTS without objects or on a form that is not a self form, first + n beyond the scene, a buffer of
 * another context or one that is too small.  n == 0: RT_OK. */
#define RT_CROSS_LIST_MAX 8
#define RT_CROSS_ANY 1u                     /* options bit 0 */
#define RT_CROSS_OTHER_OBJECTS 2u           /* options bit 1 (self forms) */
#define RT_PROBE_HITS_SEARCHED 1u           /* rt_probe_hits.flags bit 0 */
#define RT_PROBE_HITS_ANY 2u                /* rt_probe_hits.flags bit 1 */
typedef struct rt_probe { float p1[4], p2[4], p3[4]; } rt_probe;                                                                  /* 48 bytes */
typedef struct rt_probe_hits { uint32_t count; uint32_t stored; uint32_t first_primitive; uint32_t flags; } rt_probe_hits;      /* 16 bytes */
typedef struct rt_cross_member { uint32_t primitive_id; uint32_t flags; float c0[3]; float c1[3]; } rt_cross_member;            /* 32 bytes */
int rt_scene_cross(rt_ctx* ctx, const rt_probe* probes, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members_or_null);
int rt_scene_cross_buffer(rt_ctx* ctx, rt_buffer* probes, uint32_t n, uint32_t max_list, uint32_t options, rt_buffer* out, rt_buffer* members_or_null);
int rt_scene_cross_self(rt_ctx* ctx, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members_or_null);
int rt_scene_cross_self_buffer(rt_ctx* ctx, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_buffer* out, rt_buffer* members_or_null);
/* brute force over all of `triangles` (primitive_id = the index): cross.h on the host (ctx == NULL) or k_cross_brute on uploaded copies.  The two agree bit
 * for bit.  members must be NULL when max_list == 0 or with RT_CROSS_ANY (as in the scene forms) and must be given otherwise.  Refused: a NULL argument,
 * max_list > RT_CROSS_LIST_MAX, unknown option bits, RT_CROSS_OTHER_OBJECTS, members with max_list == 0 or with RT_CROSS_ANY. */
int rt_debug_cross(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const rt_probe* probes, uint32_t n, uint32_t max_list,
                   uint32_t options, rt_probe_hits* out, rt_cross_member* members);
/* k_cross's walk on the host (no GPU): the child-pair form of `nodes` (wide == 0) or build_wide_bvh's 4-wide records of them (wide == 1), pruned by cross.h's
 * box tests; triangles_tested_or_null[i] = how many triangles probe i was tested against.  Refused where rt_debug_overlap_walk is. */
int rt_debug_cross_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_probe* probes,
                        uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members, uint32_t* triangles_tested_or_null);
/* brute force of the self form: probe i is triangles[first + i]; RT_CROSS_OTHER_OBJECTS needs object_of_triangle. */
int rt_debug_cross_self(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle_or_null, uint32_t first,
                        uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members);

/* ---- separation: the nearest triangle of the uploaded scene to a CALLER's triangle (a probe), how far it is and where the two closest points lie (opt-in
 * extension): the other half of contact work -- a probe that cuts nothing asks how far it is from the scene, posed objects ask how much
 * clearance is left between them.  A triangle's distance to the scene is not the minimum over its corners (rt_scene_nearest): edge against edge and a scene
 * corner against the probe's face are candidates too.  raytracing_amd/csrc/separation.h states the rule.
 *   a probe: rt_probe, three corners (every fourth component is ignored); SEARCHED when its nine coordinates are finite and max_distance >= 0 (one value per
 *     call; +inf is allowed, a NaN is not searched).
 *   SEP(Q, T), T on its shading record's corners: when CROSS(Q, T) holds (the cross family's verdict) the distance is 0, both points are that pair's first
 *     contact point c0 and the feature is 15.  Otherwise the least of fifteen candidates, the lowest index among equal ones: 0..2 a probe corner against T
 *     (rt_scene_nearest's point-triangle distance), 3..5 a corner of T against the probe, 6 + 3 i + j edge i of the probe against edge j of T (edges 1->2,
 *     2->3, 3->1; segment against segment, clamped into the segments' boxes).
 *   rt_separation: the triangle with the least SEP within max_distance, the lowest primitive id among equal ones -- an order no tree decides.  on_probe /
 *     on_scene = the two closest points, distance = sqrtf of the squared distance (0 for a crossing), feature = the winning candidate, flags =
 *     RT_SEPARATION_SEARCHED | RT_SEPARATION_FOUND | RT_SEPARATION_CROSSING.  Nothing found: primitive_id = RT_INVALID_ID and zeros (flags keeps SEARCHED).
 *   The answer is a statement about triangles and separation.h alone -- bit for bit rt_debug_separation's brute force, whichever records are walked, after any
 *     refit or pose (separation.h has the argument).
 *   rt_scene_separation: host arrays, staged in chunks; returns when the outputs are written.  rt_scene_separation_buffer: rt_buffers of this context (n
 *     rt_probe, n rt_separation); only enqueues.
 *   rt_scene_separation_self / _buffer: probe i is scene triangle first + i, nothing is uploaded.  A pair is SKIPPED when both are the same triangle or share
 *     a corner (the cross family's rule); RT_SEPARATION_OTHER_OBJECTS (self forms only; needs rt_scene_set_objects) also skips pairs of one object.  SEP is
 *     not symmetric to the last bit (the edge-pair routine is not): a caller that holds both directions of a pair takes the smaller.
 * Refused with nothing launched: a NULL context, no scene, NULL probes with n > 0, out NULL, unknown option bits, RT_SEPARATION_OTHER_OBJECTS without objects
 * or on a form that is not a self form, first + n beyond the scene, a buffer of another context or one that is too small.  n == 0: RT_OK. */
#define RT_SEPARATION_OTHER_OBJECTS 2u      /* options bit 1 (self forms), RT_CROSS_OTHER_OBJECTS' bit */
#define RT_SEPARATION_SEARCHED 1u           /* rt_separation.flags bit 0 */
#define RT_SEPARATION_FOUND 2u              /* rt_separation.flags bit 1 */
#define RT_SEPARATION_CROSSING 4u           /* rt_separation.flags bit 2 */
#define RT_SEPARATION_FEATURE_CROSSING 15u  /* rt_separation.feature of a crossing pair */
typedef struct rt_separation { float on_probe[3]; float distance; float on_scene[3]; uint32_t primitive_id;
                               uint32_t flags; uint32_t feature; uint32_t pad[2]; } rt_separation;                               /* 48 bytes */
int rt_scene_separation(rt_ctx* ctx, const rt_probe* probes, uint32_t n, float max_distance, uint32_t options, rt_separation* out);
int rt_scene_separation_buffer(rt_ctx* ctx, rt_buffer* probes, uint32_t n, float max_distance, uint32_t options, rt_buffer* out);
int rt_scene_separation_self(rt_ctx* ctx, uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_separation* out);
int rt_scene_separation_self_buffer(rt_ctx* ctx, uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_buffer* out);
/* brute force over all of `triangles` (primitive_id = the index): separation.h on the host (ctx == NULL) or k_separation_brute on uploaded copies.  The two
 * agree bit for bit.  Refused: a NULL argument. */
int rt_debug_separation(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const rt_probe* probes, uint32_t n, float max_distance,
                        rt_separation* out);
/* k_separation's walk on the host (no GPU): the child-pair form of `nodes` (wide == 0) or build_wide_bvh's 4-wide records of them (wide == 1), the nearest
 * box first, pruned by separation.h's bound; triangles_tested_or_null[i] = how many triangles probe i was handed at a leaf.  Refused where
 * rt_debug_nearest_walk is. */
int rt_debug_separation_walk(const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, int wide, const rt_probe* probes,
                             uint32_t n, float max_distance, rt_separation* out, uint32_t* triangles_tested_or_null);
/* brute force of the self form: probe i is triangles[first + i]; RT_SEPARATION_OTHER_OBJECTS needs object_of_triangle. */
int rt_debug_separation_self(rt_ctx* ctx_or_null, const rt_triangle* triangles, uint32_t num_triangles, const uint32_t* object_of_triangle_or_null,
                             uint32_t first, uint32_t n, float max_distance, uint32_t options, rt_separation* out);

/* One fold adaptation per process GROUP instead of one per rank (N ranks that tile one image hold the same scene and would each probe, rotate and fold for
 * identical records): the context's current 4-wide records -- the closest-hit rays' and the shadow rays' (n_shadow == 0: they share), as adapted so far -- to
 * host buffers of `capacity` records each (records NULL: size query; entries2 = {closest entry, shadow entry}), and into another context that has uploaded
 * the SAME scene (same triangle order): they replace its own, its adaptation is switched off.  The launcher's channel carries the bytes in between (bench.py:
 * torch.distributed).  Any fold of the same tree is exact: results do not change.  The importer refuses -- "... do not fit this scene (<the defect>)", the
 * context left as it was -- records that are not a tree from the entry over exactly this scene's leaves, each reached once by its first triangle, at most
 * 33 record levels deep, with slot counts and frames as build_wide_bvh writes them (records the entry does not reach are tolerated, their refs range-checked).
 * A scene whose root is a leaf has no 4-wide tree: the export refuses it, and the import refuses a record count of 0. */
int rt_scene_export_folds(rt_ctx* ctx, void* closest_records, void* shadow_records, uint32_t capacity, uint32_t* n_closest, uint32_t* n_shadow, uint32_t* entries2);
int rt_scene_import_folds(rt_ctx* ctx, const void* closest_records, uint32_t n_closest, uint32_t entry_closest, const void* shadow_records, uint32_t n_shadow, uint32_t entry_shadow);

/* ---- frame: the per-pixel state CLPathTraceIntegrator allocates in its ctor
 * (cl_pt_integrator.cpp:188-259).  A frame renders a TILE of the full image:
 * the rows whose band index (row / band_height) is congruent to tile_rank
 * modulo tile_count.  tile_count == 1 is the whole image.  Random numbers are
 * keyed by GLOBAL pixel coordinates, so any tiling yields identical pixels. */
typedef struct rt_frame_desc
{
    uint32_t width, height;      /* full image */
    uint32_t tile_rank;          /* 0 .. tile_count-1 */
    uint32_t tile_count;         /* >= 1 */
    uint32_t band_height;        /* rows per interleaved band (>= 1) */
} rt_frame_desc;

/* A frame borrows its context: destroy every frame before rt_ctx_destroy. */
int rt_frame_create(rt_ctx* ctx, const rt_frame_desc* desc, rt_frame** out);
int rt_frame_destroy(rt_frame* frame);
/* number of rows / pixels this tile owns, and the global row of local row r */
uint32_t rt_frame_local_rows(rt_frame* frame);
uint32_t rt_frame_global_row(rt_frame* frame, uint32_t local_row);

/* ---- integrator state (Integrator public API, integrator.hpp:52-62) */
enum rt_option
{
    RT_OPT_MAX_BOUNCES = 0,    /* Integrator::SetMaxBounces, default 3 (integrator.hpp:91) */
    RT_OPT_WHITE_FURNACE = 1,  /* Integrator::EnableWhiteFurnace (-D ENABLE_WHITE_FURNACE) */
    RT_OPT_SAMPLER = 2,        /* Integrator::SetSamplerType: 0 = kRandom, 1 = kBlueNoise (-D BLUE_NOISE_SAMPLER) */
    RT_OPT_AOV = 3,            /* Integrator::SetAOV: 0 shaded colour, 1 diffuse albedo, 2 depth, 3 normal, 4 motion vectors
                                  (resolve_radiance.cl:25-29); per-pixel, so it works on tiles */
    RT_OPT_DENOISER = 4,       /* Integrator::EnableDenoiser: 1 = temporal reprojection (denoiser.cl) in the frame itself
                                  (needs tile_count == 1: it reprojects across rows); 2 = the frame prepares the filter's
                                  inputs only and rt_group_denoise runs it on the gathered image (the mode for tiles) */
    RT_OPT_TRACE_DROP_LAST_BOUNCE_RAYS = 5, /* 1 (default): do not emit the never-traced rays of the last bounce */
    RT_OPT_PROFILE_KERNELS = 6, /* 1: bracket every kernel launch with HIP events on the context stream */
    RT_OPT_TRACE_VARIANT = 7    /* traversal kernel: 0 = k_trace_v1 (per-ray loop; tiny launches); 8 / 9 = k_trace2 (exact BVH2
                                   walk in separate wave-uniform node / triangle / refill loops) with a 10+12 / 12+12 entry
                                   LDS stack (closest + shadow); 10 (11: 16-entry LDS stack) = k_trace_w4 (4-wide quantized
                                   tree, exact leaf re-test; rays it cannot take -- non-finite 1/dir -- go to k_trace2);
                                   5 (default) = auto: k_trace_w4 wherever the tree qualifies.  Results are identical for
                                   every value.  (1..4, 6, 7 -- round 1's flat state-machine kernel -- and 12..15 -- stack-size
                                   sweeps and the direct-visit form, which now IS k_trace_w4 -- were removed in round 3.) */
    , RT_OPT_TRACE_WAVES_PER_CU = 8 /* persistent-grid size of the trace kernels in waves per CU (0 = as many as fit) */
    , RT_OPT_SAMPLES_IN_FLIGHT = 9  /* rt_integrate traces this many consecutive samples per pixel concurrently
                                       (1..1024, allocated at once; 0 = auto, the default: as many (<= 1024) as keep
                                       the per-path buffers under ~144 GB, allocated as batches ask for them).  Results are bit-identical for every value: contributions
                                       are logged per path and replayed in the reference's order. */
    , RT_OPT_TRACE_SELECT_FORM_BOX = 10 /* validation: 1 = every ray uses the reference's compare+select min/max in the
                                       slab test (trace_bvh.cl:85-97); by default only rays whose 1/dir has a
                                       non-finite component do (the only ones for which v_min/v_max_f32 could
                                       differ).  Results are identical for both values. */
    , RT_OPT_TRACE_PACKET_BOUNCES = 11 /* removed in round 3 (the packet kernel lost on every measured launch:
                                       profiles/r02_packet_kernel_on_coherent_bounces.log); only 0 is accepted */
    , RT_OPT_DEBUG_ALLOC_LIMIT = 13 /* test hook: per-path buffer allocations for more than this many samples in flight
                                       fail as if the device were out of memory (0 = off) */
    , RT_OPT_PATH_STATE_LIMIT_MB = 14 /* upper bound (MiB) for the per-path buffers (ray queues + radiance log, 412 B per
                                       path at 8 bounces): rt_integrate then runs every batch of samples chunk by chunk
                                       over the tile's pixels instead of over the whole tile at once.  0 (default) = only
                                       the built-in rule (at most half of the HBM).  Results are bit-identical for every
                                       value: path ids, the log and the replay are per pixel. */
    , RT_OPT_PIPELINES = 15        /* 1..4 (default 1): pipes -- sets of per-path buffers, each with its own HIP stream --
                                       rt_integrate deals the tile's chunks to when a batch is large (>= 2 samples in
                                       flight, >= 4 M paths), so that chunks overlap.  Measured: no gain on MI355X
                                       (profiles/r02_pipelines_sweep.log), hence off by default.  Results are bit-identical
                                       for every value. */
    , RT_OPT_SHADE_PARTITION = 16  /* bit 0: k_shade processes each block's 512 queue entries hits first, misses last, so that
                                       a wave runs either the surface code or the environment lookup, not both; bit 1: each
                                       block's outgoing and shadow rays enter their queues grouped by direction octant, so that
                                       a wave of the next trace launch holds rays that start near each other and point the
                                       same way (closest-hit trace -2.8 %).  Default 3.  Results are identical for every value. */
    , RT_OPT_OVERLAP_SHADOW = 17   /* 1 (default): inside rt_integrate the shadow trace of bounce b runs on a second,
                                       lower-priority stream beside the closest-hit trace and k_shade of bounce b + 1
                                       (both sides depend on k_shade(b) only; the shadow queue is double-buffered), so the
                                       ~0.8 ms in which a launch's last rays drain does not idle the machine.
                                       0: every launch on one stream.  Results are identical for both values. */
    , RT_OPT_SMALL_LAUNCH_PATHS = 18 /* trace launches of fewer rays than this run k_trace_w4 in CHUNK mode -- a wave takes 64
                                       consecutive rays, finishes all of them, takes the next 64; chunks are assigned statically,
                                       no refill of single lanes, no hand-out atomics -- decided inside the kernel from the live
                                       queue counter.  It is what makes the reference's own call pattern (one Integrate() per
                                       frame, one sample per pixel in flight) fast, and the late bounces of any batch.  Default
                                       3 000 000 -- 8 000 000 in the instance small batches launch (RT_OPT_TRACE_TAIL_PATHS), whose
                                       chunks refill their lanes; setting the option sets both; 0 = never.  Results are identical
                                       for every value. */
    , RT_OPT_COMPACT_LOG = 19      /* 1: rt_integrate batches of >= 8 samples in flight keep the radiance log COMPACT: six inline
                                       entries per path (a path of the benchmark scene logs 2.7 on average, 1 % more than six) +
                                       overflow blocks, bump-allocated one bounce ahead, for an eighth of the paths -- 290 instead
                                       of 412 bytes per path at 8 bounces, 314 instead of 604 at 16 -- at ~1.5 % of the throughput
                                       (k_shade's allocation step).  A batch that runs the pool dry (long-lived paths: a closed,
                                       lit room) is discarded and repeated in the full layout, which the frame then keeps
                                       (rt_stats.log_fallbacks).  0: always the full layout.  2 (default): compact exactly when the
                                       caller bounds the path state (RT_OPT_PATH_STATE_LIMIT_MB != 0: larger chunks, +2.9 % at
                                       32 GiB), full otherwise.  The stage calls (rt_generate_rays ... rt_advance_sample) always run
                                       on the full layout -- they have no batch to repeat -- and re-allocate a compact frame once.
                                       Results are bit-identical for every value. */
    , RT_OPT_DEBUG_LOG_POOL_DIV = 20 /* test hook: the overflow pool holds paths / value blocks (default 8) */
    , RT_OPT_TRACE_TAIL_LANES = 21  /* k_trace_w4's loop D, in the instance that launches known to be small take (a batch of fewer
                                       than RT_OPT_SMALL_LAUNCH_PATHS paths: the reference's one-sample-per-frame pattern): when
                                       this many or fewer lanes of a wave are still busy and none of the others can be refilled,
                                       every busy lane fetches its next record -- wide node or triangle -- and takes its step
                                       in the SAME pass: one memory round trip per step of the chunk's last, longest rays
                                       instead of one per kind of lane.  Default 40 (sweep: 2228 / 2332 / 2479 / 2501 / 2488
                                       Mrays/s per frame at 0 / 16 / 32 / 40 / 48); 0 = off.  Results are identical for every value. */
    , RT_OPT_TRACE_TAIL_PATHS = 22  /* batches of fewer paths than this (tile pixels x samples in flight; default 100 000 000: it pays up to ~32 samples of a 1080p frame in flight and costs 2 - 3 % at 128) launch the
                                       k_trace_w4 instance that has loop D.  Results are identical for every value. */
    , RT_OPT_CHUNK_REFILL = 23      /* k_trace_w4's chunk mode (small launches): 1 (default) = a wave's statically assigned chunks are its
                                       private queue and a lane that finishes takes the next ray of it at once (no atomics, no
                                       machine-wide tail); 0 = round 3's form, a wave finishes all 64 rays of a chunk before it takes
                                       the next.  Results are identical for both. */
    , RT_OPT_STAGE_PIPES = 24       /* 1..4 (default 1): ONE sample per pixel in flight -- the stage API (the reference's frame-by-frame
                                      pattern, Render::RenderFrame -> Integrator::Integrate, src/render.cpp:197) and rt_integrate(f, 1) --
                                      is cut into this many chunks of the tile (>= 512 x 512 pixels), each travelling through the
                                      wavefront loop on a pipe (HIP stream + per-path buffers) of its own.  Every launch of that
                                      pattern is its own tail (a launch lasts as long as its longest ray); side by side the chunks'
                                      tails overlap.  Same image bit for bit (chunks are independent; path ids are chunk-relative).
                                      Not with RT_OPT_AOV / RT_OPT_DENOISER (whole tile); the debug readers want 1. */
    , RT_OPT_FRAME_KERNEL = 25      /* 0 (default) / 1 / k = 2 .. 64 (k chunks of 64 pixels per wave: more or fewer blocks than are resident; measured: never
                                      better than 1) / 255 (the choice is MEASURED: after four warm-up frames, frames 4 - 19 of a scene alternate between the stage kernels
                                      and k_frame, timed with HIP events around each frame's launches, and the faster way stays until the next rt_scene_upload:
                                      k_frame wins 1.4 - 1.8 x on scenes of up to ~1 M triangles and loses 7 - 10 % on 2.8 M / 10 M): ONE sample per pixel in flight through the stage API -- the reference's frame-by-frame pattern,
                                      Integrator::Integrate through the fifteen hooks -- as ONE launch: the stage calls of a sample are recorded while
                                      they come in the canonical order (rt_generate_rays; rt_intersect, rt_shade, rt_intersect_shadow for bounce 0 ..
                                      max_bounces; rt_advance_sample) and rt_advance_sample launches k_frame, in which every wave carries its own
                                      pixels through all the bounces (raytracing_amd/csrc/frame_kernels.h).  Any other order, a debug reader or the
                                      radiance between two stages replays the recorded stages with the stage kernels first.  Same radiance and ray
                                      counters bit for bit.  Not with AOVs / the denoiser, the compact log, RT_SCENE_EMISSIVE_NEE or profiling
                                      (those samples take the stage kernels). */
    , RT_OPT_SAMPLES_AHEAD = 26     /* 0 (default: off) / 1 (automatic depth: batches of ~32 M paths, i.e. 16 samples of a 1080p frame) / k = 2 .. 64 samples per batch;
                                      + 256: the two banks launch on a stream each (their batches overlap) instead of one after the other on one stream.
                                      The stage API -- the reference's frame-by-frame pattern, one Integrate() per frame at one sample per pixel,
                                      src/render.cpp:197 -- traces the NEXT samples of a standing camera ahead: after three samples without rt_reset the frame
                                      enqueues batches of 2, 4, .. k consecutive samples (rt_integrate's launches, its radiance log left unreplayed) into two
                                      banks beside its own stream, and a later sample that sits in a bank costs its Integrate() one replay of that sample's log
                                      slot -- the radiance after EVERY call is the reference's, bit for bit, sample by sample.  rt_reset, another camera or
                                      option, rt_scene_upload, rt_integrate and anything that looks between two stages drop what was traced ahead (at most
                                      2 k samples of device time, once; a camera that moves every frame never starts the mode).  The image of a frame is
                                      what it always was; what changes is WHEN the work is done: a launch of one sample per pixel is its own tail (3.3 ms per
                                      1080p frame of the 2.8 M-triangle scene where the rays are worth 1.6), a launch of k is not.  Costs: two more sets of
                                      per-path buffers for k samples in flight (within 64 GiB, or RT_OPT_PATH_STATE_LIMIT_MB); rt_stats' ray totals run ahead of
                                      its sample count by rt_stats.samples_ahead.  Not with AOVs / the denoiser / RT_OPT_STAGE_PIPES / profiling. */
    , RT_OPT_FUSED_RAYGEN = 27      /* 1 (default) / 0: inside rt_integrate the bounce-0 closest-hit trace of a batch makes its primary rays itself, from the queue
                                      index and the camera (the function k_raygen uses: the same bits), and leaves only their directions and path ids for the
                                      bounce-0 k_shade, which knows the throughput to be 1 and the log to be empty; k_raygen runs as one block that folds and
                                      resets the counters.  16 bytes per primary path written and read instead of 48 written and 64 read.
                                      0: k_raygen writes the queue and the bounce-0 launches read it, as the stage calls (rt_generate_rays ...), the banks of
                                      RT_OPT_SAMPLES_AHEAD and k_frame always do.  Batches whose primary queue somebody else reads (RT_OPT_AOV / RT_OPT_DENOISER,
                                      rt_frame_debug_timeline) or whose trace variant has no primary instance (RT_OPT_TRACE_VARIANT other than 5 / 10, a scene
                                      without the wide tree) take the written queue whatever the value.  Results are bit-identical for both values. */
    , RT_OPT_TRACE_TUNE = 12       /* k_trace2 (variants 8, 9) loop thresholds: value & 255 = lanes that must hold an
                                       interior node for a wave to stay in the node loop, value >> 8 & 255 = lanes that
                                       must wait at a triangle for another pass of the triangle loop, value >> 16 & 255 = rays a wave takes
                                       from the queue per hand-out / 16 (k_trace_w4; 7 bits), value >> 24 = the fewest rays per lane a wave of
                                       the persistent grid is started for (k_trace_w4: the grid follows the live queue counter, the
                                       reference's "@TODO: use indirect dispatch"; 255 = every wave), bit 23 = chunk mode for every
                                       launch (RT_OPT_SMALL_LAUNCH_PATHS).  0 in a field = its default.
                                       Results are identical for every value. */
};
int rt_set_option(rt_frame* frame, int option, uint32_t value);    /* a value out of range is refused before anything is launched or waited for */
int rt_set_camera(rt_frame* frame, const rt_camera* camera);       /* SetCameraData, cl_pt_integrator.cpp:365-371 */

/* ---- stages: the protected virtuals Integrator::Integrate() schedules
 * (integrator.hpp:65-79, integrator.cpp:27-59).  The HIP backend fuses
 *   Miss + ClearCounter x2 + HitSurface          -> rt_shade
 *   TraceBvh(SHADOW_RAYS) + AccumulateDirectSamples -> rt_intersect_shadow
 * so rt_shade_miss / rt_clear_* / rt_accumulate_direct are accepted no-ops
 * kept for schedule compatibility. */
int rt_reset(rt_frame* frame);                          /* Reset */
int rt_generate_rays(rt_frame* frame);                  /* GenerateRays */
int rt_intersect(rt_frame* frame, uint32_t bounce);     /* IntersectRays */
int rt_shade_miss(rt_frame* frame, uint32_t bounce);    /* ShadeMissedRays (fused into rt_shade) */
int rt_clear_outgoing_counter(rt_frame* frame, uint32_t bounce);   /* ClearOutgoingRayCounter (no-op) */
int rt_clear_shadow_counter(rt_frame* frame);           /* ClearShadowRayCounter (no-op) */
int rt_shade(rt_frame* frame, uint32_t bounce);         /* ShadeSurfaceHits (+ miss) */
int rt_intersect_shadow(rt_frame* frame, uint32_t bounce);  /* IntersectShadowRays (+ accumulate) */
int rt_accumulate_direct(rt_frame* frame);              /* AccumulateDirectSamples (fused, no-op) */
int rt_compute_aovs(rt_frame* frame);                   /* ComputeAOVs (after rt_intersect(frame, 0)); no-op unless an AOV or the denoiser is on */
int rt_advance_sample(rt_frame* frame);                 /* AdvanceSampleCount */
int rt_denoise(rt_frame* frame);                        /* Denoise (TemporalAccumulation); no-op unless RT_OPT_DENOISER */
int rt_copy_history(rt_frame* frame);                   /* CopyHistoryBuffers */
/* fast path: n_samples x Integrate() enqueued without returning to the caller */
int rt_integrate(rt_frame* frame, uint32_t n_samples);
/* The per-path buffers (ray queues + radiance log) are sized by the largest batch of samples
 * requested so far and grow inside rt_integrate when a larger one arrives.  This call sizes
 * them ahead of time for rt_integrate(n_samples) -- clamped to RT_OPT_SAMPLES_IN_FLIGHT --
 * and returns the samples the frame can now keep in flight (like vector::reserve; no
 * reference counterpart: the reference allocates per-pixel state once, cl_pt_integrator.cpp:204-257). */
int rt_frame_reserve_samples(rt_frame* frame, uint32_t n_samples, uint32_t* reserved);

/* ---- output.  ResolveRadiance (resolve_radiance.cl:31-86) headless: RGBA32F,
 * local_rows x width, row-major.  rt_frame_read_radiance returns the running
 * SUM over samples (radiance_buffer_), rt_frame_resolve the tonemapped image. */
int rt_frame_resolve(rt_frame* frame, float* host_rgba);
/* The same stage as the reference runs it every frame -- ResolveRadiance, then Finish() (cl_pt_integrator.cpp:677-684): when
 * this returns every kernel of the frame has run, and the tonemapped image is ON ITS WAY to host_rgba (a copy stream of its
 * own, double-buffered on the device: the reference resolves into a GL image and nothing crosses PCIe; headless the image
 * overlaps the next frame's tracing instead).  host_rgba holds the frame after rt_frame_present_wait (or the next
 * rt_frame_resolve / rt_frame_destroy); presenting again into the same buffer is fine (the copies are ordered). */
int rt_frame_present(rt_frame* frame, float* host_rgba);
int rt_frame_present_wait(rt_frame* frame);
int rt_frame_read_radiance(rt_frame* frame, float* host_rgba);
/* device pointer of the running-sum radiance (float4[local_rows*width]) for
 * device-side gathers (RCCL) without a host bounce */
void* rt_frame_radiance_device_ptr(rt_frame* frame);
uint32_t rt_frame_sample_count(rt_frame* frame);

/* ---- spatial filter (opt-in extension; no reference counterpart): the edge-avoiding a-trous wavelet filter of Dammertz et al.
 * 2010 over the shaded colour, guided by first-hit albedo, normal and depth (raytracing_amd/csrc/spatial_filter.h states it
 * exactly).  A new output beside rt_frame_resolve: the frame's radiance and every other result are untouched.
 *   - pass i = 0 .. iterations-1 spaces its 5 x 5 B3-spline taps 2^i pixels apart; a tap's weight falls with the colour distance
 *     (sigma_color, tightened 2x per pass), 1 - dot of the normals (sigma_normal) and the relative depth step per pixel (sigma_depth);
 *   - RT_FILTER_DEMODULATE filters radiance / albedo and multiplies the albedo back afterwards (texture detail stays sharp);
 *   - pixels without a first hit, and pixels with a non-finite colour, pass through unchanged and give nothing to their neighbours.
 * The guides come from a primary pass of its own: one ray per pixel through the pixel CENTRE from the camera position (the lens
 * centre: the guides are sharp with an aperture too), traced once per camera / frame size / scene and cached on the frame.
 * Whole images only (the stencil crosses rows): a tile frame (tile_count > 1) is refused. */
#define RT_FILTER_DEMODULATE 1u    /* filter radiance / albedo, multiply the albedo back afterwards */
#define RT_FILTER_MAX_ITERATIONS 8u
typedef struct rt_filter_desc
{
    uint32_t iterations;           /* 0 .. 8; pass i spaces its 5x5 taps 2^i pixels apart; 0 = no filtering (rt_frame_resolve's image) */
    uint32_t flags;                /* RT_FILTER_DEMODULATE */
    float sigma_color, sigma_normal, sigma_depth;   /* each > 0 and finite */
} rt_filter_desc;
/* the defaults: the best mean of tools/filter_sweep.py's grid (tone-mapped MSE of filtered 4-spp frames against 1024-spp ones, relative to the
 * unfiltered 4-spp frame's, 128 x 128, 4 bounces: Cornell box 0.072, coverage scene 0.238) */
#define RT_FILTER_DESC_DEFAULT { 2u, RT_FILTER_DEMODULATE, 8.0f, 0.05f, 0.1f }

/* resolve + filter: the image rt_frame_resolve would return, filtered; RGBA float, alpha 1, synchronous.
 * Fails (frame untouched) for NULL arguments, desc values out of range, RT_OPT_AOV != 0 or a tile frame. */
int rt_frame_filter(rt_frame* frame, const rt_filter_desc* desc, float* host_rgba);
/* the guide images the filter uses for the frame's current camera (computed if stale): albedo RGBA (alpha 0), unit normal RGBA
 * (alpha 0), depth (RT_MAX_RENDER_DIST where the pixel-centre ray misses); any array may be NULL.  *passes (nullable) = how many
 * guide passes this frame has run so far. */
int rt_frame_read_guides(rt_frame* frame, float* albedo_rgba, float* normal_rgba, float* depth, uint32_t* passes);
/* the filter on caller arrays (HDR in, HDR out, no tone mapping; width x height, row-major): on the GPU of ctx, or the host
 * restatement of the same arithmetic when ctx == NULL.  The two agree bit for bit. */
int rt_debug_filter(rt_ctx* ctx, uint32_t width, uint32_t height, const float* hdr_rgba, const float* albedo_rgba,
    const float* normal_rgba, const float* depth, const rt_filter_desc* desc, float* out_hdr_rgba);

/* ---- temporal filter (opt-in extension; no reference counterpart): the spatiotemporal variance-guided filter (SVGF) of Schied et al.
 * 2017 for a moving camera's one-sample frames (raytracing_amd/csrc/temporal_filter.h states it exactly).  A new output
 * beside rt_frame_resolve and rt_frame_filter: the frame's radiance and every other result are untouched.  Per call:
 *   - reproject: every pixel's first hit (the spatial filter's guides) is projected into the PREVIOUS call's camera; bilinear taps whose depth
 *     and normal agree supply a colour history and the luminance moments (mu1, mu2) with their length L;
 *   - accumulate: the (demodulated) colour and moments blend into the history by max(alpha, 1 / L);
 *   - variance: mu2 - mu1^2 where L >= 4, a 7 x 7 spatial estimate elsewhere;
 *   - iterations a-trous passes whose colour weight scales with the variance (sigma_luminance); pass 0's output is the next call's history.
 * The history lives on the frame: made on first use, freed by rt_frame_destroy, dropped by rt_scene_upload and rt_frame_filter_history_reset.
 * Whole images only (a tile frame is refused), the shaded colour only (RT_OPT_AOV != 0 is refused), and not over the reference's temporal
 * denoiser (RT_OPT_DENOISER != 0 is refused: two temporal accumulations in a row). */
typedef struct rt_temporal_filter_desc
{
    uint32_t iterations;           /* 0 .. 8 variance-guided a-trous passes; pass i spaces its 5x5 taps 2^i pixels apart */
    uint32_t flags;                /* RT_FILTER_DEMODULATE */
    float alpha_color;             /* 0 .. 1: the least weight of this call's colour in the history (1 = no history) */
    float alpha_moments;           /* 0 .. 1: the same for the luminance moments */
    float sigma_luminance, sigma_normal, sigma_depth;   /* each > 0 and finite */
} rt_temporal_filter_desc;
/* the defaults: the best mean of tools/temporal_filter_sweep.py's grid (tone-mapped MSE of the last of 16 moving-camera 1-spp frames against
 * 1024 spp, relative to the unfiltered frame's, 128 x 128, 4 bounces: Cornell box 0.090, coverage scene 0.215) */
#define RT_TEMPORAL_FILTER_DESC_DEFAULT { 5u, RT_FILTER_DEMODULATE, 0.2f, 0.2f, 2.0f, 0.05f, 0.1f }

/* resolve + reproject + accumulate + filter: RGBA float, tone-mapped (Reinhard), alpha 1, synchronous; the history advances by this call.
 * alpha_color = 1 with zero iterations is rt_frame_resolve's image bit for bit.  Fails (frame and history untouched) for NULL arguments, desc
 * values out of range, a tile frame, RT_OPT_AOV != 0 or RT_OPT_DENOISER != 0. */
/* Moved geometry.  A history made before an rt_scene_upload is dropped.  A history made before an rt_scene_refit* is dropped too (a stale history on a moved
 * surface ghosts) unless RT_CTX_OPT_REFIT_MOTION kept the pose that refit replaced AND exactly one refit lies between the previous call and this one: then
 * every pixel with a first hit is reprojected from where its surface point WAS -- the hit's barycentrics on the same triangle of the kept pose, projected
 * through the previous call's camera -- and the tap's normal is tested against the normal the point had there; depth test, taps and everything after are the
 * ordinary rule (a standing camera reprojects too).  The kept pose is ONE deep: two or more refits between two calls give a fresh history.  That is a stated
 * limit; call the filter once per refit. */
int rt_frame_filter_temporal(rt_frame* frame, const rt_temporal_filter_desc* desc, float* host_rgba);
/* drop the history: every pixel misses at the next rt_frame_filter_temporal */
int rt_frame_filter_history_reset(rt_frame* frame);
/* the history after the last call: colour RGBA (demodulated with RT_FILTER_DEMODULATE; alpha 0), moments_len RGBA = (mu1, mu2, L, 0); L = 0
 * where nothing may reproject from (no first hit, a pass-through pixel, no call yet, a dropped history).  Either array may be NULL. */
int rt_frame_read_filter_history(rt_frame* frame, float* color_rgba, float* moments_len);
/* the temporal filter on caller arrays (width x height, row-major, 4 floats per pixel except depth): HDR in, HDR out (no tone mapping),
 * on the GPU of ctx or the host restatement of the same arithmetic when ctx == NULL; the two agree bit for bit.  prev_cam == NULL, or bytes
 * equal to cam's, reuse each pixel's own history (a standing camera); otherwise the history is reprojected from prev_cam with prev_normal /
 * prev_depth.  hist_color / hist_moments: the previous call's history (L = 0: none); the new history is written to the *_out arrays. */
int rt_debug_filter_temporal(rt_ctx* ctx, uint32_t width, uint32_t height, const rt_camera* cam, const rt_camera* prev_cam,
    const float* hdr_rgba, const float* albedo_rgba, const float* normal_rgba, const float* depth, const float* prev_normal_rgba,
    const float* prev_depth, const float* hist_color, const float* hist_moments, const rt_temporal_filter_desc* desc, float* out_hdr_rgba,
    float* hist_color_out, float* hist_moments_out);
/* the same with the motion images of moved geometry: prev_position_rgba = (where the pixel's first hit was at the previous call, 1), w = 0: no motion known
 * (the camera-only rule for that pixel); prev_pose_normal_rgba = (its unit normal there, 0).  Either NULL: rt_debug_filter_temporal exactly.  With both, the
 * history is reprojected (through prev_cam, or cam when prev_cam is NULL) also when the two cameras are equal. */
int rt_debug_filter_temporal_motion(rt_ctx* ctx, uint32_t width, uint32_t height, const rt_camera* cam, const rt_camera* prev_cam,
    const float* hdr_rgba, const float* albedo_rgba, const float* normal_rgba, const float* depth, const float* prev_normal_rgba,
    const float* prev_depth, const float* hist_color, const float* hist_moments, const float* prev_position_rgba,
    const float* prev_pose_normal_rgba, const rt_temporal_filter_desc* desc, float* out_hdr_rgba, float* hist_color_out, float* hist_moments_out);
/* the motion images for the frame's current camera and the pose the context's last refit replaced (guides and images computed if stale): per pixel
 * (previous position, 1) and (previous unit normal, 0); zeros where the pixel-centre ray misses, and everywhere while the context keeps no pose
 * (RT_CTX_OPT_REFIT_MOTION off at upload, or no refit yet).  Either array may be NULL.  A tile frame is refused.  32 bytes per pixel on the device, made
 * on first use. */
int rt_frame_read_guide_motion(rt_frame* frame, float* prev_position_rgba, float* prev_normal_rgba);
/* the motion images' kernel on caller data: n pixels, hits = 4 floats per pixel (u, v, the primitive index's bits, unused; an index >= num_triangles = no
 * hit), prev_triangles = the previous pose in the reference layout.  ctx == NULL: the host restatement; the two agree bit for bit. */
int rt_debug_guide_motion(rt_ctx* ctx, uint32_t n, const float* hits, const rt_triangle* prev_triangles, uint32_t num_triangles,
    float* out_position_rgba, float* out_normal_rgba);

/* ---- statistics: the queue counters the reference keeps in
 * ray_counter_buffer_[2] / shadow_ray_counter_buffer_ (cl_pt_integrator.hpp:85-86),
 * sampled per bounce and accumulated on the device. */
typedef struct rt_stats
{
    uint64_t closest_rays;        /* sum over samples and bounces of rays traced closest-hit */
    uint64_t shadow_rays;         /* ... of shadow rays traced */
    uint64_t samples;             /* Integrate() calls since the last reset */
    uint32_t last_active[64];     /* per-bounce counts of the most recent batch of samples in flight */
    uint32_t last_shadow[64];
    uint32_t samples_in_flight;        /* samples the per-path buffers hold at the moment */
    uint32_t samples_in_flight_limit;  /* != 0: a larger batch did not fit into device memory and was halved to this */
    uint64_t path_state_bytes;         /* size of the per-path buffers (ray queues + radiance log) */
    uint32_t stack_spills;             /* lane-steps of the traversal kernels with stack entries in the HBM spill area (beyond the
                                          LDS entries) since the last reset; a 32-bit diagnostic that wraps (the headline
                                          workload adds ~1.3 M per sample per pixel of the frame: read it over short runs) */
    uint32_t slow_rays;                /* rays with a non-finite 1/dir component that k_trace_w4 handed to the BVH2 kernel */
    uint32_t chunk_pixels;             /* pixels of the tile that travel through the wavefront loop together (the whole
                                          tile unless RT_OPT_PATH_STATE_LIMIT_MB splits it) */
    uint32_t pipelines;                /* pipes (HIP streams) the chunks are dealt to */
    uint32_t log_inline_entries;       /* != 0: the radiance log is in its compact layout with this many inline entries per path
                                          (RT_OPT_COMPACT_LOG); 0: the full layout, 2 (max_bounces + 1) entries per path */
    uint32_t log_fallbacks;            /* batches whose overflow pool ran dry and that were repeated in the full layout */
    uint32_t frame_kernel_samples;     /* samples of the stage API that went through k_frame in one launch (RT_OPT_FRAME_KERNEL), since the frame was created */
    uint32_t samples_ahead;            /* RT_OPT_SAMPLES_AHEAD: samples traced (or being traced) ahead of `samples` at the moment; closest_rays / shadow_rays
                                          INCLUDE their rays (the banks count per batch) */
    uint64_t samples_from_banks;       /* RT_OPT_SAMPLES_AHEAD: samples of the stage API that were replayed out of a batch traced ahead, since the frame was created */
    uint64_t fused_raygen_launches;    /* RT_OPT_FUSED_RAYGEN: chunks of rt_integrate's batches whose bounce-0 launches made their primary rays themselves, since the frame was created */
} rt_stats;
int rt_frame_get_stats(rt_frame* frame, rt_stats* out);
/* RT_OPT_FRAME_KERNEL's per-wave rows of the latest k_frame launch (diagnostics: rays per bounce and 100 MHz ticks per phase of every wave;
 * raytracing_amd/csrc/frame_kernels.h).  out may be NULL (size query). */
int rt_frame_debug_frame_rows(rt_frame* frame, uint32_t* out, uint32_t capacity_rows, uint32_t* n_rows, uint32_t* row_words);

/* ---- per-kernel timing (RT_OPT_PROFILE_KERNELS): HIP-event durations of the
 * launches since the option was switched on / since the last call, summed per
 * kernel class.  Synchronises the stream. */
typedef struct rt_profile
{
    double ms_raygen, ms_trace_closest, ms_shade, ms_trace_shadow;
    uint32_t n_raygen, n_trace_closest, n_shade, n_trace_shadow;
} rt_profile;
int rt_frame_get_profile(rt_frame* frame, rt_profile* out);

/* D2D copy of the running-sum radiance (float4[local_rows*width]) into a caller
 * buffer on the same device (e.g. a tensor handed to an RCCL gather); ordered
 * on the context stream and completed on return. */
int rt_frame_copy_radiance(rt_frame* frame, void* device_dst);

/* ---- device groups: one image tiled over several GPUs, ONE collective.
 * The reference drives a single device (src/gpu_wrappers/cl_context.cpp:89: one queue on devices_[0]);
 * this is the multi-GPU extension the integrators' pixel independence allows: every rank renders the
 * interleaved row bands rt_frame_desc gives it (tile_rank / tile_count / band_height), nothing is exchanged
 * while rendering, and rt_group_gather_radiance is the one RCCL gather (ncclGather over xGMI) of the
 * accumulated radiance to the root, which also puts the bands back into image order.
 *   - rt_group_create: all ranks in THIS process (one host thread may drive them; ncclCommInitAll);
 *   - rt_group_unique_id + rt_group_join: one process per GPU (torch.distributed.run, mpirun): rank 0
 *     creates the id, the launcher's own channel carries its RT_GROUP_ID_BYTES to the others, all join.
 * RCCL is loaded on first use (dlopen librccl.so.1); groups are not needed for single-GPU work. */
typedef struct rt_group rt_group;
#define RT_GROUP_ID_BYTES 128
int rt_group_create(int n, const int* device_ordinals, rt_group** out);
/* rt_group_create without this library's own one-rank-per-device check, so that the list reaches ncclCommInitAll whatever it
 * holds and RCCL's own answer comes back through rt_group_last_error: the wiring test of the in-process path on a one-GPU box
 * ({0, 0} must fail with RCCL's refusal).  Not for products. */
int rt_group_create_unchecked(int n, const int* device_ordinals, rt_group** out);
int rt_group_unique_id(void* id_bytes, size_t capacity);
int rt_group_join(int nranks, int rank, const void* id_bytes, int device_ordinal, rt_group** out);
int rt_group_size(rt_group* group);                     /* ranks in the group */
int rt_group_local_count(rt_group* group);              /* ranks living in this process */
int rt_group_local_rank(rt_group* group, int i);        /* global rank of local member i */
/* What RCCL reports for the communicator of local member i: *comm_ranks = ncclCommCount, *comm_user_rank =
 * ncclCommUserRank (either may be NULL).  rt_group_size echoes the caller's argument; this is the library's own
 * count, the evidence that the gather really spans N ranks.  A local group (no RCCL) reports 0 / -1. */
int rt_group_comm_count(rt_group* group, int i, int* comm_ranks, int* comm_user_rank);
/* frames[i] = the frame of local member i (its tile_rank must be that member's rank, tile_count the group
 * size).  On the process that owns `root`: host_rgba (may be NULL) receives height x width RGBA32F running
 * sums in image order, *device_rgba (may be NULL) the device copy of the same (valid until the next gather).
 * Stream-ordered after the frames' pending work; returns when the image is complete. */
int rt_group_gather_radiance(rt_group* group, rt_frame* const* frames, int root, float* host_rgba, void** device_rgba);
/* Temporal denoiser across tiles (denoiser.cl:27-79 reprojects across rows): after every rank has rendered ONE sample
 * of its tile with RT_OPT_DENOISER = 2, one gather carries radiance + depth + motion vectors to the root, which runs
 * TemporalAccumulation against its own history, copies the history and resolves.  On the root's process:
 * host_resolved_rgba / host_radiance_rgba (each may be NULL) receive the tonemapped frame / the filtered radiance. */
int rt_group_denoise(rt_group* group, rt_frame* const* frames, int root, float* host_resolved_rgba, float* host_radiance_rgba);
/* All ranks on ONE device, device copies instead of RCCL (which refuses two ranks per GPU): the plumbing / test
 * transport for boxes with a single GPU.  Same calls, same results. */
int rt_group_create_local(int n, int device_ordinal, rt_group** out);
int rt_group_destroy(rt_group* group);
const char* rt_group_last_error(rt_group* group);

/* ---- debug / parity access: copy a ray queue back in the reference's layouts.
 * which: 0 = incoming queue of `bounce` (rays_buffer_[bounce&1]), 1 = shadow queue.
 * Returns the element count through *count; arrays may be NULL. */
int rt_frame_debug_read_queue(rt_frame* frame, int which, uint32_t bounce, rt_ray* rays, uint32_t* pixel_indices,
    rt_float4* payload /* throughput (which=0) or direct light sample (which=1) */,
    uint32_t capacity /* elements the arrays can hold; all arrays NULL = size query */, uint32_t* count);
int rt_frame_debug_read_hits(rt_frame* frame, rt_hit* hits, uint32_t count);

/* Launch timeline of the closest-hit wide-tree kernel (k_trace_w4), per bounce: when its first wave started, when
 * the first wave found the queue dry, when its last wave left, in ticks of the 100 MHz wall clock.  arm = 1 clears
 * the record and starts recording, arm = 0 stops and reads out[64][6] (0 where nothing ran): the three times, the
 * most traversal steps any ray took, the slowest ray's ticks from hand-out to retirement and its steps; then
 * out[384 + i] = waves (of all recorded launches) that left in the i-th 25 us after their launch's queue ran dry.
 * tools/launch_timeline.py */
int rt_frame_debug_timeline(rt_frame* frame, int arm, unsigned long long* out);

/* The 4-wide quantized tree rt_scene_upload builds for k_trace_w4 from the reference's LinearBVHNode[]
 * (host only, no device needed): 64-byte records {origin.xyz, meta, lo[3], hi[3], ref[4], order (64 bits)} --
 * see build_wide_bvh in rt_hip.hip.  collapse: 1 = the SAH-optimal frontier per record (what rt_scene_upload uses),
 * 2 = two BVH2 levels per record (RT_CTX_OPT_WIDE_BVH's values).  records may be NULL (count query); roots (optional, with
 * records) receives the index of the BVH2 node each record folds.  Fails when the tree does not qualify. */
int rt_debug_wide_bvh(const rt_bvh_node* nodes, uint32_t num_nodes, int collapse, void* records, uint32_t* roots, uint32_t capacity,
    uint32_t* num_records, uint32_t* entry_ref);

/* The refit on its own: `nodes` (reference layout: first child at i + 1, second at offset > i + 1) and any fold of it (`records`, a tree over all num_records
 * from entry_ref; num_records may be 0) refitted to `triangles` -- out_nodes[num_nodes]: offsets, counts and axes untouched, leaf bounds = min / max over the leaf's
 * vertices, interior bounds = min / max of the children; out_records[num_records]: ref, order and slot placement untouched, frame and planes made again.  Either
 * output may be NULL.  ctx == NULL: the host restatement; otherwise refit.hip's kernels on ctx's device (the two agree bit for bit, bounds by value).
 * Returns RT_OK, RT_ERROR, or RT_REFIT_DISQUALIFIED: refitted, but a record no longer qualifies for k_trace_w4 (its bytes are left as they were). */
#define RT_REFIT_DISQUALIFIED 2
int rt_debug_refit(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, const void* records, uint32_t num_records,
                   uint32_t entry_ref, rt_bvh_node* out_nodes, void* out_records);
/* The pose on its own: out[num_triangles] = rest[num_triangles] with triangle i posed by matrix object_of_triangle[i] (rt_scene_pose's arithmetic; .w lanes,
 * texture coordinates, mtl_index and padding copied).  ctx == NULL: the host restatement; otherwise k_pose_triangles on uploaded copies, on ctx's device (the two
 * agree bit for bit).  Refused: a NULL array, no triangles, no objects, an index >= num_objects, a non-finite matrix entry. */
int rt_debug_pose(rt_ctx* ctx, const rt_triangle* rest, const uint32_t* object_of_triangle, uint32_t num_triangles, const float* matrices3x4, uint32_t num_objects,
                  rt_triangle* out);
/* The skin on its own: out[num_triangles] = rest[num_triangles] with corner c of triangle i blended by per_corner[3 i + c] from the palette (rt_scene_skin's
 * arithmetic; .w lanes, texture coordinates, mtl_index and padding copied).  ctx == NULL: the host restatement; otherwise k_skin_triangles on uploaded copies,
 * on ctx's device (the two agree bit for bit).  Refused: a NULL array, no triangles, num_bones == 0 or above 65536, a bone index >= num_bones, a non-finite
 * weight, a non-finite matrix entry. */
int rt_debug_skin(rt_ctx* ctx, const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t num_triangles, const float* matrices3x4, uint32_t num_bones,
                  rt_triangle* out);
/* The morph on its own: out[num_triangles] = rest[num_triangles] morphed by the targets and weights (rt_scene_morph's arithmetic).  ctx == NULL: the host
 * restatement; otherwise k_morph_triangles on uploaded copies, on ctx's device (the two agree bit for bit).  Refused: a NULL array, no triangles, more than
 * 1431655765 triangles (a corner index is 32 bits), host memory that runs out while the table is checked or transposed (never an exception), and what
 * rt_scene_set_morph refuses in a table or rt_scene_morph in the weights, with the same messages.
 * rt_debug_morph_skin: the same, then the skin per corner: rt_debug_skin(ctx, rt_debug_morph(ctx, ...), per_corner, matrices3x4) -- on the host that very
 * composition, on the device k_morph_skin_triangles' one pass. */
int rt_debug_morph(rt_ctx* ctx, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles,
                   const float* weights, rt_triangle* out);
int rt_debug_morph_skin(rt_ctx* ctx, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles,
                        const float* weights, const rt_skin_influence* per_corner, const float* matrices3x4, uint32_t num_bones, rt_triangle* out);
/* What the last rt_scene_upload measured when it chose the trees (one line per ray population; "" when it had no choice), then the
 * latest fold adaptation's line (RT_CTX_OPT_ADAPTIVE_FOLD).  The pointer is valid until the next rt_integrate or rt_scene_upload on
 * this context (an adaptation rewrites its line): copy it. */
const char* rt_scene_tree_report(rt_ctx* ctx);
/* The tree rt_scene_upload would give the shadow (shadow != 0) or closest-hit rays of this scene under RT_CTX_OPT_SHADOW_TREE /
 * RT_CTX_OPT_CLOSEST_TREE = mode (host only; needs sd->triangles, nodes, lights): its records and the report line. */
int rt_debug_choose_tree(const rt_scene_desc* sd, int shadow, uint32_t mode, void* records, uint32_t capacity, uint32_t* num_records,
    uint32_t* entry_ref, char* report, size_t report_len);
/* The backend's own binary tree over the LEAVES of a reference LinearBVHNode[] (own_bvh.h; host only): same linear layout,
 * leaves copied.  Metric of a box = iso_weight * (dx dy + dy dz + dz dx) / 2 + sum over dirs of the projected area along
 * that unit direction (3 floats each).  out_nodes may be NULL (count query: 2 * leaves - 1). */
int rt_debug_own_bvh(const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs,
    rt_bvh_node* out_nodes, uint32_t capacity, uint32_t* num_out);
/* rt_debug_wide_bvh with collapse = 1 and the SAH collapse weighing boxes by that metric (what rt_scene_upload does for
 * the own trees) */
int rt_debug_wide_bvh_metric(const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs,
    void* records, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref);

/* fold_kernels.h on its own: the SAH collapse of `nodes` run on ctx's device (metric: iso_weight < 0 = plain surface area, else as rt_debug_wide_bvh_metric;
 * weights: per node, or NULL) -- the records, the node each one tests, *seconds = what the device path took.  tests/test_gpu_device_fold.py compares it
 * with rt_debug_wide_bvh / rt_debug_wide_bvh_metric / rt_debug_adapt_fold record for record. */
int rt_debug_device_fold(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs, const double* weights,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, double* seconds);
/* RT_CTX_OPT_WIDE_LAYOUT = 1 on its own (host only): the records of a fold of `nodes` (and the node each one tests) permuted in place into (parent,
 * likeliest child) pairs, by the area of the children's boxes. */
int rt_debug_pair_layout(const rt_bvh_node* nodes, uint32_t num_nodes, void* records, uint32_t* roots, uint32_t num_records);
/* rt_scene_import_folds' check on its own (host only, no context, no HIP call): would a scene whose binary tree is `nodes` take `records` with that entry?
 * The leaves the records must cover are read from `nodes`.  RT_OK, or RT_ERROR with the importer's words for the defect in rt_last_error(NULL). */
int rt_debug_check_folds(const rt_bvh_node* nodes, uint32_t num_nodes, const void* records, uint32_t num_records, uint32_t entry_ref);
/* ploc_kernels.h on its own: a binary tree over the leaves of `nodes` built on ctx's device with the metric of rt_debug_own_bvh (the same layout comes back: out_nodes[2 leaves - 1];
 * NULL = count query); *seconds = the device path's time, *rounds = clustering rounds. */
int rt_debug_device_tree(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs, rt_bvh_node* out_nodes, uint32_t capacity,
    uint32_t* num_out, double* seconds, uint32_t* rounds, uint32_t radius /* 0 = the library's */, const float* frame_dir /* NULL = world axes */, double stretch);
/* ... and the host's fold for given per-node weights (what an adaptation folds with), for that comparison */
int rt_debug_wide_bvh_weights(const rt_bvh_node* nodes, uint32_t num_nodes, const double* weights, void* records, uint32_t* roots, uint32_t capacity,
    uint32_t* num_records, uint32_t* entry_ref);

/* The adaptation's crossing counts on their own: counts[num_nodes] = how many of the n_rays rays (origins_tmax: x, y, z, t_max per ray; directions: x, y, z, - per
 * ray) pass the slab test of each node of `nodes` within [0, t_max] (plain binary32: a weight, not a result); *truncated = nodes that passed while more than
 * RT_COUNT_STACK - 3 = 61 nodes of that ray's walk were pending: such a node is counted, the subtree below it is not walked (a chain of 62 or more interior nodes
 * with their leaves pending, first child deepest).  ctx == NULL: the host's walk (wide_bvh.cpp, count_box_passes); otherwise k_count_box_passes on ctx's device.
 * The two obey the same rule and agree count for count, truncated walks included. */
int rt_debug_count_box_passes(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays,
    uint32_t* counts, unsigned long long* truncated);

/* RT_CTX_OPT_ADAPTIVE_FOLD's host half on its own (no device): the fold of `nodes` adapted to n_rays rays (origins_tmax: x, y, z, t_max per
 * ray; directions: x, y, z, - per ray) -- its records (and, optional, the node each one tests), and cost2 = {the surface-area fold's, the adapted
 * fold's} box passes at record roots per ray; *cheaper = the adapted fold would be adopted. */
int rt_debug_adapt_fold(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, double* cost2, int* cheaper);

/* The shadow side of an adaptation exactly as the worker thread runs it (host only): `nodes` = the shadow rays' current binary tree under its
 * surface-area fold, `mode` = RT_CTX_OPT_ADAPTIVE_FOLD's value (bit 3: rotate the tree first, keep whichever fold is cheaper).  Out: the candidate's
 * records (+ the node each one tests), the tree they fold (out_tree[num_nodes]), cost2 = {current, candidate} box passes at record roots per ray,
 * *rotations.  Returns 1 = would be adopted, 0 = kept, < 0 = error (rt_last_error(NULL)). */
int rt_debug_adapt_shadow_side(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, uint32_t mode,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, rt_bvh_node* out_tree, double* cost2, uint32_t* rotations,
    const rt_triangle* triangles /* for mode bit 4 (may be NULL otherwise) */, uint32_t num_triangles, uint32_t* reordered /* records whose slots moved */);

/* What rt_scene_upload / rt_ctx_destroy do to an adaptation in flight (host only): a worker is started on `nodes` and the rays given (used as both
 * populations) and abandoned after delay_ms.  Returns the milliseconds abandoning took (the worker gives up at its next check), < 0 on an error;
 * *had_finished = the worker was done already. */
double rt_debug_fold_abandon(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, uint32_t mode,
    uint32_t delay_ms, int* had_finished);

/* RT_CTX_OPT_ADAPTIVE_FOLD bit 3's tree search on its own (host only; raytracing_amd/csrc/tree_rotate.h): the binary tree `nodes` (reference
 * layout) rotated to lower the number of box crossings of the rays given (as rt_debug_adapt_fold takes them) -- out_nodes[num_nodes] holds a binary
 * tree over the same leaves in the same layout; cost2 = crossings of interior boxes per ray before / after; *rotations = how many were made. */
int rt_debug_rotate_tree(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, int max_passes,
    rt_bvh_node* out_nodes, double* cost2, uint32_t* rotations, int moves /* bit 0: child <-> grandchild, bit 1: grandchild <-> grandchild */,
    double min_gain /* a move must save more than this share of the crossings at its node */);

/* RT_CTX_OPT_ADAPTIVE_FOLD's trigger on its own (host only): 1 when camera `now` has left the view the folds were adapted to -- position by more
 * than 3 % of scene_diagonal, direction by more than 20 degrees, field of view by more than a tenth -- else 0; -1 on a NULL argument. */
int rt_debug_fold_view_left(const rt_camera* adapted, const rt_camera* now, double scene_diagonal);

/* ---- kernel self-test hooks (known-answer tests of the device math):
 * evaluates fn over n inputs on the device.  fn: 0 sin, 1 cos, 2 tan, 3 pow(a,b),
 * 4 atan2(a,b), 5 acos, 6 sqrt, 7 a/b, 8 SampleRandom(bits of a.. as uints) */
int rt_debug_eval(rt_ctx* ctx, int fn, const float* a, const float* b, float* out, uint32_t n);

#ifdef __cplusplus
}
#endif
RT_STATIC_ASSERT(sizeof(rt_skin_influence) == 24, "rt_skin_influence");
RT_STATIC_ASSERT(sizeof(rt_morph_delta) == 32, "rt_morph_delta");
RT_STATIC_ASSERT(sizeof(rt_surface) == 64, "rt_surface");
RT_STATIC_ASSERT(sizeof(rt_bake_result) == 16 && sizeof(rt_bake_desc) == 20, "rt_bake_result / rt_bake_desc");
RT_STATIC_ASSERT(sizeof(rt_light_bake_result) == 32 && sizeof(rt_light_bake_desc) == 20, "rt_light_bake_result / rt_light_bake_desc");
RT_STATIC_ASSERT(sizeof(rt_texel) == 16 && sizeof(rt_atlas_desc) == 16 && sizeof(rt_atlas_stats) == 32, "rt_texel / rt_atlas_desc / rt_atlas_stats");
RT_STATIC_ASSERT(sizeof(rt_point) == 16 && sizeof(rt_nearest) == 32, "rt_point / rt_nearest");
RT_STATIC_ASSERT(sizeof(rt_ray_hits) == 16, "rt_ray_hits");
RT_STATIC_ASSERT(sizeof(rt_point_hits) == 16, "rt_point_hits");
#endif /* RT_HIP_H */
