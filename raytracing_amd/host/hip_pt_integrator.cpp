// hip_pt_integrator.cpp -- binds the Integrator stage hooks to the C-ABI.
// Mapping to the reference backend (src/integrator/cl_pt_integrator.cpp):
//   ctor (buffers :188-259)            -> rt_frame_create
//   UploadGPUData :373-456             -> rt_scene_upload
//   SetCameraData :365-371             -> rt_set_camera
//   Reset :497-508                     -> rt_reset
//   GenerateRays :516-520              -> rt_generate_rays
//   IntersectRays :522-539             -> rt_intersect
//   ShadeMissedRays :582-592           -> rt_shade_miss   (no-op: fused into rt_shade)
//   ClearOutgoingRayCounter :651-657   -> rt_clear_outgoing_counter (no-op: per-bounce counters)
//   ClearShadowRayCounter :659-663     -> rt_clear_shadow_counter   (no-op)
//   ShadeSurfaceHits :594-643          -> rt_shade
//   IntersectShadowRays :564-580       -> rt_intersect_shadow (+ accumulate)
//   AccumulateDirectSamples :645-649   -> rt_accumulate_direct (no-op: fused)
//   AdvanceSampleCount :510-514        -> rt_advance_sample
//   ComputeAOVs :541-562               -> rt_compute_aovs
//   Denoise / CopyHistoryBuffers :665-675 -> rt_denoise / rt_copy_history
//   ResolveRadiance :677-684           -> rt_frame_resolve (the frame's only host sync)
#include "hip_pt_integrator.hpp"
#include <cstdio>
#include <cstring>
#include "spatial_filter.h"       // sf_guide_dir: the guide pass's pixel-centre direction (PickThrough shares it with rt_frame_pick)
#include "acceleration_structure.hpp"
#include "scene.hpp"

namespace rt
{
HIPContext::HIPContext(int device_ordinal)
{
    if (rt_ctx_create(device_ordinal, &ctx_) != RT_OK)
        throw HIPException(std::string("Failed to create the HIP context: ") + rt_last_error(nullptr));
}

HIPContext::~HIPContext() { rt_ctx_destroy(ctx_); }

void HIPContext::Finish() const
{
    if (rt_finish(ctx_) != RT_OK) throw HIPException(rt_last_error(ctx_));
}

void HIPContext::LoadBlueNoiseTables(const std::string& path)
{
    const size_t n[3] = {65536, 131072, 131072};
    std::vector<unsigned char> raw(n[0] + n[1] + n[2]);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f || fread(raw.data(), 1, raw.size(), f) != raw.size())
    {
        if (f) fclose(f);
        throw HIPException("Failed to load the blue-noise sampler tables " + path);
    }
    fclose(f);
    std::vector<int> t(raw.begin(), raw.end());
    if (rt_upload_blue_noise_tables(ctx_, t.data(), t.data() + n[0], t.data() + n[0] + n[1]) != RT_OK)
        throw HIPException(rt_last_error(ctx_));
    has_blue_noise_ = true;
}

std::string HIPContext::DeviceName() const
{
    char name[256] = {0};
    int cu = 0;
    size_t mem = 0;
    rt_ctx_device_info(ctx_, name, sizeof(name), &cu, &mem);
    return std::string(name) + ", " + std::to_string(cu) + " CUs, " + std::to_string(mem >> 30) + " GiB";
}

void HIPPathTraceIntegrator::Check(int rc) const
{
    if (rc != RT_OK) throw HIPException(rt_last_error(context_.Get()));
}

HIPPathTraceIntegrator::HIPPathTraceIntegrator(std::uint32_t width, std::uint32_t height,
    AccelerationStructure& acc_structure, HIPContext& context, TileDesc tile)
    : Integrator(width, height, acc_structure), context_(context)
{
    rt_frame_desc fd = {width, height, tile.rank, tile.count, tile.band_height};
    tile_count_ = tile.count;
    Check(rt_frame_create(context_.Get(), &fd, &frame_));
    // a constructor that throws runs no destructor: whatever follows the frame's creation gives it back itself
    try
    {
        resolved_.assign((size_t)rt_frame_local_rows(frame_) * width * 4, 0.0f);
        CreateKernels();
        // Integrate() through the hooks is this class's whole purpose: let the backend MEASURE whether a frame is better served by its stage
        // kernels or by one k_frame launch (RT_OPT_FRAME_KERNEL = 255; bit-identical either way; SetFrameKernel(0) keeps the stage kernels)
        Check(rt_set_option(frame_, RT_OPT_FRAME_KERNEL, 255u));
        // ... and trace a standing camera's next samples ahead, in batches (RT_OPT_SAMPLES_AHEAD = 1: the image after every Integrate() is the same
        // bit for bit; a launch of k samples is not its own tail the way a launch of one is; SetSamplesAhead(0) switches it off)
        Check(rt_set_option(frame_, RT_OPT_SAMPLES_AHEAD, 1u));
    }
    catch (...)
    {
        rt_frame_destroy(frame_);
        frame_ = nullptr;
        throw;
    }
    // ResolveRadiance() lands here every frame (the reference resolves into a GL image, cl_pt_integrator.cpp:677-684):
    // page-locked, the read-back runs at the PCIe rate.  Best effort -- a refusal only costs speed.  Registered LAST: nothing
    // after it can throw and leave the vector's memory freed while still page-locked.
    resolved_pinned_ = !resolved_.empty() &&
        rt_host_register(context_.Get(), resolved_.data(), resolved_.size() * sizeof(float)) == RT_OK;
}

std::vector<float> const& HIPPathTraceIntegrator::GetResolvedImage() const
{
    Check(rt_frame_present_wait(frame_));
    return resolved_;
}

HIPPathTraceIntegrator::~HIPPathTraceIntegrator()
{
    if (frame_) rt_frame_present_wait(frame_);
    if (resolved_pinned_) rt_host_unregister(context_.Get(), resolved_.data());
    rt_frame_destroy(frame_);
}

void HIPPathTraceIntegrator::UploadGPUData(Scene const& scene, AccelerationStructure const& acc_structure)
{
    auto const& nodes = acc_structure.GetNodes();
    auto const& env = scene.GetEnvImage();
    rt_scene_desc sd = {};
    sd.triangles = (const rt_triangle*)scene.GetTriangles().data();
    sd.num_triangles = (uint32_t)scene.GetTriangles().size();
    sd.nodes = (const rt_bvh_node*)nodes.data();
    sd.num_nodes = (uint32_t)nodes.size();
    sd.materials = scene.GetMaterials().data();
    sd.num_materials = (uint32_t)scene.GetMaterials().size();
    sd.textures = scene.GetTextures().data();
    sd.num_textures = (uint32_t)scene.GetTextures().size();
    sd.texture_data = scene.GetTextureData().data();
    sd.num_texture_data = (uint32_t)scene.GetTextureData().size();
    sd.lights = scene.GetLights().data();
    sd.num_lights = (uint32_t)scene.GetLights().size();
    sd.emissive_indices = scene.GetEmissiveIndices().data();
    sd.num_emissive = (uint32_t)scene.GetEmissiveIndices().size();
    // opt-in extensions (rt_scene_desc): both absent = the reference's behaviour
    sd.material_texture_indices = scene.GetMaterialTextureIndices().empty() ? nullptr : scene.GetMaterialTextureIndices().data();
    sd.flags = scene.GetEmissiveNee() ? RT_SCENE_EMISSIVE_NEE : 0u;
    sd.env_rgba = (const float*)env.data.data();
    sd.env_width = env.width;
    sd.env_height = env.height;
    Check(rt_scene_upload(context_.Get(), &sd));
}

void HIPPathTraceIntegrator::SetRefittable(bool on)
{
    Check(rt_ctx_set_option(context_.Get(), RT_CTX_OPT_REFITTABLE, on ? 1u : 0u));
    refittable_ = on;
}

void HIPPathTraceIntegrator::SetRefitMotion(bool on)
{
    if (on && !refittable_) throw HIPException("SetRefitMotion: SetRefittable(true) first (RT_CTX_OPT_REFIT_MOTION needs RT_CTX_OPT_REFITTABLE)");
    Check(rt_ctx_set_option(context_.Get(), RT_CTX_OPT_REFIT_MOTION, on ? 1u : 0u));
}

void HIPPathTraceIntegrator::RefitGeometry(Triangle const* triangles, std::size_t count)
{
    Check(rt_scene_refit(context_.Get(), (const rt_triangle*)triangles, (uint32_t)count));
    RequestReset();
}

void HIPPathTraceIntegrator::SetObjects(std::uint32_t const* object_of_triangle, std::size_t triangle_count, std::uint32_t object_count)
{
    Check(rt_scene_set_objects(context_.Get(), object_of_triangle, (uint32_t)triangle_count, object_count));
}

void HIPPathTraceIntegrator::PoseObjects(float const* matrices3x4, std::size_t object_count)
{
    Check(rt_scene_pose(context_.Get(), matrices3x4, (uint32_t)object_count));
    RequestReset();
}

void HIPPathTraceIntegrator::SetSkin(rt_skin_influence const* per_corner, std::size_t triangle_count, std::uint32_t bone_count)
{
    Check(rt_scene_set_skin(context_.Get(), per_corner, (uint32_t)triangle_count, bone_count));
}

void HIPPathTraceIntegrator::SkinBones(float const* matrices3x4, std::size_t bone_count)
{
    Check(rt_scene_skin(context_.Get(), matrices3x4, (uint32_t)bone_count));
    RequestReset();
}

void HIPPathTraceIntegrator::SetMorph(rt_morph_delta const* deltas, std::uint32_t const* target_offsets, std::uint32_t target_count, std::size_t triangle_count)
{
    Check(rt_scene_set_morph(context_.Get(), deltas, target_offsets, target_count, (uint32_t)triangle_count));
}

void HIPPathTraceIntegrator::MorphTargets(float const* weights, std::size_t target_count)
{
    Check(rt_scene_morph(context_.Get(), weights, (uint32_t)target_count));
    RequestReset();
}

void HIPPathTraceIntegrator::MorphAndSkin(float const* weights, std::size_t target_count, float const* matrices3x4, std::size_t bone_count)
{
    Check(rt_scene_morph_skin(context_.Get(), weights, (uint32_t)target_count, matrices3x4, (uint32_t)bone_count));
    RequestReset();
}

void HIPPathTraceIntegrator::TraceRays(rt_ray const* rays, std::size_t count, bool any_hit, rt_hit* hits, std::uint32_t* occluded, rt_surface* surfaces)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::TraceRays: more than 2^32 - 1 rays in one call");
    Check(rt_scene_trace(context_.Get(), rays, (uint32_t)count, any_hit ? RT_QUERY_ANY_HIT : RT_QUERY_CLOSEST, hits, occluded, surfaces));
}

void HIPPathTraceIntegrator::NearestPoints(rt_point const* points, std::size_t count, rt_nearest* out, rt_surface* surfaces)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::NearestPoints: more than 2^32 - 1 points in one call");
    Check(rt_scene_nearest(context_.Get(), points, (uint32_t)count, out, surfaces));
}

void HIPPathTraceIntegrator::PointsWithin(rt_point const* points, std::size_t count, std::uint32_t max_near, std::uint32_t options, rt_point_hits* out,
    rt_nearest* near, rt_surface* surfaces)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::PointsWithin: more than 2^32 - 1 points in one call");
    Check(rt_scene_within(context_.Get(), points, (uint32_t)count, max_near, options, out, near, surfaces));
}

void HIPPathTraceIntegrator::TrianglesCross(rt_probe const* probes, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::TrianglesCross: more than 2^32 - 1 probes in one call");
    Check(rt_scene_cross(context_.Get(), probes, (uint32_t)count, max_list, options, out, members));
}

void HIPPathTraceIntegrator::SelfCross(std::uint32_t first, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::SelfCross: more than 2^32 - 1 probes in one call");
    Check(rt_scene_cross_self(context_.Get(), first, (uint32_t)count, max_list, options, out, members));
}

void HIPPathTraceIntegrator::TrianglesSeparation(rt_probe const* probes, std::size_t count, float max_distance, rt_separation* out)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::TrianglesSeparation: more than 2^32 - 1 probes in one call");
    Check(rt_scene_separation(context_.Get(), probes, (uint32_t)count, max_distance, 0u, out));
}

void HIPPathTraceIntegrator::SelfSeparation(std::uint32_t first, std::size_t count, float max_distance, std::uint32_t options, rt_separation* out)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::SelfSeparation: more than 2^32 - 1 probes in one call");
    Check(rt_scene_separation_self(context_.Get(), first, (uint32_t)count, max_distance, options, out));
}

void HIPPathTraceIntegrator::RegionsOverlap(rt_region const* regions, std::size_t count, std::uint32_t max_list, rt_region_hits* out, rt_region_member* members)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::RegionsOverlap: more than 2^32 - 1 regions in one call");
    Check(rt_scene_overlap(context_.Get(), regions, (uint32_t)count, max_list, out, members));
}

void HIPPathTraceIntegrator::SelectRegions(rt_region const* regions, std::uint32_t count, std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching,
    std::uint32_t* object_inside)
{
    Check(rt_scene_select(context_.Get(), regions, count, touching, inside, object_touching, object_inside));
}

void HIPPathTraceIntegrator::PickRect(std::uint32_t x0, std::uint32_t y0, std::uint32_t x1, std::uint32_t y1, float t_near, float t_far, rt_region* region,
    std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside)
{
    Check(rt_frame_pick_rect(frame_, x0, y0, x1, y1, t_near, t_far, region, touching, inside, object_touching, object_inside));
}

void HIPPathTraceIntegrator::PickRectThrough(Camera const& camera, std::uint32_t x0, std::uint32_t y0, std::uint32_t x1, std::uint32_t y1, float t_near, float t_far,
    rt_region* region, std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside)
{
    if (rt_frame_local_rows(frame_) != height_) throw HIPException("HIPPathTraceIntegrator::PickRectThrough: a tile frame: pick on a frame of the whole image");
    // rt_frame_pick_rect's region for this camera (region.h's region_of_rect through rt_debug_rect_region: the same host arithmetic), then its select
    rt_camera cam;
    static_assert(sizeof(cam) == sizeof(camera), "Camera is rt_camera");
    std::memcpy(&cam, &camera, sizeof(cam));
    rt_region g;
    if (rt_debug_rect_region(&cam, width_, height_, x0, y0, x1, y1, t_near, t_far, &g) != RT_OK)
        throw HIPException(std::string("HIPPathTraceIntegrator::PickRectThrough: ") + rt_last_error(nullptr));
    if (touching || inside || object_touching || object_inside) Check(rt_scene_select(context_.Get(), &g, 1u, touching, inside, object_touching, object_inside));
    if (region) *region = g;
}

void HIPPathTraceIntegrator::Pick(std::uint32_t x, std::uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface)
{
    Check(rt_frame_pick(frame_, x, y, ray, hit, surface));
}

rt_ray HIPPathTraceIntegrator::PickRayThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, char const* who) const
{
    if (rt_frame_local_rows(frame_) != height_) throw HIPException(std::string("HIPPathTraceIntegrator::") + who + ": a tile frame: pick on a frame of the whole image");
    if (x >= width_ || y >= height_) throw HIPException(std::string("HIPPathTraceIntegrator::") + who + ": the pixel is outside the image");
    // rt_frame_pick's ray for this camera: sf_guide_dir (spatial_filter.h, the guide pass's direction, the same binary32 arithmetic on the host), from the
    // camera position, t_min 0, t_max RT_MAX_RENDER_DIST
    rt_camera cam;
    static_assert(sizeof(cam) == sizeof(camera), "Camera is rt_camera");
    std::memcpy(&cam, &camera, sizeof(cam));
    float d[3];
    sf_guide_dir(cam, rt_tanf(0.5f * cam.fov), width_, height_, x, y, d);
    rt_ray r;
    r.origin = {cam.position.x, cam.position.y, cam.position.z, 0.0f};
    r.direction = {d[0], d[1], d[2], RT_MAX_RENDER_DIST};
    return r;
}

void HIPPathTraceIntegrator::TraceAllHits(rt_ray const* rays, std::size_t count, std::uint32_t max_hits, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::TraceAllHits: more than 2^32 - 1 rays in one call");
    Check(rt_scene_trace_all(context_.Get(), rays, (uint32_t)count, max_hits, out, hits, surfaces));
}

void HIPPathTraceIntegrator::PickAll(std::uint32_t x, std::uint32_t y, std::uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    Check(rt_frame_pick_all(frame_, x, y, max_hits, ray, out, hits, surfaces));
}

void HIPPathTraceIntegrator::PickAllThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, std::uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits,
    rt_surface* surfaces)
{
    const rt_ray r = PickRayThrough(camera, x, y, "PickAllThrough");
    Check(rt_scene_trace_all(context_.Get(), &r, 1u, max_hits, out, hits, surfaces));
    if (ray) *ray = r;
}

void HIPPathTraceIntegrator::PickThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface)
{
    const rt_ray r = PickRayThrough(camera, x, y, "PickThrough");
    rt_hit h;
    rt_surface s;
    Check(rt_scene_trace(context_.Get(), &r, 1u, RT_QUERY_CLOSEST, &h, nullptr, &s));
    if (ray) *ray = r;
    if (hit) *hit = h;
    if (surface) *surface = s;
}

void HIPPathTraceIntegrator::BakeOcclusion(void const* points, std::size_t count, rt_bake_desc const& desc, rt_bake_result* out)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::BakeOcclusion: more than 2^32 - 1 points in one call");
    Check(rt_scene_bake(context_.Get(), points, (uint32_t)count, &desc, out));
}

void HIPPathTraceIntegrator::OcclusionImageThrough(Camera const& camera, rt_bake_desc desc, float* out)
{
    if (!out) throw HIPException("HIPPathTraceIntegrator::OcclusionImageThrough: out is NULL");
    if (rt_frame_local_rows(frame_) != height_) throw HIPException("HIPPathTraceIntegrator::OcclusionImageThrough: a tile frame: bake on a frame of the whole image");
    rt_camera cam;
    std::memcpy(&cam, &camera, sizeof(cam));
    const float tan_half = rt_tanf(0.5f * cam.fov);
    const std::size_t n = (std::size_t)width_ * height_;
    std::vector<rt_ray> rays(n);
    for (std::uint32_t y = 0; y < height_; ++y)
        for (std::uint32_t x = 0; x < width_; ++x)
        {
            float d[3];
            sf_guide_dir(cam, tan_half, width_, height_, x, y, d);              // PickThrough's ray
            rt_ray& r = rays[(std::size_t)y * width_ + x];
            r.origin = {cam.position.x, cam.position.y, cam.position.z, 0.0f};
            r.direction = {d[0], d[1], d[2], RT_MAX_RENDER_DIST};
        }
    desc.flags |= RT_BAKE_FROM_SURFACES;
    rt_buffer *b_rays = nullptr, *b_surf = nullptr, *b_out = nullptr;
    std::vector<rt_bake_result> results(n);
    // rays up, surfaces and results stay on the device, 16 bytes per pixel come back
    int rc = rt_buffer_create(context_.Get(), n * sizeof(rt_ray), rays.data(), &b_rays);
    if (rc == RT_OK) rc = rt_buffer_create(context_.Get(), n * sizeof(rt_surface), nullptr, &b_surf);
    if (rc == RT_OK) rc = rt_buffer_create(context_.Get(), n * sizeof(rt_bake_result), nullptr, &b_out);
    if (rc == RT_OK) rc = rt_scene_trace_buffer(context_.Get(), b_rays, (uint32_t)n, RT_QUERY_CLOSEST, nullptr, nullptr, b_surf);
    if (rc == RT_OK) rc = rt_scene_bake_buffer(context_.Get(), b_surf, (uint32_t)n, &desc, b_out);
    if (rc == RT_OK) rc = rt_buffer_read(b_out, 0, results.data(), n * sizeof(rt_bake_result));
    const std::string why = rc == RT_OK ? std::string() : std::string(rt_last_error(context_.Get()));
    rt_buffer_destroy(b_rays); rt_buffer_destroy(b_surf); rt_buffer_destroy(b_out);
    if (rc != RT_OK) throw HIPException(why);
    for (std::size_t i = 0; i < n; ++i) out[i] = results[i].unoccluded == RT_INVALID_ID ? 1.0f : (float)results[i].unoccluded / (float)desc.samples;
}

void HIPPathTraceIntegrator::AtlasCover(rt_atlas_desc const& desc, float const* uv, rt_texel* texels, rt_atlas_stats* stats)
{
    Check(rt_scene_atlas(context_.Get(), &desc, uv, texels, stats));
}

void HIPPathTraceIntegrator::AtlasSurfaces(rt_texel const* texels, std::size_t count, rt_surface* surfaces)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::AtlasSurfaces: more than 2^32 - 1 records in one call");
    Check(rt_scene_atlas_surfaces(context_.Get(), texels, (uint32_t)count, surfaces));
}

void HIPPathTraceIntegrator::BakeAtlas(rt_atlas_desc const& atlas, float const* uv, rt_bake_desc const& desc, rt_bake_result* out, rt_texel* texels, rt_atlas_stats* stats)
{
    Check(rt_scene_atlas_bake(context_.Get(), &atlas, uv, &desc, out, texels, stats));
}

void HIPPathTraceIntegrator::BakeLight(void const* points, std::size_t count, rt_light_bake_desc const& desc, rt_light_bake_result* out)
{
    if (count > 0xFFFFFFFFull) throw HIPException("HIPPathTraceIntegrator::BakeLight: more than 2^32 - 1 points in one call");
    Check(rt_scene_light_bake(context_.Get(), points, (uint32_t)count, &desc, out));
}

void HIPPathTraceIntegrator::IrradianceImageThrough(Camera const& camera, rt_light_bake_desc desc, float* out)
{
    if (!out) throw HIPException("HIPPathTraceIntegrator::IrradianceImageThrough: out is NULL");
    if (rt_frame_local_rows(frame_) != height_) throw HIPException("HIPPathTraceIntegrator::IrradianceImageThrough: a tile frame: bake on a frame of the whole image");
    rt_camera cam;
    std::memcpy(&cam, &camera, sizeof(cam));
    const float tan_half = rt_tanf(0.5f * cam.fov);
    const std::size_t n = (std::size_t)width_ * height_;
    std::vector<rt_ray> rays(n);
    for (std::uint32_t y = 0; y < height_; ++y)
        for (std::uint32_t x = 0; x < width_; ++x)
        {
            float d[3];
            sf_guide_dir(cam, tan_half, width_, height_, x, y, d);              // PickThrough's ray
            rt_ray& r = rays[(std::size_t)y * width_ + x];
            r.origin = {cam.position.x, cam.position.y, cam.position.z, 0.0f};
            r.direction = {d[0], d[1], d[2], RT_MAX_RENDER_DIST};
        }
    desc.flags |= RT_BAKE_FROM_SURFACES;
    rt_buffer *b_rays = nullptr, *b_surf = nullptr, *b_out = nullptr;
    std::vector<rt_light_bake_result> results(n);
    // rays up, surfaces and results stay on the device, 32 bytes per pixel come back
    int rc = rt_buffer_create(context_.Get(), n * sizeof(rt_ray), rays.data(), &b_rays);
    if (rc == RT_OK) rc = rt_buffer_create(context_.Get(), n * sizeof(rt_surface), nullptr, &b_surf);
    if (rc == RT_OK) rc = rt_buffer_create(context_.Get(), n * sizeof(rt_light_bake_result), nullptr, &b_out);
    if (rc == RT_OK) rc = rt_scene_trace_buffer(context_.Get(), b_rays, (uint32_t)n, RT_QUERY_CLOSEST, nullptr, nullptr, b_surf);
    if (rc == RT_OK) rc = rt_scene_light_bake_buffer(context_.Get(), b_surf, (uint32_t)n, &desc, b_out);
    if (rc == RT_OK) rc = rt_buffer_read(b_out, 0, results.data(), n * sizeof(rt_light_bake_result));
    const std::string why = rc == RT_OK ? std::string() : std::string(rt_last_error(context_.Get()));
    rt_buffer_destroy(b_rays); rt_buffer_destroy(b_surf); rt_buffer_destroy(b_out);
    if (rc != RT_OK) throw HIPException(why);
    for (std::size_t i = 0; i < n; ++i)
        for (int q = 0; q < 3; ++q) out[3 * i + q] = results[i].sky[q] + results[i].lights[q];       // (a skipped point's are zeros)
}

void HIPPathTraceIntegrator::BakeLightAtlas(rt_atlas_desc const& atlas, float const* uv, rt_light_bake_desc const& desc, rt_light_bake_result* out, rt_texel* texels,
    rt_atlas_stats* stats)
{
    Check(rt_scene_atlas_bake_light(context_.Get(), &atlas, uv, &desc, out, texels, stats));
}

void HIPPathTraceIntegrator::SetCameraData(Camera const& camera)
{
    prev_camera_ = camera_;
    camera_ = camera;
    Check(rt_set_camera(frame_, &camera));
}

void HIPPathTraceIntegrator::SetSamplerType(SamplerType sampler_type)
{
    if (sampler_type == sampler_type_) return;
    if (sampler_type == SamplerType::kBlueNoise && !context_.HasBlueNoiseTables())
        context_.LoadBlueNoiseTables(blue_noise_path_);
    Check(rt_set_option(frame_, RT_OPT_SAMPLER, sampler_type == SamplerType::kBlueNoise ? 1u : 0u));
    sampler_type_ = sampler_type;
    RequestReset();
}

void HIPPathTraceIntegrator::SetAOV(AOV aov)
{
    if (aov == aov_) return;
    Check(rt_set_option(frame_, RT_OPT_AOV, (uint32_t)aov));
    aov_ = aov;
    RequestReset();
}

void HIPPathTraceIntegrator::EnableDenoiser(bool enable)
{
    if (enable == enable_denoiser_) return;
    if (enable && temporal_on_) throw HIPException("EnableDenoiser: the temporal filter is on (SetTemporalFilter): two temporal accumulations in a row");
    Check(rt_set_option(frame_, RT_OPT_DENOISER, enable ? 1u : 0u));
    enable_denoiser_ = enable;
    RequestReset();
}

// Kernel variants are compiled ahead of time for gfx950; "creating kernels"
// (cl_pt_integrator.cpp:261-363, a JIT build per variant) reduces to selecting them.
void HIPPathTraceIntegrator::CreateKernels() { SyncOptions(); }

void HIPPathTraceIntegrator::SyncOptions()
{
    Check(rt_set_option(frame_, RT_OPT_MAX_BOUNCES, max_bounces_));
    Check(rt_set_option(frame_, RT_OPT_WHITE_FURNACE, enable_white_furnace_ ? 1u : 0u));
}

void HIPPathTraceIntegrator::SetFrameKernel(std::uint32_t mode) { Check(rt_set_option(frame_, RT_OPT_FRAME_KERNEL, mode)); }
void HIPPathTraceIntegrator::SetSamplesAhead(std::uint32_t mode) { Check(rt_set_option(frame_, RT_OPT_SAMPLES_AHEAD, mode)); }
void HIPPathTraceIntegrator::Reset() { SyncOptions(); Check(rt_reset(frame_)); }
void HIPPathTraceIntegrator::AdvanceSampleCount() { Check(rt_advance_sample(frame_)); }
void HIPPathTraceIntegrator::GenerateRays() { SyncOptions(); Check(rt_generate_rays(frame_)); }
void HIPPathTraceIntegrator::IntersectRays(std::uint32_t bounce) { Check(rt_intersect(frame_, bounce)); }
void HIPPathTraceIntegrator::ComputeAOVs() { Check(rt_compute_aovs(frame_)); }
void HIPPathTraceIntegrator::ShadeMissedRays(std::uint32_t bounce) { Check(rt_shade_miss(frame_, bounce)); }
void HIPPathTraceIntegrator::ShadeSurfaceHits(std::uint32_t bounce) { Check(rt_shade(frame_, bounce)); }
void HIPPathTraceIntegrator::IntersectShadowRays() { Check(rt_intersect_shadow(frame_, current_bounce_)); }
void HIPPathTraceIntegrator::AccumulateDirectSamples() { Check(rt_accumulate_direct(frame_)); }
void HIPPathTraceIntegrator::ClearOutgoingRayCounter(std::uint32_t bounce) { Check(rt_clear_outgoing_counter(frame_, bounce)); }
void HIPPathTraceIntegrator::ClearShadowRayCounter() { Check(rt_clear_shadow_counter(frame_)); }
void HIPPathTraceIntegrator::Denoise() { Check(rt_denoise(frame_)); }
void HIPPathTraceIntegrator::CopyHistoryBuffers() { Check(rt_copy_history(frame_)); }

void HIPPathTraceIntegrator::ResolveRadiance()
{
    // the frame's kernels have finished when this returns (Finish(), cl_pt_integrator.cpp:682); the image travels to
    // resolved_ meanwhile and GetResolvedImage() waits for it
    if (!resolve_every_frame_) return;
    if (filter_on_) Check(rt_frame_filter(frame_, &filter_, resolved_.data()));      // synchronous: the filtered image is in resolved_ on return
    else if (temporal_on_) Check(rt_frame_filter_temporal(frame_, &temporal_, resolved_.data()));   // likewise
    else Check(rt_frame_present(frame_, resolved_.data()));
}

void HIPPathTraceIntegrator::SetSpatialFilter(rt_filter_desc const* desc)
{
    if (desc && tile_count_ > 1) throw HIPException("SetSpatialFilter: a tile of a larger image: the filter needs the whole image");
    if (desc && temporal_on_) throw HIPException("SetSpatialFilter: the temporal filter is on (SetTemporalFilter): switch it off first");
    if (desc) filter_ = *desc;
    filter_on_ = desc != nullptr;
}

void HIPPathTraceIntegrator::SetTemporalFilter(rt_temporal_filter_desc const* desc)
{
    if (desc && tile_count_ > 1) throw HIPException("SetTemporalFilter: a tile of a larger image: the filter needs the whole image");
    if (desc && filter_on_) throw HIPException("SetTemporalFilter: the spatial filter is on (SetSpatialFilter): switch it off first");
    if (desc && enable_denoiser_) throw HIPException("SetTemporalFilter: the denoiser is on (EnableDenoiser): two temporal accumulations in a row");
    if (desc) temporal_ = *desc;
    temporal_on_ = desc != nullptr;
}

void HIPPathTraceIntegrator::IntegrateSamples(std::uint32_t n_samples)
{
    if (request_reset_ || enable_denoiser_) { Reset(); request_reset_ = false; }
    SyncOptions();
    Check(rt_integrate(frame_, n_samples));
}

std::uint32_t HIPPathTraceIntegrator::ReserveSamples(std::uint32_t n_samples)
{
    SyncOptions();
    std::uint32_t reserved = 0;
    Check(rt_frame_reserve_samples(frame_, n_samples, &reserved));
    return reserved;
}

std::vector<float> HIPPathTraceIntegrator::ReadRadianceSum() const
{
    std::vector<float> out((size_t)rt_frame_local_rows(frame_) * width_ * 4);
    Check(rt_frame_read_radiance(frame_, out.data()));
    return out;
}

std::vector<float> const& HIPPathTraceIntegrator::ResolveNow()
{
    if (filter_on_) Check(rt_frame_filter(frame_, &filter_, resolved_.data()));
    else if (temporal_on_) Check(rt_frame_filter_temporal(frame_, &temporal_, resolved_.data()));
    else Check(rt_frame_resolve(frame_, resolved_.data()));
    return resolved_;
}

std::uint32_t HIPPathTraceIntegrator::GetSampleCount() const { return rt_frame_sample_count(frame_); }
std::uint32_t HIPPathTraceIntegrator::GetLocalRows() const { return rt_frame_local_rows(frame_); }
std::uint32_t HIPPathTraceIntegrator::GetGlobalRow(std::uint32_t r) const { return rt_frame_global_row(frame_, r); }

rt_stats HIPPathTraceIntegrator::GetStats() const
{
    rt_stats st;
    Check(rt_frame_get_stats(frame_, &st));
    return st;
}
} // namespace rt
