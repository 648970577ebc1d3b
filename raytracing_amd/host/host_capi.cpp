// host_capi.cpp -- flat C entry points over the C++ host layer (Scene, Bvh,
// Render, HIPPathTraceIntegrator) so that scripts and tests can drive it
// through ctypes.  Errors: functions return NULL / non-zero and the message is
// kept per thread (rth_last_error).
#include <cstring>
#include <string>
#include "render.hpp"

namespace
{
thread_local std::string g_err;
template <class F>
auto guard(F&& f, decltype(f()) fail_value) -> decltype(f())
{
    try { return f(); }
    catch (std::exception& e) { g_err = e.what(); return fail_value; }
}
} // namespace

extern "C" {

const char* rth_last_error() { return g_err.c_str(); }

// ---- Scene ----------------------------------------------------------------
void* rth_scene_load(const char* path, float scale, int flip_yz)
{
    return guard([&]() -> void* { return new rt::Scene(path, scale, flip_yz != 0); }, nullptr);
}

// options: rt::Scene::Options (1 = wide texture indices, 2 = emissive-triangle next-event estimation, 4 = number the OBJ's o / g shapes)
void* rth_scene_load_ex(const char* path, float scale, int flip_yz, unsigned options)
{
    return guard([&]() -> void* { return new rt::Scene(path, scale, flip_yz != 0, options); }, nullptr);
}
int rth_scene_set_material_texture_indices(void* s, const uint16_t* idx, uint32_t n)
{
    return guard([&]() { ((rt::Scene*)s)->SetMaterialTextureIndices(std::vector<uint16_t>(idx, idx + n)); return 0; }, 1);
}
void rth_scene_set_emissive_nee(void* s, int enable) { ((rt::Scene*)s)->SetEmissiveNee(enable != 0); }
int rth_scene_emissive_nee(void* s) { return ((rt::Scene*)s)->GetEmissiveNee() ? 1 : 0; }
uint32_t rth_scene_num_material_texture_indices(void* s) { return (uint32_t)((rt::Scene*)s)->GetMaterialTextureIndices().size(); }
const void* rth_scene_material_texture_indices(void* s) { return ((rt::Scene*)s)->GetMaterialTextureIndices().data(); }

void* rth_scene_from_arrays(const rt_triangle* tris, uint32_t ntris, const rt_packed_material* mats, uint32_t nmats,
    const rt_texture* tex, uint32_t ntex, const uint32_t* texdata, uint32_t ntexdata)
{
    return guard([&]() -> void*
    {
        std::vector<rt::Triangle> t(ntris);
        if (ntris) memcpy(static_cast<void*>(t.data()), tris, (size_t)ntris * sizeof(rt_triangle));
        std::vector<rt::PackedMaterial> m(mats, mats + nmats);
        std::vector<rt::Texture> tx(tex, tex + ntex);
        std::vector<uint32_t> td(texdata, texdata + ntexdata);
        return new rt::Scene(std::move(t), std::move(m), std::move(tx), std::move(td));
    }, nullptr);
}

// kObjects / SetTriangleObjects: names may be NULL (the objects are then unnamed)
int rth_scene_set_triangle_objects(void* s, const uint32_t* ids, uint32_t n, const char* const* names, uint32_t num_names)
{
    return guard([&]() {
        std::vector<std::string> nm;
        for (uint32_t k = 0; names && k < num_names; ++k) nm.emplace_back(names[k]);
        ((rt::Scene*)s)->SetTriangleObjects(std::vector<uint32_t>(ids, ids + n), std::move(nm));
        return 0; }, 1);
}
uint32_t rth_scene_num_objects(void* s) { return (uint32_t)((rt::Scene*)s)->GetObjectNames().size(); }
const char* rth_scene_object_name(void* s, uint32_t i) { return ((rt::Scene*)s)->GetObjectNames()[i].c_str(); }
uint32_t rth_scene_num_triangle_objects(void* s) { return (uint32_t)((rt::Scene*)s)->GetTriangleObjects().size(); }
const void* rth_scene_triangle_objects(void* s) { return ((rt::Scene*)s)->GetTriangleObjects().data(); }
// SetTriangleSkin / GetTriangleSkin: three influences per triangle, the caller's triangle order in, the BVH's out (after Finalize)
int rth_scene_set_triangle_skin(void* s, const rt_skin_influence* per_corner, uint32_t num_triangles)
{
    return guard([&]() { ((rt::Scene*)s)->SetTriangleSkin(std::vector<rt_skin_influence>(per_corner, per_corner + (size_t)num_triangles * 3)); return 0; }, 1);
}
uint32_t rth_scene_num_triangle_skin(void* s) { return (uint32_t)((rt::Scene*)s)->GetTriangleSkin().size(); }
const void* rth_scene_triangle_skin(void* s) { return ((rt::Scene*)s)->GetTriangleSkin().data(); }

void rth_scene_destroy(void* s) { delete (rt::Scene*)s; }
void rth_scene_add_directional_light(void* s, float dx, float dy, float dz, float r, float g, float b)
{
    ((rt::Scene*)s)->AddDirectionalLight(rt::float3(dx, dy, dz), rt::float3(r, g, b));
}
void rth_scene_add_point_light(void* s, float x, float y, float z, float r, float g, float b)
{
    ((rt::Scene*)s)->AddPointLight(rt::float3(x, y, z), rt::float3(r, g, b));
}
void rth_scene_set_env_path(void* s, const char* path) { ((rt::Scene*)s)->SetEnvironmentPath(path); }
int rth_scene_set_env_image(void* s, const float* rgba, uint32_t w, uint32_t h)
{
    rt::Image img;
    img.width = w; img.height = h;
    img.data.resize((size_t)w * h * 4);
    memcpy(img.data.data(), rgba, (size_t)w * h * 16);
    ((rt::Scene*)s)->SetEnvironmentImage(std::move(img));
    return 0;
}
int rth_scene_finalize(void* s) { return guard([&]() { ((rt::Scene*)s)->Finalize(); return 0; }, 1); }

uint32_t rth_scene_num_triangles(void* s) { return (uint32_t)((rt::Scene*)s)->GetTriangles().size(); }
const void* rth_scene_triangles(void* s) { return ((rt::Scene*)s)->GetTriangles().data(); }
uint32_t rth_scene_num_materials(void* s) { return (uint32_t)((rt::Scene*)s)->GetMaterials().size(); }
const void* rth_scene_materials(void* s) { return ((rt::Scene*)s)->GetMaterials().data(); }
uint32_t rth_scene_num_textures(void* s) { return (uint32_t)((rt::Scene*)s)->GetTextures().size(); }
const void* rth_scene_textures(void* s) { return ((rt::Scene*)s)->GetTextures().data(); }
uint32_t rth_scene_num_texture_data(void* s) { return (uint32_t)((rt::Scene*)s)->GetTextureData().size(); }
const void* rth_scene_texture_data(void* s) { return ((rt::Scene*)s)->GetTextureData().data(); }
uint32_t rth_scene_num_lights(void* s) { return (uint32_t)((rt::Scene*)s)->GetLights().size(); }
const void* rth_scene_lights(void* s) { return ((rt::Scene*)s)->GetLights().data(); }
uint32_t rth_scene_num_emissive(void* s) { return (uint32_t)((rt::Scene*)s)->GetEmissiveIndices().size(); }
const void* rth_scene_emissive(void* s) { return ((rt::Scene*)s)->GetEmissiveIndices().data(); }
uint32_t rth_scene_env_width(void* s) { return ((rt::Scene*)s)->GetEnvImage().width; }
uint32_t rth_scene_env_height(void* s) { return ((rt::Scene*)s)->GetEnvImage().height; }
const void* rth_scene_env_data(void* s) { return ((rt::Scene*)s)->GetEnvImage().data.data(); }

// ---- Bvh ------------------------------------------------------------------
void* rth_bvh_build(void* scene)
{
    return guard([&]() -> void*
    {
        auto* b = new rt::Bvh();
        auto* s = (rt::Scene*)scene;
        if (s->HasPrebuiltBvh()) b->AdoptNodes(s->GetPrebuiltNodes());
        else b->BuildCPU(s->GetTriangles());
        return b;
    }, nullptr);
}
void rth_bvh_destroy(void* b) { delete (rt::Bvh*)b; }
int rth_scene_save_cache(void* scene, void* bvh, const char* path)
{
    return guard([&]() { ((rt::Scene*)scene)->SaveCache(path, ((rt::Bvh*)bvh)->GetNodes()); return 0; }, 1);
}
uint32_t rth_bvh_num_nodes(void* b) { return (uint32_t)((rt::Bvh*)b)->GetNodes().size(); }
const void* rth_bvh_nodes(void* b) { return ((rt::Bvh*)b)->GetNodes().data(); }

// ---- loaders / camera -------------------------------------------------------
static rt::Image g_img;
int rth_load_hdr(const char* path, uint32_t* w, uint32_t* h)
{
    g_img = rt::Image();
    if (!rt::LoadHDR(path, g_img)) return 1;
    *w = g_img.width; *h = g_img.height;
    return 0;
}
int rth_load_jpeg(const char* path, uint32_t* w, uint32_t* h)
{
    g_img = rt::Image();
    if (!rt::LoadJPEG(path, g_img)) return 1;
    *w = g_img.width; *h = g_img.height;
    return 0;
}
int rth_load_tga(const char* path, uint32_t* w, uint32_t* h)
{
    g_img = rt::Image();
    if (!rt::LoadTGA(path, g_img)) return 1;
    *w = g_img.width; *h = g_img.height;
    return 0;
}
int rth_load_png(const char* path, uint32_t* w, uint32_t* h)
{
    g_img = rt::Image();
    if (!rt::LoadPNG(path, g_img)) return 1;
    *w = g_img.width; *h = g_img.height;
    return 0;
}
const void* rth_loaded_image_data() { return g_img.data.data(); }
void rth_default_camera(uint32_t w, uint32_t h, rt_camera* out) { *out = rt::DefaultCamera(w, h); }
void rth_make_camera(float px, float py, float pz, float yaw, float pitch, float fov, float aspect, float aperture,
    float focus, rt_camera* out)
{
    *out = rt::MakeCamera(rt::float3(px, py, pz), yaw, pitch, fov, aspect, aperture, focus);
}

// ---- Render (needs a GPU) ---------------------------------------------------
void* rth_render_create(uint32_t w, uint32_t h, void* scene, int device, uint32_t tile_rank, uint32_t tile_count,
    uint32_t band_height)
{
    return guard([&]() -> void*
    {
        rt::TileDesc t; t.rank = tile_rank; t.count = tile_count; t.band_height = band_height;
        return new rt::Render(w, h, *(rt::Scene*)scene, device, t);
    }, nullptr);
}
// ... with context options set before the upload: options = n_options x {option, value}
void* rth_render_create_with_options(uint32_t w, uint32_t h, void* scene, int device, uint32_t tile_rank, uint32_t tile_count,
    uint32_t band_height, const uint32_t* options, uint32_t n_options)
{
    return guard([&]() -> void*
    {
        rt::TileDesc t; t.rank = tile_rank; t.count = tile_count; t.band_height = band_height;
        std::vector<std::pair<int, std::uint32_t>> opts;
        for (uint32_t i = 0; i < n_options; ++i) opts.emplace_back((int)options[2 * i], options[2 * i + 1]);
        return new rt::Render(w, h, *(rt::Scene*)scene, device, t, opts);
    }, nullptr);
}
void rth_render_destroy(void* r) { delete (rt::Render*)r; }
int rth_render_set_camera(void* r, const rt_camera* cam) { return guard([&]() { ((rt::Render*)r)->SetCamera(*cam); return 0; }, 1); }
int rth_render_set_max_bounces(void* r, uint32_t b) { return guard([&]() { ((rt::Render*)r)->GetIntegrator().SetMaxBounces(b); return 0; }, 1); }
int rth_render_enable_white_furnace(void* r, int e) { return guard([&]() { ((rt::Render*)r)->GetIntegrator().EnableWhiteFurnace(e != 0); return 0; }, 1); }
int rth_render_set_sampler(void* r, int blue_noise)
{
    return guard([&]() { ((rt::Render*)r)->GetIntegrator().SetSamplerType(blue_noise ? rt::Integrator::SamplerType::kBlueNoise : rt::Integrator::SamplerType::kRandom); return 0; }, 1);
}
int rth_render_set_blue_noise_path(void* r, const char* path) { ((rt::Render*)r)->GetIntegrator().SetBlueNoiseTablePath(path); return 0; }
int rth_render_enable_denoiser(void* r, int e) { return guard([&]() { ((rt::Render*)r)->GetIntegrator().EnableDenoiser(e != 0); return 0; }, 1); }
int rth_render_set_aov(void* r, int aov) { return guard([&]() { ((rt::Render*)r)->GetIntegrator().SetAOV((rt::Integrator::AOV)aov); return 0; }, 1); }
int rth_render_resolve(void* r, float* out)
{
    return guard([&]()
    {
        auto const& v = ((rt::Render*)r)->GetIntegrator().ResolveNow();
        memcpy(out, v.data(), v.size() * sizeof(float));
        return 0;
    }, 1);
}
// desc NULL = off
int rth_render_set_spatial_filter(void* r, const rt_filter_desc* desc)
{
    return guard([&]() { ((rt::Render*)r)->GetIntegrator().SetSpatialFilter(desc); return 0; }, 1);
}
// desc NULL = off
int rth_render_set_temporal_filter(void* r, const rt_temporal_filter_desc* desc)
{
    return guard([&]() { ((rt::Render*)r)->GetIntegrator().SetTemporalFilter(desc); return 0; }, 1);
}
int rth_render_set_resolve_every_frame(void* r, int e) { ((rt::Render*)r)->GetIntegrator().SetResolveEveryFrame(e != 0); return 0; }
int rth_render_frame(void* r) { return guard([&]() { ((rt::Render*)r)->RenderFrame(); return 0; }, 1); }
int rth_render_samples(void* r, uint32_t n) { return guard([&]() { ((rt::Render*)r)->RenderSamples(n); return 0; }, 1); }
int rth_render_reserve_samples(void* r, uint32_t n)
{
    return guard([&]() { return (int)((rt::Render*)r)->GetIntegrator().ReserveSamples(n); }, -1);
}
int rth_render_finish(void* r) { return guard([&]() { ((rt::Render*)r)->GetContext().Finish(); return 0; }, 1); }
uint32_t rth_render_local_rows(void* r) { return ((rt::Render*)r)->GetIntegrator().GetLocalRows(); }
void rth_render_setup_seconds(void* r, double* out4) { const double* s = ((rt::Render*)r)->GetSetupSeconds(); for (int i = 0; i < 4; ++i) out4[i] = s[i]; }
uint32_t rth_render_global_row(void* r, uint32_t row) { return ((rt::Render*)r)->GetIntegrator().GetGlobalRow(row); }
uint32_t rth_render_sample_count(void* r) { return ((rt::Render*)r)->GetIntegrator().GetSampleCount(); }
int rth_render_read_radiance(void* r, float* out)
{
    return guard([&]()
    {
        std::vector<float> v = ((rt::Render*)r)->GetIntegrator().ReadRadianceSum();
        memcpy(out, v.data(), v.size() * sizeof(float));
        return 0;
    }, 1);
}
int rth_render_read_resolved(void* r, float* out)
{
    auto const& v = ((rt::Render*)r)->GetIntegrator().GetResolvedImage();
    memcpy(out, v.data(), v.size() * sizeof(float));
    return 0;
}
int rth_render_stats(void* r, rt_stats* out) { return guard([&]() { *out = ((rt::Render*)r)->GetIntegrator().GetStats(); return 0; }, 1); }
uint32_t rth_render_num_nodes(void* r) { return (uint32_t)((rt::Render*)r)->GetAccelerationStructure().GetNodes().size(); }
const void* rth_render_nodes(void* r) { return ((rt::Render*)r)->GetAccelerationStructure().GetNodes().data(); }
void* rth_render_frame_handle(void* r) { return ((rt::Render*)r)->GetIntegrator().GetFrame(); }
void* rth_render_ctx_handle(void* r) { return ((rt::Render*)r)->GetContext().Get(); }
int rth_render_set_refittable(void* r, int on) { return guard([&]() { ((rt::Render*)r)->SetRefittable(on != 0); return 0; }, 1); }
int rth_render_set_refit_motion(void* r, int on) { return guard([&]() { ((rt::Render*)r)->SetRefitMotion(on != 0); return 0; }, 1); }
int rth_render_refit(void* r, const void* triangles, uint32_t count) { return guard([&]() { ((rt::Render*)r)->RefitGeometry((const rt::Triangle*)triangles, count); return 0; }, 1); }
int rth_render_set_objects(void* r, const uint32_t* object_of_triangle, uint32_t num_triangles, uint32_t num_objects)
{
    return guard([&]() { ((rt::Render*)r)->SetObjects(object_of_triangle, num_triangles, num_objects); return 0; }, 1);
}
int rth_render_pose(void* r, const float* matrices3x4, uint32_t num_objects) { return guard([&]() { ((rt::Render*)r)->PoseObjects(matrices3x4, num_objects); return 0; }, 1); }
int rth_render_set_skin(void* r, const rt_skin_influence* per_corner, uint32_t num_triangles, uint32_t num_bones)
{
    return guard([&]() { ((rt::Render*)r)->SetSkin(per_corner, num_triangles, num_bones); return 0; }, 1);
}
int rth_render_skin(void* r, const float* matrices3x4, uint32_t num_bones) { return guard([&]() { ((rt::Render*)r)->SkinBones(matrices3x4, num_bones); return 0; }, 1); }
int rth_render_set_morph(void* r, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t num_targets, uint32_t num_triangles)
{
    return guard([&]() { ((rt::Render*)r)->SetMorph(deltas, target_offsets, num_targets, num_triangles); return 0; }, 1);
}
int rth_render_morph(void* r, const float* weights, uint32_t num_targets) { return guard([&]() { ((rt::Render*)r)->MorphTargets(weights, num_targets); return 0; }, 1); }
int rth_render_morph_skin(void* r, const float* weights, uint32_t num_targets, const float* matrices3x4, uint32_t num_bones)
{
    return guard([&]() { ((rt::Render*)r)->MorphAndSkin(weights, num_targets, matrices3x4, num_bones); return 0; }, 1);
}
int rth_render_pick(void* r, uint32_t x, uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface) { return guard([&]() { ((rt::Render*)r)->Pick(x, y, ray, hit, surface); return 0; }, 1); }
// HIPPathTraceIntegrator::Pick itself: the FRAME's camera (what the last RenderFrame / RenderSamples handed over), where rth_render_pick uses the Render's
int rth_render_integrator_pick(void* r, uint32_t x, uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface)
{
    return guard([&]() { ((rt::Render*)r)->GetIntegrator().Pick(x, y, ray, hit, surface); return 0; }, 1);
}
int rth_render_trace(void* r, const rt_ray* rays, uint32_t n, int any_hit, rt_hit* hits, uint32_t* occluded, rt_surface* surfaces)
{
    return guard([&]() { ((rt::Render*)r)->TraceRays(rays, n, any_hit != 0, hits, occluded, surfaces); return 0; }, 1);
}
int rth_render_trace_all(void* r, const rt_ray* rays, uint32_t n, uint32_t max_hits, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    return guard([&]() { ((rt::Render*)r)->TraceAllHits(rays, n, max_hits, out, hits, surfaces); return 0; }, 1);
}
int rth_render_pick_all(void* r, uint32_t x, uint32_t y, uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces)
{
    return guard([&]() { ((rt::Render*)r)->PickAll(x, y, max_hits, ray, out, hits, surfaces); return 0; }, 1);
}
int rth_render_bake(void* r, const void* points, uint32_t n, const rt_bake_desc* desc, rt_bake_result* out)
{
    return guard([&]() { if (!desc) throw rt::HIPException("rth_render_bake: desc is NULL"); ((rt::Render*)r)->BakeOcclusion(points, n, *desc, out); return 0; }, 1);
}
int rth_render_occlusion_image(void* r, const rt_bake_desc* desc, float* out)
{
    return guard([&]() { if (!desc) throw rt::HIPException("rth_render_occlusion_image: desc is NULL"); ((rt::Render*)r)->OcclusionImage(*desc, out); return 0; }, 1);
}
int rth_render_atlas(void* r, const rt_atlas_desc* desc, const float* uv, rt_texel* texels, rt_atlas_stats* stats)
{
    return guard([&]() { if (!desc) throw rt::HIPException("rth_render_atlas: desc is NULL"); ((rt::Render*)r)->AtlasCover(*desc, uv, texels, stats); return 0; }, 1);
}
int rth_render_occlusion_atlas(void* r, const rt_atlas_desc* atlas, const float* uv, const rt_bake_desc* desc, float* out, rt_atlas_stats* stats)
{
    return guard([&]() { if (!atlas || !desc) throw rt::HIPException("rth_render_occlusion_atlas: desc is NULL"); ((rt::Render*)r)->OcclusionAtlas(*atlas, uv, *desc, out, stats); return 0; }, 1);
}
int rth_render_bake_light(void* r, const void* points, uint32_t n, const rt_light_bake_desc* desc, rt_light_bake_result* out)
{
    return guard([&]() { if (!desc) throw rt::HIPException("rth_render_bake_light: desc is NULL"); ((rt::Render*)r)->BakeLight(points, n, *desc, out); return 0; }, 1);
}
int rth_render_irradiance_image(void* r, const rt_light_bake_desc* desc, float* out)
{
    return guard([&]() { if (!desc) throw rt::HIPException("rth_render_irradiance_image: desc is NULL"); ((rt::Render*)r)->IrradianceImage(*desc, out); return 0; }, 1);
}
int rth_render_irradiance_atlas(void* r, const rt_atlas_desc* atlas, const float* uv, const rt_light_bake_desc* desc, float* out, rt_atlas_stats* stats)
{
    return guard([&]() { if (!atlas || !desc) throw rt::HIPException("rth_render_irradiance_atlas: desc is NULL"); ((rt::Render*)r)->IrradianceAtlas(*atlas, uv, *desc, out, stats); return 0; }, 1);
}
int rth_render_nearest(void* r, const rt_point* points, uint32_t n, rt_nearest* out, rt_surface* surfaces)
{
    return guard([&]() { ((rt::Render*)r)->Nearest(points, n, out, surfaces); return 0; }, 1);
}
int rth_render_within(void* r, const rt_point* points, uint32_t n, uint32_t max_near, uint32_t options, rt_point_hits* out, rt_nearest* near, rt_surface* surfaces)
{
    return guard([&]() { ((rt::Render*)r)->Within(points, n, max_near, options, out, near, surfaces); return 0; }, 1);
}
int rth_render_cross(void* r, const rt_probe* probes, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    return guard([&]() { ((rt::Render*)r)->Cross(probes, n, max_list, options, out, members); return 0; }, 1);
}
int rth_render_self_cross(void* r, uint32_t first, uint32_t n, uint32_t max_list, uint32_t options, rt_probe_hits* out, rt_cross_member* members)
{
    return guard([&]() { ((rt::Render*)r)->SelfCross(first, n, max_list, options, out, members); return 0; }, 1);
}
int rth_render_separation(void* r, const rt_probe* probes, uint32_t n, float max_distance, rt_separation* out)
{
    return guard([&]() { ((rt::Render*)r)->Separation(probes, n, max_distance, out); return 0; }, 1);
}
int rth_render_clearance(void* r, uint32_t first, uint32_t n, float max_distance, rt_separation* out)
{
    return guard([&]() { ((rt::Render*)r)->Clearance(first, n, max_distance, out); return 0; }, 1);
}
int rth_render_overlap(void* r, const rt_region* regions, uint32_t n, uint32_t max_list, rt_region_hits* out, rt_region_member* members)
{
    return guard([&]() { ((rt::Render*)r)->Overlap(regions, n, max_list, out, members); return 0; }, 1);
}
int rth_render_select(void* r, const rt_region* regions, uint32_t n, uint32_t* touching, uint32_t* inside, uint32_t* object_touching, uint32_t* object_inside)
{
    return guard([&]() { ((rt::Render*)r)->Select(regions, n, touching, inside, object_touching, object_inside); return 0; }, 1);
}
int rth_render_pick_rect(void* r, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far, rt_region* region, uint32_t* touching, uint32_t* inside,
    uint32_t* object_touching, uint32_t* object_inside)
{
    return guard([&]() { ((rt::Render*)r)->PickRect(x0, y0, x1, y1, t_near, t_far, region, touching, inside, object_touching, object_inside); return 0; }, 1);
}
// HIPPathTraceIntegrator::PickRect itself: the FRAME's camera, as rth_render_integrator_pick
int rth_render_integrator_pick_rect(void* r, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far, rt_region* region, uint32_t* touching,
    uint32_t* inside)
{
    return guard([&]() { ((rt::Render*)r)->GetIntegrator().PickRect(x0, y0, x1, y1, t_near, t_far, region, touching, inside, nullptr, nullptr); return 0; }, 1);
}
int rth_render_upload_gpu_data(void* r) { return guard([&]() { ((rt::Render*)r)->UploadGPUData(); return 0; }, 1); }

} // extern "C"
