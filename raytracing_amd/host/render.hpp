// render.hpp -- headless frame orchestration: owns the HIP context, the BVH,
// the integrator and the camera (reference: src/render.{hpp,cpp}, minus the
// window, GL framebuffer and ImGui).  RenderFrame() = one sample per pixel.
#pragma once
#include <utility>
#include <memory>
#include <vector>
#include "bvh.hpp"
#include "hip_pt_integrator.hpp"
#include "scene.hpp"

namespace rt
{
// The reference's start-up camera (src/utils/camera_controller.cpp:30-41,77-80).
Camera DefaultCamera(std::uint32_t width, std::uint32_t height);
Camera MakeCamera(float3 position, float yaw, float pitch, float fov, float aspect, float aperture, float focus);

class Render
{
public:
    // context_options: (rt_ctx_option, value) pairs set on the context before the scene is uploaded -- e.g. a rank of a group that will take another
    // rank's folds (rt_scene_import_folds) uploads without a shadow tree and without an adaptation of its own: {{2, 0}, {4, 0}}
    Render(std::uint32_t width, std::uint32_t height, Scene& scene, int device_ordinal = 0, TileDesc tile = TileDesc(),
        std::vector<std::pair<int, std::uint32_t>> const& context_options = {});

    void RenderFrame();                          // render.cpp:172-204 without present/GUI
    void RenderSamples(std::uint32_t n);         // n samples through the fused fast path
    void SetCamera(Camera const& camera);
    HIPPathTraceIntegrator& GetIntegrator() { return *integrator_; }
    HIPContext& GetContext() { return *context_; }
    // Uploads the scene again (after an rt_ctx_set_option that changes the device-side layout: tools, A/B runs)
    void UploadGPUData() { integrator_->UploadGPUData(scene_, *acc_structure_); }
    // Moving geometry: SetRefittable(true) uploads the scene again with what a refit needs kept on the device; RefitGeometry takes the moved triangles (the
    // scene's count and BVH order: GetTriangles() of the finalised scene) and restarts the accumulation.  The host Scene object keeps the pose it was built for.
    void SetRefittable(bool on) { integrator_->SetRefittable(on); UploadGPUData(); }
    void RefitGeometry(Triangle const* triangles, std::size_t count) { integrator_->RefitGeometry(triangles, count); }
    // ... and SetRefitMotion(true) (after SetRefittable(true)) uploads it again with room for the pose each refit replaces: the temporal filter then follows
    // the moved surfaces across a RefitGeometry instead of dropping its history
    void SetRefitMotion(bool on) { integrator_->SetRefitMotion(on); UploadGPUData(); }
    // Posed objects, after SetRefittable(true): which object each triangle belongs to (the finalised scene's BVH order), then one 3x4
    // matrix per object and pose -- 12 floats per object instead of RefitGeometry's 160 bytes per triangle.  An upload drops the objects: set them again.
    void SetObjects(std::uint32_t const* object_of_triangle, std::size_t triangle_count, std::uint32_t object_count) { integrator_->SetObjects(object_of_triangle, triangle_count, object_count); }
    void PoseObjects(float const* matrices3x4, std::size_t object_count) { integrator_->PoseObjects(matrices3x4, object_count); }
    // Skinned triangles, after SetRefittable(true): four bones and weights per triangle corner (the finalised scene's BVH order:
    // Scene::GetTriangleSkin), then one 3x4 matrix per bone and frame -- 48 bytes per bone instead of RefitGeometry's 160 bytes per triangle.  An upload drops
    // the skin: set it again.
    void SetSkin(rt_skin_influence const* per_corner, std::size_t triangle_count, std::uint32_t bone_count) { integrator_->SetSkin(per_corner, triangle_count, bone_count); }
    void SkinBones(float const* matrices3x4, std::size_t bone_count) { integrator_->SkinBones(matrices3x4, bone_count); }
    // Morph targets, after SetRefittable(true): sparse targets over the finalised scene's BVH order, then one weight per target and
    // frame -- 4 bytes per target instead of RefitGeometry's 160 bytes per triangle -- alone or fused with the skin.  An upload drops the targets: set them again.
    void SetMorph(rt_morph_delta const* deltas, std::uint32_t const* target_offsets, std::uint32_t target_count, std::size_t triangle_count) { integrator_->SetMorph(deltas, target_offsets, target_count, triangle_count); }
    void MorphTargets(float const* weights, std::size_t target_count) { integrator_->MorphTargets(weights, target_count); }
    void MorphAndSkin(float const* weights, std::size_t target_count, float const* matrices3x4, std::size_t bone_count) { integrator_->MorphAndSkin(weights, target_count, matrices3x4, bone_count); }
    // Ray queries: what lies under pixel (x, y) of the Render's current camera -- also one set since the last frame, which the integrator
    // has not been given yet: the ray is made from it here and traced as a query, the frame (its camera and previous camera included) is not touched -- and the
    // caller's own rays against the scene as it is posed now
    void Pick(std::uint32_t x, std::uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface) { integrator_->PickThrough(camera_, x, y, ray, hit, surface); }
    void TraceRays(rt_ray const* rays, std::size_t count, bool any_hit, rt_hit* hits, std::uint32_t* occluded, rt_surface* surfaces) { integrator_->TraceRays(rays, count, any_hit, hits, occluded, surfaces); }
    // Occlusion bakes: ambient occlusion and bent normals at the caller's points, and the exact ambient occlusion image of the Render's
    // current camera (also one set since the last frame), width x height floats, 1 where the pixel-centre ray misses; the frame is not touched
    void BakeOcclusion(void const* points, std::size_t count, rt_bake_desc const& desc, rt_bake_result* out) { integrator_->BakeOcclusion(points, count, desc, out); }
    void OcclusionImage(rt_bake_desc const& desc, float* out) { integrator_->OcclusionImageThrough(camera_, desc, out); }
    // The UV atlas: the cover, the surfaces of its records, and the ambient occlusion baked into it -- out[y * width + x] = unoccluded /
    // samples of texel (x, y), NaN where no triangle covers it (after the gutter); stats may be nullptr.
    void AtlasCover(rt_atlas_desc const& desc, float const* uv, rt_texel* texels, rt_atlas_stats* stats) { integrator_->AtlasCover(desc, uv, texels, stats); }
    void AtlasSurfaces(rt_texel const* texels, std::size_t count, rt_surface* surfaces) { integrator_->AtlasSurfaces(texels, count, surfaces); }
    void OcclusionAtlas(rt_atlas_desc const& atlas, float const* uv, rt_bake_desc const& desc, float* out, rt_atlas_stats* stats);
    // Light bakes: the irradiance of the sky and of the scene's lights at the caller's points; the irradiance image of the Render's current
    // camera, width x height x 3 floats of sky + lights, zeros where the pixel-centre ray misses; and the lightmap -- out[(y * width + x) * 3 ..] = sky + lights
    // of texel (x, y), NaN where no triangle covers it (after the gutter); stats may be nullptr.  The frame is not touched.
    void BakeLight(void const* points, std::size_t count, rt_light_bake_desc const& desc, rt_light_bake_result* out) { integrator_->BakeLight(points, count, desc, out); }
    void IrradianceImage(rt_light_bake_desc const& desc, float* out) { integrator_->IrradianceImageThrough(camera_, desc, out); }
    void IrradianceAtlas(rt_atlas_desc const& atlas, float const* uv, rt_light_bake_desc const& desc, float* out, rt_atlas_stats* stats);
    // the nearest surface point to each of the caller's points; the frame is not touched
    void Nearest(rt_point const* points, std::size_t count, rt_nearest* out, rt_surface* surfaces) { integrator_->NearestPoints(points, count, out, surfaces); }
    // every triangle within max_distance of each of the caller's points, counted and the nearest max_near listed; the frame is not touched
    void Within(rt_point const* points, std::size_t count, std::uint32_t max_near, std::uint32_t options, rt_point_hits* out, rt_nearest* near, rt_surface* surfaces) { integrator_->PointsWithin(points, count, max_near, options, out, near, surfaces); }
    // every triangle a convex region touches or encloses: counted and the lowest ids listed per region (Overlap), a bit per region for every
    // triangle and object of at most 32 regions (Select), the pixel rectangle of the Render's current camera (PickRect); the frame is not touched
    // every scene triangle a caller's triangle crosses, with contact points, and the scene's self-crossings
    void Cross(rt_probe const* probes, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members) { integrator_->TrianglesCross(probes, count, max_list, options, out, members); }
    void SelfCross(std::uint32_t first, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members) { integrator_->SelfCross(first, count, max_list, options, out, members); }
    // the nearest scene triangle to a caller's triangle with the two closest points (Separation), and the same for every scene triangle against the triangles
    // of the OTHER objects (Clearance: out[i] is triangle i's record; after SetObjects)
    void Separation(rt_probe const* probes, std::size_t count, float max_distance, rt_separation* out) { integrator_->TrianglesSeparation(probes, count, max_distance, out); }
    void Clearance(std::uint32_t first, std::size_t count, float max_distance, rt_separation* out) { integrator_->SelfSeparation(first, count, max_distance, RT_SEPARATION_OTHER_OBJECTS, out); }
    void Overlap(rt_region const* regions, std::size_t count, std::uint32_t max_list, rt_region_hits* out, rt_region_member* members) { integrator_->RegionsOverlap(regions, count, max_list, out, members); }
    void Select(rt_region const* regions, std::uint32_t count, std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside) { integrator_->SelectRegions(regions, count, touching, inside, object_touching, object_inside); }
    void PickRect(std::uint32_t x0, std::uint32_t y0, std::uint32_t x1, std::uint32_t y1, float t_near, float t_far, rt_region* region, std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside) { integrator_->PickRectThrough(camera_, x0, y0, x1, y1, t_near, t_far, region, touching, inside, object_touching, object_inside); }
    // every surface a ray crosses, counted and the nearest max_hits sorted; PickAll: through the centre of a pixel of the Render's current camera
    void TraceAllHits(rt_ray const* rays, std::size_t count, std::uint32_t max_hits, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces) { integrator_->TraceAllHits(rays, count, max_hits, out, hits, surfaces); }
    void PickAll(std::uint32_t x, std::uint32_t y, std::uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces) { integrator_->PickAllThrough(camera_, x, y, max_hits, ray, out, hits, surfaces); }
    AccelerationStructure const& GetAccelerationStructure() const { return *acc_structure_; }
    std::uint32_t GetWidth() const { return width_; }
    std::uint32_t GetHeight() const { return height_; }
    // what the constructor spent, seconds: {Bvh::BuildCPU (or adopting a cached tree), Scene::Finalize, the integrator (frame buffers), UploadGPUData}
    double const* GetSetupSeconds() const { return setup_seconds_; }

private:
    Scene& scene_;
    std::uint32_t width_, height_;
    double setup_seconds_[4] = {0.0, 0.0, 0.0, 0.0};
    std::shared_ptr<HIPContext> context_;
    std::unique_ptr<AccelerationStructure> acc_structure_;
    std::unique_ptr<HIPPathTraceIntegrator> integrator_;
    Camera camera_;
    bool camera_changed_ = true;
};

// One image over several GPUs of this process (no reference counterpart: the reference drives
// devices_[0] only, src/gpu_wrappers/cl_context.cpp:89).  The scene and its BVH are built once and
// uploaded to every device; device i renders the interleaved row bands of tile i
// (rt_frame_desc) on its own host thread; GatherRadiance() is the one RCCL gather (rt_group_*).
class TiledRender
{
public:
    // devices[i] = the GPU of tile i.  All entries equal = every tile on ONE device, exchanged by device copies
    // (rt_group_create_local: RCCL refuses two ranks per GPU) -- the way to run the whole tiled path on a one-GPU box.
    TiledRender(std::uint32_t width, std::uint32_t height, Scene& scene, std::vector<int> const& devices,
        std::uint32_t band_height = 8);
    // The image rows tile `rank` of `count` owns: bands of band_height rows dealt round-robin (rt_frame_desc); no device needed.
    static std::vector<std::uint32_t> TileRows(std::uint32_t height, std::uint32_t rank, std::uint32_t count, std::uint32_t band_height = 8);
    int GetRcclRanks() const;                             // ncclCommCount of the group's communicator (0: local group)
    ~TiledRender();
    void SetCamera(Camera const& camera);
    void SetMaxBounces(std::uint32_t max_bounces);
    void EnableWhiteFurnace(bool enable);
    // The spatial filter needs the whole image (its stencil crosses the tiles' rows): any desc throws; nullptr (off) is accepted.
    void SetSpatialFilter(rt_filter_desc const* desc);
    // Likewise the temporal filter (its history would have to cross the tiles' rows): any desc throws; nullptr (off) is accepted.
    void SetTemporalFilter(rt_temporal_filter_desc const* desc);
    // Moving geometry, forwarded to every tile's context (the scene is replicated; folds imported from tile 0 refit like any other)
    void SetRefittable(bool on);
    void RefitGeometry(Triangle const* triangles, std::size_t count);
    // forwarded too (the option only: the filters stay refused on tiles)
    void SetRefitMotion(bool on);
    // posed objects, forwarded to every tile's context likewise (tiles work because the refit does)
    void SetObjects(std::uint32_t const* object_of_triangle, std::size_t triangle_count, std::uint32_t object_count);
    void PoseObjects(float const* matrices3x4, std::size_t object_count);
    // skinned triangles, likewise
    void SetSkin(rt_skin_influence const* per_corner, std::size_t triangle_count, std::uint32_t bone_count);
    void SkinBones(float const* matrices3x4, std::size_t bone_count);
    void RenderSamples(std::uint32_t n);               // every tile, concurrently; returns when all are enqueued and finished
    std::vector<float> GatherRadiance(int root = 0);      // height x width x RGBA running sums, image order
    rt_stats GetStats() const;                            // ray counters summed over the tiles
    std::size_t GetTileCount() const { return integrators_.size(); }
    std::vector<double> const& GetLastTileSeconds() const { return tile_seconds_; }
    // One fold adaptation per GROUP: tile 0 adapts (its first RenderSamples waits for it), the other tiles -- uploaded without a shadow tree or an adaptation
    // of their own -- take its records (rt_scene_export_folds / rt_scene_import_folds).  Called by the first RenderSamples; results do not depend on it.
    void ShareFolds();
    bool FoldsShared() const { return folds_shared_; }
    HIPContext& GetContext(std::size_t i) { return *contexts_[i]; }
    AccelerationStructure const& GetAccelerationStructure() const { return *acc_structure_; }

private:
    Scene& scene_;
    std::uint32_t width_, height_;
    std::unique_ptr<AccelerationStructure> acc_structure_;
    std::vector<std::unique_ptr<HIPContext>> contexts_;
    std::vector<std::unique_ptr<HIPPathTraceIntegrator>> integrators_;
    std::vector<double> tile_seconds_;
    bool folds_shared_ = false;
    rt_group* group_ = nullptr;
    Camera camera_;
    bool camera_changed_ = true;
};
} // namespace rt
