// hip_pt_integrator.hpp -- the MI355X backend of Integrator: the class that
// takes the place of CLPathTraceIntegrator (reference:
// src/integrator/cl_pt_integrator.{hpp,cpp}) and talks to the device only
// through the C-ABI of include/rt_hip.h.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "integrator.hpp"
#include "rt_hip.h"

namespace rt
{
// What CLException is to the OpenCL backend (src/utils/cl_exception.hpp:109-123).
class HIPException : public std::runtime_error
{
public:
    explicit HIPException(const std::string& what) : std::runtime_error(what) {}
};

// RAII owner of an rt_ctx (CLContext's role, src/gpu_wrappers/cl_context.hpp:37-65).
class HIPContext
{
public:
    explicit HIPContext(int device_ordinal = 0);
    ~HIPContext();
    HIPContext(const HIPContext&) = delete;
    HIPContext& operator=(const HIPContext&) = delete;
    rt_ctx* Get() const { return ctx_; }
    void Finish() const;
    std::string DeviceName() const;
    // Loads the blue-noise sampler tables (the data the reference compiles in through
    // src/utils/blue_noise_sampler.hpp) from a packed asset file and uploads them.
    void LoadBlueNoiseTables(const std::string& path);
    bool HasBlueNoiseTables() const { return has_blue_noise_; }

private:
    rt_ctx* ctx_ = nullptr;
    bool has_blue_noise_ = false;
};

struct TileDesc   // which interleaved row bands of the image this integrator renders
{
    std::uint32_t rank = 0, count = 1, band_height = 8;
};

class HIPPathTraceIntegrator : public Integrator
{
public:
    HIPPathTraceIntegrator(std::uint32_t width, std::uint32_t height, AccelerationStructure& acc_structure,
        HIPContext& context, TileDesc tile = TileDesc());
    ~HIPPathTraceIntegrator() override;

    void UploadGPUData(Scene const& scene, AccelerationStructure const& acc_structure) override;
    void SetCameraData(Camera const& camera) override;
    void SetSamplerType(SamplerType sampler_type) override;
    void SetAOV(AOV aov) override;
    void EnableDenoiser(bool enable) override;

    // Fast path: n x Integrate() without leaving the native side between stages.
    void IntegrateSamples(std::uint32_t n_samples);
    // Sizes the per-path device buffers for IntegrateSamples(n_samples) ahead of time; returns the
    // number of samples the device will trace together.
    std::uint32_t ReserveSamples(std::uint32_t n_samples);
    // Headless outputs (the reference writes a GL-shared image in ResolveRadiance).
    std::vector<float> const& GetResolvedImage() const;   // local_rows x width x RGBA; waits for the image of the last frame to arrive
    std::vector<float> ReadRadianceSum() const;
    std::vector<float> const& ResolveNow();      // runs the resolve stage and returns the image
    std::uint32_t GetSampleCount() const;
    std::uint32_t GetLocalRows() const;
    std::uint32_t GetGlobalRow(std::uint32_t local_row) const;
    rt_stats GetStats() const;
    void SetResolveEveryFrame(bool enable) { resolve_every_frame_ = enable; }
    // RT_OPT_FRAME_KERNEL: 255 (this class's default) = measured choice between the stage kernels and one k_frame launch per Integrate(); 0 / 1 = forced
    void SetFrameKernel(std::uint32_t mode);
    // RT_OPT_SAMPLES_AHEAD: 1 (this class's default) = while the camera stands still the backend traces the next samples ahead in batches and an
    // Integrate() whose sample is there only replays it (same radiance after every call); 0 = every Integrate() traces its own sample; k = batch size
    void SetSamplesAhead(std::uint32_t mode);
    // packed uint8 tables, see tools/make_blue_noise_asset.py (default: relative to the CWD like the env map)
    void SetBlueNoiseTablePath(std::string path) { blue_noise_path_ = std::move(path); }
    // The spatial filter (rt_frame_filter, the edge-avoiding a-trous wavelet filter): desc = its settings (copied; RT_FILTER_DESC_DEFAULT is a good
    // start), nullptr = off (the default).  While it is on, ResolveRadiance() and ResolveNow() produce the FILTERED image through rt_frame_filter --
    // synchronously, without the asynchronous present.  A tile of a larger image (TileDesc::count > 1) refuses: the filter needs the whole image.
    void SetSpatialFilter(rt_filter_desc const* desc);
    // The temporal filter (rt_frame_filter_temporal, SVGF): desc = its settings (copied; RT_TEMPORAL_FILTER_DESC_DEFAULT is a good start), nullptr =
    // off (the default).  While it is on, ResolveRadiance() and ResolveNow() produce the temporally filtered image, synchronously, and each of them
    // advances the frame's history by one call.  It excludes SetSpatialFilter and EnableDenoiser(true): turning one on while another is on throws.
    // A tile of a larger image refuses it.
    void SetTemporalFilter(rt_temporal_filter_desc const* desc);
    // Moving geometry (rt_scene_refit).  SetRefittable: RT_CTX_OPT_REFITTABLE on this integrator's context -- effective at the next
    // UploadGPUData.  RefitGeometry: the uploaded scene's triangles moved (same count, same BVH order): every tree is refitted on the device in milliseconds
    // where UploadGPUData takes a third of a second or more; requests a reset, since the accumulated samples show the old pose.
    void SetRefittable(bool on);
    void RefitGeometry(Triangle const* triangles, std::size_t count);
    // RT_CTX_OPT_REFIT_MOTION: every refit keeps the pose it replaces (96 bytes per triangle), and with SetTemporalFilter on the
    // next ResolveRadiance() after a RefitGeometry filters with the history followed across the move instead of dropped.  Effective at the next
    // UploadGPUData; throws unless SetRefittable(true) came first.  One pose deep: resolve once per refit.
    void SetRefitMotion(bool on);
    // Posed objects (rt_scene_set_objects / rt_scene_pose), after SetRefittable(true) and UploadGPUData.  SetObjects: every triangle's
    // object (the uploaded BVH order); the scene's current pose becomes the rest pose; dropped by the next UploadGPUData.  PoseObjects: one row-major 3x4 matrix
    // per object, 12 floats each, absolute (always applied to the rest pose); the triangles are written and refitted on the device; requests a reset.  Both throw
    // HIPException with the library's message on a refusal.
    void SetObjects(std::uint32_t const* object_of_triangle, std::size_t triangle_count, std::uint32_t object_count);
    void PoseObjects(float const* matrices3x4, std::size_t object_count);
    // Skinned triangles (rt_scene_set_skin / rt_scene_skin), after SetRefittable(true) and UploadGPUData.  SetSkin: four bones and weights
    // per triangle corner, 3 * triangle_count records in the uploaded BVH order (Scene::GetTriangleSkin); the scene's current pose becomes the rest pose; dropped
    // by the next UploadGPUData; independent of SetObjects.  SkinBones: one row-major 3x4 matrix per bone, absolute; the triangles are written and refitted on
    // the device; requests a reset.  Both throw HIPException with the library's message on a refusal.
    void SetSkin(rt_skin_influence const* per_corner, std::size_t triangle_count, std::uint32_t bone_count);
    void SkinBones(float const* matrices3x4, std::size_t bone_count);
    // Morph targets (rt_scene_set_morph / rt_scene_morph / rt_scene_morph_skin), after SetRefittable(true) and UploadGPUData.  SetMorph:
    // sparse targets, target t owning deltas[target_offsets[t] .. target_offsets[t + 1]), corners = 3 * triangle + c in the uploaded BVH order; the scene's current
    // pose becomes the morph's rest pose; dropped by the next UploadGPUData; independent of SetObjects and SetSkin.  MorphTargets: one weight per target, absolute;
    // the triangles are written and refitted on the device; requests a reset.  MorphAndSkin: the morph, then SetSkin's influences with this palette, in one
    // kernel, from the MORPH's rest pose.  All throw HIPException with the library's message on a refusal.
    void SetMorph(rt_morph_delta const* deltas, std::uint32_t const* target_offsets, std::uint32_t target_count, std::size_t triangle_count);
    void MorphTargets(float const* weights, std::size_t target_count);
    void MorphAndSkin(float const* weights, std::size_t target_count, float const* matrices3x4, std::size_t bone_count);
    // Ray queries (rt_scene_trace / rt_frame_pick): the caller's rays against the uploaded scene as it is posed now.  TraceRays: closest hits
    // (hits and / or surfaces, either may be null) or, any_hit, one 0 / 1 word per ray in occluded; a count of 2^32 or more is refused.  Pick: the ray through the
    // centre of pixel (x, y) of the frame's current camera, its hit and surface (any may be null).  PickThrough: the same for a camera the frame has not been given
    // (Render's pending one): the ray is made here with the guide pass's own function and traced as a query, so neither the frame's camera nor its previous
    // camera moves.  All throw HIPException with the library's message on a refusal; none requests a reset or touches the frame.
    void TraceRays(rt_ray const* rays, std::size_t count, bool any_hit, rt_hit* hits, std::uint32_t* occluded, rt_surface* surfaces);
    void Pick(std::uint32_t x, std::uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface);
    void PickThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, rt_ray* ray, rt_hit* hit, rt_surface* surface);
    // Occlusion bakes (rt_scene_bake).  BakeOcclusion: ambient occlusion and bent normals at the caller's points (eight floats each, or
    // rt_surface records with RT_BAKE_FROM_SURFACES in desc.flags); a count of 2^32 or more is refused.  OcclusionImageThrough: for every pixel of the frame's size
    // the pixel-centre ray of `camera` -- made as PickThrough makes it -- is traced into an rt_surface on the device and those are baked there (RT_BAKE_FROM_SURFACES);
    // out[y * width + x] = unoccluded / samples, 1 where nothing is walked (a miss; a hit without a usable shading normal).  Both throw HIPException with the
    // library's message on a refusal; neither requests a reset or touches the frame.
    void BakeOcclusion(void const* points, std::size_t count, rt_bake_desc const& desc, rt_bake_result* out);
    void OcclusionImageThrough(Camera const& camera, rt_bake_desc desc, float* out);
    // The UV atlas (rt_scene_atlas).  AtlasCover: per texel of desc's atlas the lowest triangle whose UVs cover its centre, where on it
    // and how many do (uv: six floats per triangle, a second UV set, or nullptr for the triangles' own; stats may be nullptr).  AtlasSurfaces: the rt_surface of
    // each record on the triangles as posed now.  BakeAtlas: the cover, its surfaces and their occlusion bake in one call on the device (desc.flags must be 0;
    // texels and stats may be nullptr); an uncovered texel's result is a skipped point's.
    void AtlasCover(rt_atlas_desc const& desc, float const* uv, rt_texel* texels, rt_atlas_stats* stats);
    void AtlasSurfaces(rt_texel const* texels, std::size_t count, rt_surface* surfaces);
    void BakeAtlas(rt_atlas_desc const& atlas, float const* uv, rt_bake_desc const& desc, rt_bake_result* out, rt_texel* texels, rt_atlas_stats* stats);
    // Light bakes (rt_scene_light_bake).  BakeLight: the irradiance of the sky and of the scene's analytic lights at the caller's points
    // (BakeOcclusion's records), direct terms only; a count of 2^32 or more is refused.  IrradianceImageThrough: OcclusionImageThrough's pixel-centre surfaces,
    // light-baked on the device; out[(y * width + x) * 3 ..] = sky + lights, zeros where nothing is walked.  BakeLightAtlas: the cover, its surfaces and their
    // light bake in one call on the device (desc.flags must be 0; texels and stats may be nullptr); an uncovered texel's result is a skipped point's.
    void BakeLight(void const* points, std::size_t count, rt_light_bake_desc const& desc, rt_light_bake_result* out);
    void IrradianceImageThrough(Camera const& camera, rt_light_bake_desc desc, float* out);
    void BakeLightAtlas(rt_atlas_desc const& atlas, float const* uv, rt_light_bake_desc const& desc, rt_light_bake_result* out, rt_texel* texels, rt_atlas_stats* stats);
    // Nearest surface points (rt_scene_nearest): for each of the caller's points the nearest triangle of the scene as it is posed now, where
    // on it and how far, optionally with the rt_surface there; a count of 2^32 or more is refused.  Throws HIPException with the library's message on a
    // refusal; requests no reset and does not touch the frame.
    void NearestPoints(rt_point const* points, std::size_t count, rt_nearest* out, rt_surface* surfaces);
    // Within (rt_scene_within): every triangle of the scene as it is posed now within max_distance of each point -- the counts in out, the
    // nearest max_near members in near and surfaces (max_near records per point; either may be null); options: RT_WITHIN_K_NEAREST.  Throws HIPException with
    // the library's message on a refusal; requests no reset and does not touch the frame.
    void PointsWithin(rt_point const* points, std::size_t count, std::uint32_t max_near, std::uint32_t options, rt_point_hits* out, rt_nearest* near, rt_surface* surfaces);
    // Overlap (rt_scene_overlap / rt_scene_select / rt_frame_pick_rect): RegionsOverlap -- per convex region (up to 8 half-spaces) the counts
    // of the triangles it touches and encloses in out and the touching ones with the lowest ids in members (max_list per region; may be null); SelectRegions --
    // at most 32 regions against every triangle, a bit per region in a word per triangle (touching, inside) and per object (after SetObjects; any may be null);
    // PickRect -- the region of the inclusive pixel rectangle of the frame's current camera, then one select with it (bit 0); PickRectThrough -- the same for a
    // camera the frame has not been given, as PickThrough.  All throw HIPException with the library's message on a refusal; none requests a reset or touches
    // the frame.
    void RegionsOverlap(rt_region const* regions, std::size_t count, std::uint32_t max_list, rt_region_hits* out, rt_region_member* members);
    void SelectRegions(rt_region const* regions, std::uint32_t count, std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside);
    void PickRect(std::uint32_t x0, std::uint32_t y0, std::uint32_t x1, std::uint32_t y1, float t_near, float t_far, rt_region* region, std::uint32_t* touching,
        std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside);
    void PickRectThrough(Camera const& camera, std::uint32_t x0, std::uint32_t y0, std::uint32_t x1, std::uint32_t y1, float t_near, float t_far, rt_region* region,
        std::uint32_t* touching, std::uint32_t* inside, std::uint32_t* object_touching, std::uint32_t* object_inside);
    // Cross (rt_scene_cross / rt_scene_cross_self): TrianglesCross -- per caller-supplied triangle the scene triangles it crosses, the counts
    // in out and the crossing ones with the lowest ids, their six tests' bits and two contact points in members (max_list per probe; may be null); SelfCross --
    // the same where probe i is scene triangle first + i, neighbours that share a corner skipped (RT_CROSS_OTHER_OBJECTS: pairs of one object too, after
    // SetObjects).  options: RT_CROSS_ANY, RT_CROSS_OTHER_OBJECTS.  Both throw HIPException with the library's message on a refusal; neither requests a reset or
    // touches the frame.
    void TrianglesCross(rt_probe const* probes, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members);
    void SelfCross(std::uint32_t first, std::size_t count, std::uint32_t max_list, std::uint32_t options, rt_probe_hits* out, rt_cross_member* members);
    // Separation (rt_scene_separation / rt_scene_separation_self): TrianglesSeparation -- per caller-supplied triangle the nearest scene
    // triangle within max_distance, the two closest points and their distance (0 and RT_SEPARATION_CROSSING where the two cross); SelfSeparation -- the same
    // where probe i is scene triangle first + i, neighbours that share a corner skipped (RT_SEPARATION_OTHER_OBJECTS: pairs of one object too, after
    // SetObjects).  Both throw HIPException with the library's message on a refusal; neither requests a reset or touches the frame.
    void TrianglesSeparation(rt_probe const* probes, std::size_t count, float max_distance, rt_separation* out);
    void SelfSeparation(std::uint32_t first, std::size_t count, float max_distance, std::uint32_t options, rt_separation* out);
    // All hits (rt_scene_trace_all / rt_frame_pick_all): every surface each ray crosses -- the counts in out, the nearest max_hits crossings
    // in hits and surfaces (max_hits records per ray; either may be null).  PickAll: the ray through the centre of pixel (x, y) of the frame's current camera;
    // PickAllThrough: the same for a camera the frame has not been given, as PickThrough.  All throw HIPException with the library's message on a refusal; none
    // requests a reset or touches the frame.
    void TraceAllHits(rt_ray const* rays, std::size_t count, std::uint32_t max_hits, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces);
    void PickAll(std::uint32_t x, std::uint32_t y, std::uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces);
    void PickAllThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, std::uint32_t max_hits, rt_ray* ray, rt_ray_hits* out, rt_hit* hits, rt_surface* surfaces);
    rt_frame* GetFrame() const { return frame_; }

protected:
    void CreateKernels() override;
    void Reset() override;
    void AdvanceSampleCount() override;
    void GenerateRays() override;
    void IntersectRays(std::uint32_t bounce) override;
    void ComputeAOVs() override;
    void ShadeMissedRays(std::uint32_t bounce) override;
    void ShadeSurfaceHits(std::uint32_t bounce) override;
    void IntersectShadowRays() override;
    void AccumulateDirectSamples() override;
    void ClearOutgoingRayCounter(std::uint32_t bounce) override;
    void ClearShadowRayCounter() override;
    void Denoise() override;
    void CopyHistoryBuffers() override;
    void ResolveRadiance() override;

private:
    void Check(int rc) const;
    void SyncOptions();
    // rt_frame_pick's ray for a camera the frame has not been given; throws (naming `who`) for a tile frame or a pixel outside the image
    rt_ray PickRayThrough(Camera const& camera, std::uint32_t x, std::uint32_t y, char const* who) const;

    HIPContext& context_;
    rt_frame* frame_ = nullptr;
    std::vector<float> resolved_;
    bool resolved_pinned_ = false;     // resolved_ is page-locked (rt_host_register)
    bool resolve_every_frame_ = true;
    bool filter_on_ = false;           // SetSpatialFilter
    rt_filter_desc filter_ = RT_FILTER_DESC_DEFAULT;
    bool temporal_on_ = false;         // SetTemporalFilter
    rt_temporal_filter_desc temporal_ = RT_TEMPORAL_FILTER_DESC_DEFAULT;
    std::uint32_t tile_count_ = 1;
    std::string blue_noise_path_ = "assets/blue_noise/heitz2019_256spp_256d.bin";
    bool refittable_ = false;     // SetRefittable's last value (SetRefitMotion needs it)
};
} // namespace rt
