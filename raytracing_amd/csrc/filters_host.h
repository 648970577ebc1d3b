// filters_host.h -- the interface of filters.hip: the guide pass's ray generation and guide values, the spatial filter's a-trous passes and the
// temporal filter's stages on the device, and their host restatements (rt_frame_filter, rt_frame_read_guides, rt_debug_filter,
// rt_frame_filter_temporal, rt_debug_filter_temporal in frame_filters.cpp; the pose a refit replaces in scene_upload.cpp).  A translation unit of its own,
// like device_fold.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by the filters.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <vector>
#include "rt_hip.h"

struct DScene;

namespace filt
{
// one ray per pixel of a width x height image in k_raygen's o4 / d4 layout: the pixel-centre pinhole ray from cam.position (d4.w = the pixel's index)
hipError_t guide_rays(hipStream_t stream, uint32_t width, uint32_t height, const rt_camera& cam, float tan_half_fov, float4* o4, float4* d4);
// k_aov's first-hit values from the closest hits of those rays: alb = ApplyTextures' diffuse albedo (w 0), nz = (unit normal, depth);
// a miss gets k_aov_clear's values (0, 0, 0 / depth RT_MAX_RENDER_DIST)
hipError_t guide_values(hipStream_t stream, const DScene& sc, const float4* o4, const float4* hits, uint32_t n, float4* alb, float4* nz);

// what one spatial filter call filters: a width x height image, the settings (desc.iterations >= 1), and whether col is a radiance sum to
// divide by spp (divide) and the output is tone-mapped
struct Spatial
{
    uint32_t width, height;
    rt_filter_desc desc;
    int divide;
    float spp;
    int tonemap;
};
// the a-trous passes.  col: h; alb, nz: the guides (albedo; unit normal + depth); ping / pong: two scratch images; out: the result.
hipError_t spatial(hipStream_t stream, const Spatial& s, const float4* col, const float4* alb, const float4* nz, float4* ping, float4* pong, float4* out);
// the same passes on the host, threads over rows; the same arithmetic bit for bit.  Every array holds 4 floats per pixel.
void spatial_host(const Spatial& s, const float* col, const float* alb, const float* nz, float* out);

// how a temporal call finds its history: none (every pixel misses), each pixel's own (the same camera and scene), reprojected from the previous
// camera (temporal_filter.h's TF_NO_HISTORY, TF_IDENTITY, TF_REPROJECT)
enum Mode : uint32_t { NO_HISTORY = 0, IDENTITY = 1, REPROJECT = 2 };
// what one temporal call filters: the image, its camera and the previous call's, how the history is found (Mode), the settings, and whether col
// is a radiance sum to divide by spp (divide) and the output is tone-mapped
struct Temporal
{
    uint32_t width, height;
    rt_camera cam, prev;
    uint32_t mode;
    rt_temporal_filter_desc desc;
    int divide;
    float spp;
    int tonemap;
};
// every stage.  col: h; alb, nz: this call's guides; prev_nz: the previous call's; hist_in / mom_in: the previous history (colour rgb; mu1, mu2, L);
// hist_out / mom_out: the new one (hist_out may be hist_in: it is written after the accumulation has read it; mom_out may not be mom_in); a, b: two
// scratch images; out: the result.  prev_pos / prev_n (both or neither; only read under REPROJECT): where each first hit was, and its normal there, in
// the pose before the last refit (guide_motion) -- the accumulation follows moved geometry with them (temporal_filter.h, step 1).
hipError_t temporal(hipStream_t stream, const Temporal& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz,
    const float4* hist_in, const float4* mom_in, float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out, const float4* prev_pos = nullptr,
    const float4* prev_n = nullptr);
// the same stages on the host, threads over rows; the same arithmetic bit for bit.  Every array holds 4 floats per pixel.
void temporal_host(const Temporal& c, const float* col, const float* alb, const float* nz, const float* prev_nz, const float* hist_in,
    const float* mom_in, float* hist_out, float* mom_out, float* out, const float* prev_pos = nullptr, const float* prev_n = nullptr);

// RT_CTX_OPT_REFIT_MOTION.  A pose = 6 float4 per triangle (96 bytes): three positions, three shading normals, the xyz of the shading record's q0 .. q5.
// snapshot_pose copies the current one out of the nt 128-byte shading records tris_sh, before a refit overwrites them.
hipError_t snapshot_pose(hipStream_t stream, const float4* tris_sh, uint32_t nt, float4* snap);
// per pixel with a first hit (hits: u, v, primitive bits; a primitive >= nt = none): prev_pos = (the hit's position in the pose `snap`, 1), prev_n = (its
// unit normal there, 0); zeros without a hit
hipError_t guide_motion(hipStream_t stream, const float4* snap, uint32_t nt, const float4* hits, uint32_t n, float4* prev_pos, float4* prev_n);
// the same on caller arrays: a pose made from reference-layout triangles; the kernel with its own device buffers; the host restatement (bit for bit)
std::vector<float> pose_records(const rt_triangle* tris, uint32_t nt);
hipError_t guide_motion_device(hipStream_t stream, const float* records, uint32_t nt, const float* hits, uint32_t n, float* prev_pos, float* prev_n);
void guide_motion_host(const float* records, uint32_t nt, const float* hits, uint32_t n, float* prev_pos, float* prev_n);
} // namespace filt
