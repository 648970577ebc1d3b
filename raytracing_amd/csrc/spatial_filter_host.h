// spatial_filter_host.h -- the interface of spatial_filter.hip: the guide pass's ray generation and guide values, the a-trous passes on the device,
// and their host restatement (rt_frame_filter, rt_frame_read_guides, rt_debug_filter in rt_hip.hip).  A translation unit of its own, like
// device_fold.hip: the hot path's code object (rt_hip.hip) is neither rebuilt nor re-hashed by the filter.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include "rt_types.h"

struct DScene;

namespace sfilt
{
// one ray per pixel of a width x height image in k_raygen's o4 / d4 layout: the pixel-centre pinhole ray from cam.position (d4.w = the pixel's index)
hipError_t guide_rays(hipStream_t stream, uint32_t width, uint32_t height, const rt_camera& cam, float tan_half_fov, float4* o4, float4* d4);
// k_aov's first-hit values from the closest hits of those rays: alb = ApplyTextures' diffuse albedo (w 0), nz = (unit normal, depth);
// a miss gets k_aov_clear's values (0, 0, 0 / depth RT_MAX_RENDER_DIST)
hipError_t guide_values(hipStream_t stream, const DScene& sc, const float4* o4, const float4* hits, uint32_t n, float4* alb, float4* nz);
// the a-trous passes over a width x height image.  col: the radiance sum (divided by spp when divide != 0) or an HDR image; ping / pong: two scratch
// images; out: the result (tone-mapped when tonemap != 0).  flags: RT_FILTER_DEMODULATE.  iterations >= 1.
hipError_t passes(hipStream_t stream, uint32_t width, uint32_t height, const float4* col, const float4* alb, const float4* nz, uint32_t iterations,
    uint32_t flags, float sigma_color, float sigma_normal, float sigma_depth, int divide, float spp, int tonemap, float4* ping, float4* pong, float4* out);
// the same passes on the host (HDR in, HDR out), threads over rows; the same arithmetic bit for bit
void host_passes(uint32_t width, uint32_t height, const float* col, const float* alb, const float* nz, uint32_t iterations, uint32_t flags,
    float sigma_color, float sigma_normal, float sigma_depth, float* out);
} // namespace sfilt
