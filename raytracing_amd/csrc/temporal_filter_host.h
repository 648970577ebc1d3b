// temporal_filter_host.h -- the interface of temporal_filter.hip: the temporal filter's stages on the device and their host restatement
// (rt_frame_filter_temporal, rt_debug_filter_temporal in rt_hip.hip).  A translation unit of its own, like spatial_filter.hip: the hot path's code
// object (rt_hip.hip) is neither rebuilt nor re-hashed by the filter.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include "rt_hip.h"

namespace tfilt
{
// how a call finds its history: none (every pixel misses), each pixel's own (the same camera and scene), reprojected from the previous camera
// (temporal_filter.h's TF_NO_HISTORY, TF_IDENTITY, TF_REPROJECT)
enum Mode : uint32_t { NO_HISTORY = 0, IDENTITY = 1, REPROJECT = 2 };
// what one call filters: the image, its camera and the previous call's, how the history is found (Mode), the settings, and whether col is a
// radiance sum to divide by spp (divide) and the output is tone-mapped
struct Call
{
    uint32_t width, height;
    rt_camera cam, prev;
    uint32_t mode;
    rt_temporal_filter_desc desc;
    int divide;
    float spp;
    int tonemap;
};
// every stage over a width x height image.  col: h; alb, nz: this call's guides (albedo; unit normal + depth); prev_nz: the previous call's;
// hist_in / mom_in: the previous history (colour rgb; mu1, mu2, L); hist_out / mom_out: the new one (hist_out may be hist_in: it is written after
// the accumulation has read it; mom_out may not be mom_in); a, b: two scratch images; out: the result.
hipError_t run(hipStream_t stream, const Call& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz, const float4* hist_in,
    const float4* mom_in, float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out);
// the same stages on the host, threads over rows; the same arithmetic bit for bit.  Every array holds 4 floats per pixel.
void host_run(const Call& c, const float* col, const float* alb, const float* nz, const float* prev_nz, const float* hist_in, const float* mom_in,
    float* hist_out, float* mom_out, float* out);
} // namespace tfilt
