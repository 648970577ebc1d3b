// spatial_filter.hip -- the spatial filter's device code and its host restatement (rt_frame_filter, rt_frame_read_guides, rt_debug_filter):
// the guide pass's pixel-centre rays, the guide values from their closest hits, and one launch per a-trous pass (spatial_filter.h).
// A translation unit of its own so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <thread>
#include <vector>
#include "rt_hip.h"
#include "kernels_common.h"
#include "spatial_filter.h"
#include "spatial_filter_host.h"

#include "material_kernels.h"     // ApplyTextures: the albedo guide

namespace
{
// raygen_ray (raygen_kernels.h) with both random pixel offsets 0.5 and no lens: the ray through the pixel centre from cam.position
__global__ __launch_bounds__(256) void k_sf_guide_rays(uint32_t width, uint32_t height, rt_camera cam, float tan_half_fov, float4* __restrict__ o4,
    float4* __restrict__ d4)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t pixel_y = i / width, pixel_x = i - pixel_y * width;
    float inv_width = 1.0f / (float)width;
    float inv_height = 1.0f / (float)height;
    float x = ((float)pixel_x + 0.5f) * inv_width;
    float y = ((float)pixel_y + 0.5f) * inv_height;
    float angle = tan_half_fov;
    x = (x * 2.0f - 1.0f) * angle * cam.aspect_ratio;
    y = (y * 2.0f - 1.0f) * angle;
    f3 front = F3(cam.front.x, cam.front.y, cam.front.z);
    f3 up = F3(cam.up.x, cam.up.y, cam.up.z);
    f3 right = cross3(front, up);
    f3 dir = normalize3(right * x + up * y + front);
    o4[i] = make_float4(cam.position.x, cam.position.y, cam.position.z, RT_MAX_RENDER_DIST);
    d4[i] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(i));
}

// k_aov's formulas (aov_kernels.h) for ray i = pixel i
__global__ __launch_bounds__(256) void k_sf_guide_values(DScene sc, const float4* __restrict__ o4, const float4* __restrict__ hits, uint32_t n,
    float4* __restrict__ alb, float4* __restrict__ nz)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 hit = hits[i];
    const uint32_t prim = __float_as_uint(hit.z);
    if (prim == RT_INVALID_ID)
    {
        alb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        nz[i] = make_float4(0.0f, 0.0f, 0.0f, RT_MAX_RENDER_DIST);
        return;
    }
    const float4 ro = o4[i];
    const float4* tp = sc.tris_sh + (size_t)prim * 8;
    float4 q0 = tp[0], q1 = tp[1], q2 = tp[2], q3 = tp[3], q4 = tp[4], q5 = tp[5], q6 = tp[6];
    f3 p1 = xyz(q0), p2 = xyz(q1), p3 = xyz(q2);
    f3 n1 = xyz(q3), n2 = xyz(q4), n3 = xyz(q5);
    float bu = hit.x, bv = hit.y;
    float w0 = 1.0f - bu - bv;
    f3 position = p1 * w0 + p2 * bu + p3 * bv;
    f2 texcoord;
    texcoord.x = q0.w * w0 + q2.w * bu + q4.w * bv;
    texcoord.y = q1.w * w0 + q3.w * bu + q5.w * bv;
    f3 normal = normalize3(n1 * w0 + n2 * bu + n3 * bv);
    Material material;
    ApplyTextures(sc, __float_as_uint(q6.x), material, texcoord);
    alb[i] = make_float4(material.diffuse_albedo.x, material.diffuse_albedo.y, material.diffuse_albedo.z, 0.0f);
    nz[i] = make_float4(normal.x, normal.y, normal.z, length3(F3(ro.x, ro.y, ro.z) - position));
}

// one a-trous pass: one thread per pixel, 16 x 16 blocks
__global__ __launch_bounds__(256) void k_sf_pass(SfPass P)
{
    const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
    if (x >= P.width || y >= P.height) return;
    P.out[y * P.width + x] = sf_filter_pixel(P, x, y);
}

// pass i of n: everything but the images (the same host floats for the kernel and the host restatement)
SfPass pass_setup(uint32_t width, uint32_t height, uint32_t i, uint32_t n, uint32_t flags, float sigma_color, float sigma_normal, float sigma_depth,
    int divide, float spp, int tonemap)
{
    SfPass P = {};
    P.width = width; P.height = height; P.step = 1u << i;
    P.flags = (i == 0 ? SF_FIRST : 0u) | (i + 1 == n ? SF_LAST : 0u) | (divide ? SF_DIVIDE : 0u) | ((flags & RT_FILTER_DEMODULATE) ? SF_DEMOD : 0u) |
              (tonemap && i + 1 == n ? SF_TONEMAP : 0u);
    P.spp = spp;
    P.inv_c = (1.0f / (sigma_color * sigma_color)) * (float)(1u << (2u * i));
    P.inv_n = 1.0f / sigma_normal;
    P.inv_z = 1.0f / sigma_depth;
    return P;
}
} // namespace

namespace sfilt
{
hipError_t guide_rays(hipStream_t stream, uint32_t width, uint32_t height, const rt_camera& cam, float tan_half_fov, float4* o4, float4* d4)
{
    const uint32_t n = width * height;
    hipLaunchKernelGGL(k_sf_guide_rays, dim3((n + 255u) / 256u), dim3(256), 0, stream, width, height, cam, tan_half_fov, o4, d4);
    return hipGetLastError();
}

hipError_t guide_values(hipStream_t stream, const DScene& sc, const float4* o4, const float4* hits, uint32_t n, float4* alb, float4* nz)
{
    hipLaunchKernelGGL(k_sf_guide_values, dim3((n + 255u) / 256u), dim3(256), 0, stream, sc, o4, hits, n, alb, nz);
    return hipGetLastError();
}

hipError_t passes(hipStream_t stream, uint32_t width, uint32_t height, const float4* col, const float4* alb, const float4* nz, uint32_t iterations,
    uint32_t flags, float sigma_color, float sigma_normal, float sigma_depth, int divide, float spp, int tonemap, float4* ping, float4* pong, float4* out)
{
    const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u);
    for (uint32_t i = 0; i < iterations; ++i)
    {
        SfPass P = pass_setup(width, height, i, iterations, flags, sigma_color, sigma_normal, sigma_depth, divide, spp, tonemap);
        P.col = (const sf_f4*)(i == 0 ? col : ((i & 1u) ? ping : pong));            // pass i writes ping (even i) / pong (odd i), the last one `out`
        P.alb = (const sf_f4*)alb; P.nz = (const sf_f4*)nz; P.src = (const sf_f4*)col;
        P.out = (sf_f4*)(i + 1 == iterations ? out : ((i & 1u) ? pong : ping));
        hipLaunchKernelGGL(k_sf_pass, grid, dim3(16, 16), 0, stream, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void host_passes(uint32_t width, uint32_t height, const float* col, const float* alb, const float* nz, uint32_t iterations, uint32_t flags,
    float sigma_color, float sigma_normal, float sigma_depth, float* out)
{
    const size_t n = (size_t)width * height;
    std::vector<sf_f4> c0(n), a(n), g(n), res(n), ping(n), pong(n);     // sf_f4 is 16-byte aligned: the caller's arrays need not be
    memcpy(c0.data(), col, n * sizeof(sf_f4)); memcpy(a.data(), alb, n * sizeof(sf_f4)); memcpy(g.data(), nz, n * sizeof(sf_f4));
    unsigned hw = std::thread::hardware_concurrency();
    const uint32_t n_threads = std::max(1u, std::min({hw ? hw : 1u, 16u, height}));
    for (uint32_t i = 0; i < iterations; ++i)
    {
        SfPass P = pass_setup(width, height, i, iterations, flags, sigma_color, sigma_normal, sigma_depth, 0, 1.0f, 0);
        P.col = i == 0 ? c0.data() : ((i & 1u) ? ping.data() : pong.data());
        P.alb = a.data(); P.nz = g.data(); P.src = c0.data();
        P.out = i + 1 == iterations ? res.data() : ((i & 1u) ? pong.data() : ping.data());
        auto rows = [&](uint32_t t) {
            for (uint32_t y = t; y < height; y += n_threads)
                for (uint32_t x = 0; x < width; ++x) P.out[(size_t)y * width + x] = sf_filter_pixel(P, x, y);
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(rows, t);
        rows(0);
        for (auto& th : pool) th.join();
    }
    memcpy(out, res.data(), n * sizeof(sf_f4));
}
} // namespace sfilt
