// temporal_filter.hip -- the temporal filter's device code and its host restatement (rt_frame_filter_temporal, rt_debug_filter_temporal):
// one launch each for the accumulation, the variance estimate and every variance-guided pass (temporal_filter.h states them).
// A translation unit of its own, like spatial_filter.hip, so that the hot path's code object (rt_hip.hip, codeobj.code_object_sha256) does not change.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <thread>
#include <vector>
#include "rt_hip.h"
#include "temporal_filter.h"
#include "temporal_filter_host.h"

static_assert(tfilt::NO_HISTORY == TF_NO_HISTORY && tfilt::IDENTITY == TF_IDENTITY && tfilt::REPROJECT == TF_REPROJECT, "modes");

namespace
{
// one thread per pixel, 16 x 16 blocks (as k_sf_pass)
__global__ __launch_bounds__(256) void k_tf_accumulate(TfAccum A)
{
    const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    tf_accumulate_pixel(A, x, y);
}

__global__ __launch_bounds__(256) void k_tf_variance(TfVar V)
{
    const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
    if (x >= V.width || y >= V.height) return;
    V.out[y * V.width + x] = tf_variance_pixel(V, x, y);
}

__global__ __launch_bounds__(256) void k_tf_pass(TfPass P)
{
    const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
    if (x >= P.width || y >= P.height) return;
    P.out[y * P.width + x] = tf_pass_pixel(P, x, y);
}

// everything but the images, the same host floats for the kernels and the host restatement
struct Plan
{
    TfAccum A;
    TfVar V;
    std::vector<TfPass> passes;     // iterations of them, or one finish (step 0) for zero iterations
};

// stage images: the accumulation writes a, the variance b; pass i reads b (even i) / a (odd i) and writes the other, the last one `out`
Plan plan(const tfilt::Call& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz, const float4* hist_in, const float4* mom_in,
    float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out)
{
    const rt_temporal_filter_desc& d = c.desc;
    const uint32_t demod = (d.flags & RT_FILTER_DEMODULATE) ? SF_DEMOD : 0u, divide = c.divide ? SF_DIVIDE : 0u;
    Plan p;
    p.A = {};
    p.A.col = (const sf_f4*)col; p.A.alb = (const sf_f4*)alb; p.A.nz = (const sf_f4*)nz; p.A.prev_nz = (const sf_f4*)prev_nz;
    p.A.hist = (const sf_f4*)hist_in; p.A.mom = (const sf_f4*)mom_in; p.A.out_col = (sf_f4*)a; p.A.out_mom = (sf_f4*)mom_out;
    p.A.cam = c.cam; p.A.prev = c.prev;
    p.A.tan_cam = rt_tanf(0.5f * c.cam.fov); p.A.tan_prev = rt_tanf(0.5f * c.prev.fov);
    p.A.width = c.width; p.A.height = c.height; p.A.mode = c.mode; p.A.flags = demod | divide; p.A.spp = c.spp;
    p.A.alpha_color = d.alpha_color; p.A.alpha_moments = d.alpha_moments;
    const float inv_n = 1.0f / d.sigma_normal, inv_z = 1.0f / d.sigma_depth;
    p.V = {};
    p.V.acc = (const sf_f4*)a; p.V.mom = (const sf_f4*)mom_out; p.V.nz = (const sf_f4*)nz; p.V.out = (sf_f4*)b;
    p.V.width = c.width; p.V.height = c.height; p.V.inv_n = inv_n; p.V.inv_z = inv_z;
    const uint32_t n = d.iterations ? d.iterations : 1u;
    for (uint32_t i = 0; i < n; ++i)
    {
        TfPass P = {};
        P.col = (const sf_f4*)(d.iterations == 0 ? a : ((i & 1u) ? a : b));
        P.mom = (const sf_f4*)mom_out; P.alb = (const sf_f4*)alb; P.nz = (const sf_f4*)nz; P.src = (const sf_f4*)col;
        P.out = (sf_f4*)(i + 1 == n ? out : ((i & 1u) ? b : a));
        P.hist = i == 0 ? (sf_f4*)hist_out : nullptr;
        P.width = c.width; P.height = c.height;
        P.step = d.iterations ? 1u << i : 0u;
        P.flags = (i + 1 == n ? SF_LAST : 0u) | divide | demod | (c.tonemap ? SF_TONEMAP : 0u);
        P.spp = c.spp;
        P.sigma_l = d.sigma_luminance; P.inv_n = inv_n; P.inv_z = inv_z;
        p.passes.push_back(P);
    }
    return p;
}

// rows y = t, t + n_threads, ... of a width x height image on n_threads host threads
template <class F> void host_rows(uint32_t height, F&& row)
{
    unsigned hw = std::thread::hardware_concurrency();
    const uint32_t n_threads = std::max(1u, std::min({hw ? hw : 1u, 16u, height}));
    auto rows = [&](uint32_t t) { for (uint32_t y = t; y < height; y += n_threads) row(y); };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(rows, t);
    rows(0);
    for (auto& th : pool) th.join();
}
} // namespace

namespace tfilt
{
hipError_t run(hipStream_t stream, const Call& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz, const float4* hist_in,
    const float4* mom_in, float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out)
{
    const Plan p = plan(c, col, alb, nz, prev_nz, hist_in, mom_in, hist_out, mom_out, a, b, out);
    const dim3 grid((c.width + 15u) / 16u, (c.height + 15u) / 16u);
    hipLaunchKernelGGL(k_tf_accumulate, grid, dim3(16, 16), 0, stream, p.A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (c.desc.iterations)
    {
        hipLaunchKernelGGL(k_tf_variance, grid, dim3(16, 16), 0, stream, p.V);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (const TfPass& P : p.passes)
    {
        hipLaunchKernelGGL(k_tf_pass, grid, dim3(16, 16), 0, stream, P);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

void host_run(const Call& c, const float* col, const float* alb, const float* nz, const float* prev_nz, const float* hist_in, const float* mom_in,
    float* hist_out, float* mom_out, float* out)
{
    const size_t n = (size_t)c.width * c.height, bytes = n * sizeof(sf_f4);
    // sf_f4 is 16-byte aligned: the caller's arrays need not be
    std::vector<sf_f4> c0(n), al(n), g(n), pg(n), hi(n), mi(n), ho(n), mo(n), a(n), b(n), res(n);
    memcpy(c0.data(), col, bytes); memcpy(al.data(), alb, bytes); memcpy(g.data(), nz, bytes); memcpy(pg.data(), prev_nz, bytes);
    memcpy(hi.data(), hist_in, bytes); memcpy(mi.data(), mom_in, bytes);
    const Plan p = plan(c, (const float4*)c0.data(), (const float4*)al.data(), (const float4*)g.data(), (const float4*)pg.data(), (const float4*)hi.data(),
        (const float4*)mi.data(), (float4*)ho.data(), (float4*)mo.data(), (float4*)a.data(), (float4*)b.data(), (float4*)res.data());
    host_rows(c.height, [&](uint32_t y) { for (uint32_t x = 0; x < c.width; ++x) tf_accumulate_pixel(p.A, x, y); });
    if (c.desc.iterations)
        host_rows(c.height, [&](uint32_t y) { for (uint32_t x = 0; x < c.width; ++x) p.V.out[(size_t)y * c.width + x] = tf_variance_pixel(p.V, x, y); });
    for (const TfPass& P : p.passes)
        host_rows(c.height, [&](uint32_t y) { for (uint32_t x = 0; x < c.width; ++x) P.out[(size_t)y * c.width + x] = tf_pass_pixel(P, x, y); });
    memcpy(out, res.data(), bytes); memcpy(hist_out, ho.data(), bytes); memcpy(mom_out, mo.data(), bytes);
}
} // namespace tfilt
