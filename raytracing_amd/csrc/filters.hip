// filters.hip -- the spatial and temporal filters' device code and their host restatements (filters_host.h): the guide pass's pixel-centre rays and
// the guide values from their closest hits, one launch per a-trous pass (spatial_filter.h), and one launch each for the temporal filter's accumulation,
// variance estimate and variance-guided passes (temporal_filter.h).  A translation unit of its own so that the hot path's code object (rt_hip.hip,
// codeobj.code_object_sha256) does not change.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <thread>
#include <vector>
#include "rt_hip.h"
#include "kernels_common.h"
#include "temporal_filter.h"
#include "filters_host.h"
#include "device_memory.h"

#include "material_kernels.h"     // ApplyTextures: the albedo guide

static_assert(filt::NO_HISTORY == TF_NO_HISTORY && filt::IDENTITY == TF_IDENTITY && filt::REPROJECT == TF_REPROJECT, "modes");

namespace
{
__global__ __launch_bounds__(256) void k_sf_guide_rays(uint32_t width, uint32_t height, rt_camera cam, float tan_half_fov, float4* __restrict__ o4,
    float4* __restrict__ d4)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t pixel_y = i / width, pixel_x = i - pixel_y * width;
    float d[3];
    sf_guide_dir(cam, tan_half_fov, width, height, pixel_x, pixel_y, d);
    o4[i] = make_float4(cam.position.x, cam.position.y, cam.position.z, RT_MAX_RENDER_DIST);
    d4[i] = make_float4(d[0], d[1], d[2], __uint_as_float(i));
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

// RT_CTX_OPT_REFIT_MOTION: the pose a refit is about to replace -- the first six float4 (three positions, three shading normals) of every 128-byte shading
// record, 96 bytes per triangle.  One thread per float4: a wave reads 96 of every 128 bytes it touches and writes whole lines; pure streaming, no LDS.
__global__ __launch_bounds__(256) void k_sf_snapshot_pose(const float4* __restrict__ tsh, uint32_t nt, float4* __restrict__ snap)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)nt * 6u) return;
    const size_t t = i / 6u;
    snap[i] = tsh[t * 8u + (i - t * 6u)];
}

// where each pixel's first hit was in the snapshot's pose (tf_guide_motion): one thread per pixel, a gather of 96 bytes; a pixel without a hit gets zeros
__global__ __launch_bounds__(256) void k_sf_guide_motion(const float4* __restrict__ snap, uint32_t nt, const float4* __restrict__ hits, uint32_t n,
    float4* __restrict__ prev_pos, float4* __restrict__ prev_n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 hit = hits[i];
    const uint32_t prim = __float_as_uint(hit.z);
    sf_f4 pos = {0.0f, 0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f, 0.0f};
    if (prim < nt)                                               // RT_INVALID_ID (a miss) is above every count
    {
        const float4* tp = snap + (size_t)prim * 6;
        const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2], q3 = tp[3], q4 = tp[4], q5 = tp[5];
        const sf_f4 rec[6] = {{q0.x, q0.y, q0.z, 0.0f}, {q1.x, q1.y, q1.z, 0.0f}, {q2.x, q2.y, q2.z, 0.0f},
                              {q3.x, q3.y, q3.z, 0.0f}, {q4.x, q4.y, q4.z, 0.0f}, {q5.x, q5.y, q5.z, 0.0f}};
        tf_guide_motion(rec, hit.x, hit.y, &pos, &nrm);
    }
    prev_pos[i] = make_float4(pos.x, pos.y, pos.z, pos.w);
    prev_n[i] = make_float4(nrm.x, nrm.y, nrm.z, nrm.w);
}

// the per-pixel kernels: one thread per pixel, 16 x 16 blocks; false for a thread outside the width x height image
__device__ inline bool pixel16(uint32_t width, uint32_t height, uint32_t& x, uint32_t& y)
{
    x = blockIdx.x * 16u + threadIdx.x;
    y = blockIdx.y * 16u + threadIdx.y;
    return x < width && y < height;
}

__global__ __launch_bounds__(256) void k_sf_pass(SfPass P)
{
    uint32_t x, y;
    if (pixel16(P.width, P.height, x, y)) P.out[y * P.width + x] = sf_filter_pixel(P, x, y);
}

__global__ __launch_bounds__(256) void k_tf_accumulate(TfAccum A)
{
    uint32_t x, y;
    if (pixel16(A.width, A.height, x, y)) tf_accumulate_pixel(A, x, y);
}

__global__ __launch_bounds__(256) void k_tf_variance(TfVar V)
{
    uint32_t x, y;
    if (pixel16(V.width, V.height, x, y)) V.out[y * V.width + x] = tf_variance_pixel(V, x, y);
}

__global__ __launch_bounds__(256) void k_tf_pass(TfPass P)
{
    uint32_t x, y;
    if (pixel16(P.width, P.height, x, y)) P.out[y * P.width + x] = tf_pass_pixel(P, x, y);
}

template <class T> hipError_t launch_pixels(hipStream_t stream, void (*kernel)(T), const T& arg, uint32_t width, uint32_t height)
{
    hipLaunchKernelGGL(kernel, dim3((width + 15u) / 16u, (height + 15u) / 16u), dim3(16, 16), 0, stream, arg);
    return hipGetLastError();
}

// pixel(x, y) for every pixel of a width x height image on the host: rows y = t, t + n_threads, ... on n_threads threads (at most 16)
template <class F> void host_pixels(uint32_t width, uint32_t height, F&& pixel)
{
    unsigned hw = std::thread::hardware_concurrency();
    const uint32_t n_threads = std::max(1u, std::min({hw ? hw : 1u, 16u, height}));
    auto rows = [&](uint32_t t) {
        for (uint32_t y = t; y < height; y += n_threads)
            for (uint32_t x = 0; x < width; ++x) pixel(x, y);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(rows, t);
    rows(0);
    for (auto& th : pool) th.join();
}

// n pixels of a caller's array (4 floats per pixel; any alignment, nullptr for zeros) as a 16-byte-aligned image
std::vector<float4> staged(const float* p, size_t n)
{
    std::vector<float4> v(n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (p) memcpy(v.data(), p, n * sizeof(float4));
    return v;
}

// everything but the images is the same host floats for the kernels and the host restatement

// pass i reads the previous pass's image (pass 0: col) and writes ping (even i) / pong (odd i), the last one `out`
std::vector<SfPass> spatial_plan(const filt::Spatial& s, const float4* col, const float4* alb, const float4* nz, float4* ping, float4* pong, float4* out)
{
    const rt_filter_desc& d = s.desc;
    std::vector<SfPass> passes;
    for (uint32_t i = 0; i < d.iterations; ++i)
    {
        const bool last = i + 1 == d.iterations;
        SfPass P = {};
        P.col = (const sf_f4*)(i == 0 ? col : ((i & 1u) ? ping : pong));
        P.alb = (const sf_f4*)alb; P.nz = (const sf_f4*)nz; P.src = (const sf_f4*)col;
        P.out = (sf_f4*)(last ? out : ((i & 1u) ? pong : ping));
        P.width = s.width; P.height = s.height; P.step = 1u << i;
        P.flags = (i == 0 ? SF_FIRST : 0u) | (last ? SF_LAST : 0u) | (s.divide ? SF_DIVIDE : 0u) | ((d.flags & RT_FILTER_DEMODULATE) ? SF_DEMOD : 0u) |
                  (s.tonemap && last ? SF_TONEMAP : 0u);
        P.spp = s.spp;
        P.inv_c = (1.0f / (d.sigma_color * d.sigma_color)) * (float)(1u << (2u * i));
        P.inv_n = 1.0f / d.sigma_normal;
        P.inv_z = 1.0f / d.sigma_depth;
        passes.push_back(P);
    }
    return passes;
}

struct TemporalPlan
{
    TfAccum A;
    TfVar V;
    std::vector<TfPass> passes;     // iterations of them, or one finish (step 0) for zero iterations
};

// the accumulation writes a, the variance b; pass i reads b (even i) / a (odd i) and writes the other, the last one `out`
TemporalPlan temporal_plan(const filt::Temporal& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz, const float4* hist_in,
    const float4* mom_in, float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out, const float4* prev_pos, const float4* prev_n)
{
    const rt_temporal_filter_desc& d = c.desc;
    const uint32_t demod = (d.flags & RT_FILTER_DEMODULATE) ? SF_DEMOD : 0u, divide = c.divide ? SF_DIVIDE : 0u;
    TemporalPlan p;
    p.A = {};
    p.A.col = (const sf_f4*)col; p.A.alb = (const sf_f4*)alb; p.A.nz = (const sf_f4*)nz; p.A.prev_nz = (const sf_f4*)prev_nz;
    p.A.hist = (const sf_f4*)hist_in; p.A.mom = (const sf_f4*)mom_in; p.A.out_col = (sf_f4*)a; p.A.out_mom = (sf_f4*)mom_out;
    p.A.cam = c.cam; p.A.prev = c.prev;
    p.A.tan_cam = rt_tanf(0.5f * c.cam.fov); p.A.tan_prev = rt_tanf(0.5f * c.prev.fov);
    p.A.width = c.width; p.A.height = c.height; p.A.mode = c.mode; p.A.flags = demod | divide; p.A.spp = c.spp;
    p.A.alpha_color = d.alpha_color; p.A.alpha_moments = d.alpha_moments;
    const bool motion = prev_pos && prev_n;
    p.A.prev_pos = motion ? (const sf_f4*)prev_pos : nullptr; p.A.prev_n = motion ? (const sf_f4*)prev_n : nullptr;
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
} // namespace

namespace filt
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

hipError_t snapshot_pose(hipStream_t stream, const float4* tris_sh, uint32_t nt, float4* snap)
{
    if (nt == 0) return hipSuccess;
    const size_t blocks = ((size_t)nt * 6u + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sf_snapshot_pose, dim3((uint32_t)blocks), dim3(256), 0, stream, tris_sh, nt, snap);
    return hipGetLastError();
}

hipError_t guide_motion(hipStream_t stream, const float4* snap, uint32_t nt, const float4* hits, uint32_t n, float4* prev_pos, float4* prev_n)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sf_guide_motion, dim3((n + 255u) / 256u), dim3(256), 0, stream, snap, nt, hits, n, prev_pos, prev_n);
    return hipGetLastError();
}

std::vector<float> pose_records(const rt_triangle* tris, uint32_t nt)
{
    std::vector<float> r((size_t)nt * 24, 0.0f);
    for (uint32_t t = 0; t < nt; ++t)
    {
        const rt_vertex* v[3] = {&tris[t].v1, &tris[t].v2, &tris[t].v3};
        float* q = r.data() + (size_t)t * 24;
        for (int k = 0; k < 3; ++k)
        {
            q[4 * k] = v[k]->position.x; q[4 * k + 1] = v[k]->position.y; q[4 * k + 2] = v[k]->position.z;
            q[12 + 4 * k] = v[k]->normal.x; q[12 + 4 * k + 1] = v[k]->normal.y; q[12 + 4 * k + 2] = v[k]->normal.z;
        }
    }
    return r;
}

void guide_motion_host(const float* records, uint32_t nt, const float* hits, uint32_t n, float* prev_pos, float* prev_n)
{
    const std::vector<float4> rec = staged(records, (size_t)nt * 6);
    for (uint32_t i = 0; i < n; ++i)
    {
        uint32_t prim;
        memcpy(&prim, hits + 4 * (size_t)i + 2, sizeof(prim));
        sf_f4 pos = {0.0f, 0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f, 0.0f};
        if (prim < nt) tf_guide_motion((const sf_f4*)rec.data() + (size_t)prim * 6, hits[4 * (size_t)i], hits[4 * (size_t)i + 1], &pos, &nrm);
        memcpy(prev_pos + 4 * (size_t)i, &pos, sizeof(pos));
        memcpy(prev_n + 4 * (size_t)i, &nrm, sizeof(nrm));
    }
}

hipError_t guide_motion_device(hipStream_t stream, const float* records, uint32_t nt, const float* hits, uint32_t n, float* prev_pos, float* prev_n)
{
    const size_t pb = (size_t)n * sizeof(float4);
    dev::Temps tmp(stream);
    float4* d[4] = {nullptr, nullptr, nullptr, nullptr};            // records (six pieces each), hits, prev_pos, prev_n
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = tmp.array(d[k], k == 0 ? (size_t)nt * 6 : (size_t)n) ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess && nt) e = hipMemcpyAsync(d[0], records, (size_t)nt * 96, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d[1], hits, pb, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = guide_motion(stream, d[0], nt, d[1], n, d[2], d[3]);
    if (e == hipSuccess) e = hipMemcpyAsync(prev_pos, d[2], pb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(prev_n, d[3], pb, hipMemcpyDeviceToHost, stream);
    const hipError_t es = hipStreamSynchronize(stream);
    return e == hipSuccess ? es : e;
}

hipError_t spatial(hipStream_t stream, const Spatial& s, const float4* col, const float4* alb, const float4* nz, float4* ping, float4* pong, float4* out)
{
    for (const SfPass& P : spatial_plan(s, col, alb, nz, ping, pong, out))
    {
        hipError_t e = launch_pixels(stream, k_sf_pass, P, s.width, s.height);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void spatial_host(const Spatial& s, const float* col, const float* alb, const float* nz, float* out)
{
    const size_t n = (size_t)s.width * s.height;
    std::vector<float4> c0 = staged(col, n), al = staged(alb, n), g = staged(nz, n), ping(n), pong(n), res(n);
    for (const SfPass& P : spatial_plan(s, c0.data(), al.data(), g.data(), ping.data(), pong.data(), res.data()))
        host_pixels(s.width, s.height, [&](uint32_t x, uint32_t y) { P.out[(size_t)y * s.width + x] = sf_filter_pixel(P, x, y); });
    memcpy(out, res.data(), n * sizeof(float4));
}

hipError_t temporal(hipStream_t stream, const Temporal& c, const float4* col, const float4* alb, const float4* nz, const float4* prev_nz,
    const float4* hist_in, const float4* mom_in, float4* hist_out, float4* mom_out, float4* a, float4* b, float4* out, const float4* prev_pos,
    const float4* prev_n)
{
    const TemporalPlan p = temporal_plan(c, col, alb, nz, prev_nz, hist_in, mom_in, hist_out, mom_out, a, b, out, prev_pos, prev_n);
    hipError_t e = launch_pixels(stream, k_tf_accumulate, p.A, c.width, c.height);
    if (e == hipSuccess && c.desc.iterations) e = launch_pixels(stream, k_tf_variance, p.V, c.width, c.height);
    for (size_t i = 0; i < p.passes.size() && e == hipSuccess; ++i) e = launch_pixels(stream, k_tf_pass, p.passes[i], c.width, c.height);
    return e;
}

void temporal_host(const Temporal& c, const float* col, const float* alb, const float* nz, const float* prev_nz, const float* hist_in,
    const float* mom_in, float* hist_out, float* mom_out, float* out, const float* prev_pos, const float* prev_n)
{
    const size_t n = (size_t)c.width * c.height;
    const bool motion = prev_pos && prev_n;
    std::vector<float4> c0 = staged(col, n), al = staged(alb, n), g = staged(nz, n), pg = staged(prev_nz, n), hi = staged(hist_in, n),
                        mi = staged(mom_in, n), ho(n), mo(n), a(n), b(n), res(n), pp = staged(prev_pos, motion ? n : 0), pn = staged(prev_n, motion ? n : 0);
    const TemporalPlan p = temporal_plan(c, c0.data(), al.data(), g.data(), pg.data(), hi.data(), mi.data(), ho.data(), mo.data(), a.data(), b.data(),
                                         res.data(), motion ? pp.data() : nullptr, motion ? pn.data() : nullptr);
    host_pixels(c.width, c.height, [&](uint32_t x, uint32_t y) { tf_accumulate_pixel(p.A, x, y); });
    if (c.desc.iterations)
        host_pixels(c.width, c.height, [&](uint32_t x, uint32_t y) { p.V.out[(size_t)y * c.width + x] = tf_variance_pixel(p.V, x, y); });
    for (const TfPass& P : p.passes)
        host_pixels(c.width, c.height, [&](uint32_t x, uint32_t y) { P.out[(size_t)y * c.width + x] = tf_pass_pixel(P, x, y); });
    memcpy(out, res.data(), n * sizeof(float4)); memcpy(hist_out, ho.data(), n * sizeof(float4)); memcpy(mom_out, mo.data(), n * sizeof(float4));
}
} // namespace filt
