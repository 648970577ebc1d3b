// skin.hip -- the scene's triangles skinned ON THE DEVICE from a palette of bone matrices (rt_scene_set_skin / rt_scene_skin).
//
// A deforming mesh is 48 bytes per bone and frame, not 160 bytes per triangle: the scene keeps its rest pose and every corner's four bones and weights on the
// device, k_skin_triangles writes the skinned triangles into a staging area in rt_triangle layout, and the refit (refit.hip) runs on that as on any other
// triangle array.
//
//   k_skin_rest        once per rt_scene_set_skin: the 128-byte shading records back into rt_triangle layout (the rest pose; k_pose_rest's rule)
//   k_skin_triangles   one thread per triangle, 256 per block: rest + influences + palette -> staged (skin.h's arithmetic)
//
// k_skin_triangles streams 232 bytes in and 160 out per triangle.  The block's 256 triangles (40 KB, contiguous) go through LDS in 16-byte pieces exactly as
// in k_pose_triangles.  So do its influences: 72 bytes per triangle, contiguous, 18 432 bytes for a full block, so every block's first byte is 16-byte aligned;
// a tail block of n triangles holds 9 n 8-byte words, loaded as floor(9 n / 2) 16-byte pieces and, for an odd n, one 8-byte word -- nothing is read past the
// array and nothing is mis-aligned.  A thread reads its own 72 bytes back as nine 8-byte words (stride 9 words, odd: no bank conflict for 8-byte reads).
// A palette of at most LDS_BONES matrices (6 KB) is staged in LDS once per block and gathered from there; a larger one is gathered from global memory through
// the vector L1 / L2.  Both branches call the same skin.h function on the same values, so they agree bit for bit.  LDS: 40 960 + 18 432 + 6 144 = 65 536 bytes,
// two blocks per CU.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "skin.h"
#include "skin_host.h"
#include "device_memory.h"

namespace skin
{
static_assert(sizeof(rt_triangle) == 10 * sizeof(float4), "rt_triangle = ten 16-byte pieces");
static_assert(sizeof(rt_skin_influence) == 24 && 3 * sizeof(rt_skin_influence) == INFLUENCE_BYTES, "three 24-byte influences per triangle");
static_assert(256 * 160 + 256 * INFLUENCE_BYTES + LDS_BONES * MATRIX_BYTES <= 65536, "k_skin_triangles' LDS");

__global__ __launch_bounds__(256) void k_skin_rest(const float4* __restrict__ tsh, uint32_t nt, float4* __restrict__ rest)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nt) return;
    const float4* q = tsh + (size_t)i * 8;
    const float4 a = q[0], b = q[1], c = q[2], n1 = q[3], n2 = q[4], n3 = q[5], m = q[6];
    float4* o = rest + (size_t)i * 10;
    o[0] = make_float4(a.x, a.y, a.z, 0.0f); o[1] = make_float4(a.w, b.w, 0.0f, 0.0f);   o[2] = make_float4(n1.x, n1.y, n1.z, 0.0f);
    o[3] = make_float4(b.x, b.y, b.z, 0.0f); o[4] = make_float4(c.w, n1.w, 0.0f, 0.0f);  o[5] = make_float4(n2.x, n2.y, n2.z, 0.0f);
    o[6] = make_float4(c.x, c.y, c.z, 0.0f); o[7] = make_float4(n2.w, n3.w, 0.0f, 0.0f); o[8] = make_float4(n3.x, n3.y, n3.z, 0.0f);
    o[9] = make_float4(m.x, 0.0f, 0.0f, 0.0f);
}

// one corner from its three 8-byte words: (bone 0 | bone 1 << 16, bone 2 | bone 3 << 16), (w0, w1), (w2, w3)
__device__ inline void skin_corner(const float* palette, uint32_t n_bones, uint2 bones, uint2 w01, uint2 w23, rt_vertex& v)
{
    const uint32_t b0 = bones.x & 0xFFFFu, b1 = bones.x >> 16, b2 = bones.y & 0xFFFFu, b3 = bones.y >> 16;
    if (b0 >= n_bones || b1 >= n_bones || b2 >= n_bones || b3 >= n_bones) return;       // (rt_scene_set_skin has checked every index)
    const float w[4] = {__uint_as_float(w01.x), __uint_as_float(w01.y), __uint_as_float(w23.x), __uint_as_float(w23.y)};
    skin_vertex(palette + b0 * 12u, palette + b1 * 12u, palette + b2 * 12u, palette + b3 * 12u, w, v);
}

__device__ inline void skin_triangle(const float* palette, uint32_t n_bones, const uint2* q, rt_triangle& t)
{
    skin_corner(palette, n_bones, q[0], q[1], q[2], t.v1);
    skin_corner(palette, n_bones, q[3], q[4], q[5], t.v2);
    skin_corner(palette, n_bones, q[6], q[7], q[8], t.v3);
}

__global__ __launch_bounds__(256) void k_skin_triangles(const float4* __restrict__ rest, const uint2* __restrict__ influences, const float* __restrict__ palette,
    uint32_t nt, uint32_t n_bones, float4* __restrict__ out)
{
    __shared__ float4 tile[256 * 10];
    __shared__ uint4 infl[256 * 9 / 2];                            // 256 x nine 8-byte words
    __shared__ float4 bones[LDS_BONES * 3];
    const uint32_t first = blockIdx.x * 256u;                      // < nt: the grid is ceil(nt / 256) blocks
    const uint32_t n = nt - first < 256u ? nt - first : 256u;      // this block's triangles
    const uint32_t pieces = n * 10u;
    const size_t base = (size_t)first * 10;
    for (uint32_t k = threadIdx.x; k < pieces; k += 256u) tile[k] = rest[base + k];
    const uint32_t words = n * 9u;                                 // this block's influences in 8-byte words, from a 16-byte aligned address (first * 72)
    const uint2* const src = influences + (size_t)first * 9;
    uint2* const infl2 = reinterpret_cast<uint2*>(infl);
    for (uint32_t k = threadIdx.x; k < words / 2u; k += 256u) infl[k] = reinterpret_cast<const uint4*>(src)[k];
    if ((words & 1u) != 0u && threadIdx.x == 0u) infl2[words - 1u] = src[words - 1u];   // an odd tail's last word
    const bool staged = n_bones <= (uint32_t)LDS_BONES;            // the same for every block of a launch
    if (staged)
        for (uint32_t k = threadIdx.x; k < n_bones * 3u; k += 256u) bones[k] = reinterpret_cast<const float4*>(palette)[k];
    __syncthreads();
    if (threadIdx.x < n)
    {
        uint2 q[9];
        for (uint32_t j = 0; j < 9u; ++j) q[j] = infl2[threadIdx.x * 9u + j];
        rt_triangle& t = *reinterpret_cast<rt_triangle*>(&tile[threadIdx.x * 10u]);
        if (staged) skin_triangle(reinterpret_cast<const float*>(bones), n_bones, q, t);
        else skin_triangle(palette, n_bones, q, t);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < pieces; k += 256u) out[base + k] = tile[k];
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------
int influences_fault(const rt_skin_influence* per_corner, uint32_t nt, uint32_t n_bones)
{
    for (size_t i = 0; i < (size_t)nt * 3; ++i)
        for (int k = 0; k < 4; ++k)
        {
            if (per_corner[i].bone[k] >= n_bones) return 1;
            if (!std::isfinite(per_corner[i].weight[k])) return 2;
        }
    return 0;
}

bool matrices_finite(const float* m, uint32_t n_bones)
{
    for (size_t k = 0; k < (size_t)n_bones * 12; ++k) if (!std::isfinite(m[k])) return false;
    return true;
}

void release(State& st)
{
    dev::drop(st.rest); dev::drop(st.influences); dev::drop(st.staged); dev::drop(st.palette);
    if (st.host_palette) (void)hipHostFree(st.host_palette);
    st = State();
}

bool arm(hipStream_t stream, State& st, const float4* tris_sh, const rt_skin_influence* per_corner, uint32_t nt, uint32_t n_bones)
{
    release(st);
    st.n_tris = nt; st.n_bones = n_bones;
    st.bytes = (size_t)nt * BYTES_PER_TRIANGLE + (size_t)n_bones * MATRIX_BYTES;
    bool ok = dev::get(st.rest, (size_t)nt * REST_BYTES) && dev::get(st.influences, (size_t)nt * INFLUENCE_BYTES) && dev::get(st.staged, (size_t)nt * STAGED_BYTES) &&
              dev::get(st.palette, (size_t)n_bones * MATRIX_BYTES) && hipHostMalloc((void**)&st.host_palette, (size_t)n_bones * MATRIX_BYTES) == hipSuccess &&
              hipMemcpyAsync(st.influences, per_corner, (size_t)nt * INFLUENCE_BYTES, hipMemcpyHostToDevice, stream) == hipSuccess;
    if (ok)
    {
        hipLaunchKernelGGL(k_skin_rest, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, tris_sh, nt, (float4*)st.rest);
        ok = dev::clean();
    }
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    if (!ok) { (void)hipGetLastError(); release(st); }
    return ok;
}

bool upload_palette(hipStream_t stream, State& st, const float* matrices3x4)
{
    memcpy(st.host_palette, matrices3x4, (size_t)st.n_bones * MATRIX_BYTES);
    return hipMemcpyAsync(st.palette, st.host_palette, (size_t)st.n_bones * MATRIX_BYTES, hipMemcpyHostToDevice, stream) == hipSuccess;
}

bool run(hipStream_t stream, State& st, const float* matrices3x4)
{
    if (!upload_palette(stream, st, matrices3x4)) return false;
    hipLaunchKernelGGL(k_skin_triangles, dim3(dev::blocks_for(st.n_tris, 256u)), dim3(256), 0, stream, (const float4*)st.rest, (const uint2*)st.influences,
        (const float*)st.palette, st.n_tris, st.n_bones, (float4*)st.staged);
    return dev::clean();
}

void debug_host(const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t nt, const float* matrices3x4, uint32_t n_bones, rt_triangle* out)
{
    (void)n_bones;
    for (uint32_t i = 0; i < nt; ++i)
    {
        rt_triangle t = rest[i];
        rt_vertex* const corners[3] = {&t.v1, &t.v2, &t.v3};
        for (int c = 0; c < 3; ++c)
        {
            const rt_skin_influence& f = per_corner[(size_t)i * 3 + c];
            skin_vertex(matrices3x4 + (size_t)f.bone[0] * 12, matrices3x4 + (size_t)f.bone[1] * 12, matrices3x4 + (size_t)f.bone[2] * 12,
                matrices3x4 + (size_t)f.bone[3] * 12, f.weight, *corners[c]);
        }
        out[i] = t;
    }
}

bool debug_device(hipStream_t stream, const rt_triangle* rest, const rt_skin_influence* per_corner, uint32_t nt, const float* matrices3x4, uint32_t n_bones, rt_triangle* out)
{
    dev::Temps tmp(stream);
    void* const d_rest = tmp.get(rest, (size_t)nt * sizeof(rt_triangle));
    void* const d_infl = tmp.get(per_corner, (size_t)nt * INFLUENCE_BYTES);
    void* const d_palette = tmp.get(matrices3x4, (size_t)n_bones * MATRIX_BYTES);
    void* const d_out = tmp.get(nullptr, (size_t)nt * sizeof(rt_triangle));
    const bool ok = d_rest && d_infl && d_palette && d_out;
    if (ok)
        hipLaunchKernelGGL(k_skin_triangles, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, (const float4*)d_rest, (const uint2*)d_infl, (const float*)d_palette, nt, n_bones, (float4*)d_out);
    return tmp.finish(ok && dev::clean(), out, d_out, (size_t)nt * sizeof(rt_triangle));
}
} // namespace skin
