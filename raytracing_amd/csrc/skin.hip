// skin.hip -- the scene's triangles skinned ON THE DEVICE from a palette of bone matrices (rt_scene_set_skin / rt_scene_skin).
//
// A deforming mesh is 48 bytes per bone and frame, not 160 bytes per triangle: the scene keeps its rest pose and every corner's four bones and weights on the
// device, k_skin_triangles writes the skinned triangles into a staging area in rt_triangle layout, and the refit (refit.hip) runs on that as on any other
// triangle array.
//
//   k_skin_triangles   one thread per triangle, 256 per block: rest + influences + palette -> staged (skin.h's arithmetic)
//
// The rest pose and the staging area are a moved::Stage.  k_skin_triangles streams 232 bytes in and 160 out per triangle.  The block's 256 triangles go through
// LDS as moved_tile.h describes.  So do its influences: 72 bytes per triangle, contiguous, 18 432 bytes for a full block, so every block starts 16-byte aligned;
// a tail block of n triangles holds 9 n 8-byte words, loaded as floor(9 n / 2) 16-byte pieces and, for an odd n, one 8-byte word -- nothing is read past the
// array and nothing is mis-aligned.  A thread reads its own 72 bytes back as nine 8-byte words (stride 9 words, odd: no bank conflict for 8-byte reads).
// A palette of at most LDS_BONES matrices (6 KB) is staged in LDS once per block and gathered from there; a larger one is gathered from global memory through
// the vector L1 / L2.  Both branches call the same skin.h function on the same values, so they agree bit for bit.  LDS: 40 960 + 18 432 + 6 144 = 65 536 bytes,
// two blocks per CU.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "skin.h"
#include "skin_host.h"
#include "moved_tile.h"
#include "device_memory.h"

namespace skin
{
static_assert(sizeof(rt_skin_influence) == 24 && 3 * sizeof(rt_skin_influence) == INFLUENCE_BYTES, "three 24-byte influences per triangle");
static_assert(256 * 160 + 256 * INFLUENCE_BYTES + LDS_BONES * MATRIX_BYTES <= 65536, "k_skin_triangles' LDS");

__global__ __launch_bounds__(256) void k_skin_triangles(const float4* __restrict__ rest, const uint2* __restrict__ influences, const float* __restrict__ palette,
    uint32_t nt, uint32_t n_bones, float4* __restrict__ out)
{
    __shared__ float4 tile[256 * 10];
    __shared__ uint4 infl[256 * 9 / 2];                            // 256 x nine 8-byte words
    __shared__ float4 bones[LDS_BONES * 3];
    const moved::Tile b = moved::block_tile(nt);
    moved::load_tile(b, rest, tile);
    const uint32_t words = b.n * 9u;                               // this block's influences in 8-byte words, from a 16-byte aligned address (first * 72)
    const uint2* const src = influences + (size_t)b.first * 9;
    uint2* const infl2 = reinterpret_cast<uint2*>(infl);
    for (uint32_t k = threadIdx.x; k < words / 2u; k += 256u) infl[k] = reinterpret_cast<const uint4*>(src)[k];
    if ((words & 1u) != 0u && threadIdx.x == 0u) infl2[words - 1u] = src[words - 1u];   // an odd tail's last word
    const bool staged = n_bones <= (uint32_t)LDS_BONES;            // the same for every block of a launch
    if (staged)
        for (uint32_t k = threadIdx.x; k < n_bones * 3u; k += 256u) bones[k] = reinterpret_cast<const float4*>(palette)[k];
    __syncthreads();
    if (threadIdx.x < b.n)
    {
        uint2 q[9];
        for (uint32_t j = 0; j < 9u; ++j) q[j] = infl2[threadIdx.x * 9u + j];
        rt_triangle& t = *reinterpret_cast<rt_triangle*>(&tile[threadIdx.x * 10u]);
        if (staged) skin_triangle(reinterpret_cast<const float*>(bones), n_bones, q, t);
        else skin_triangle(palette, n_bones, q, t);
    }
    __syncthreads();
    moved::store_tile(b, tile, out);
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
    st.stage.release(); dev::drop(st.influences); dev::drop(st.palette);
    if (st.host_palette) (void)hipHostFree(st.host_palette);
    st = State();
}

bool arm(hipStream_t stream, State& st, const float4* tris_sh, const rt_skin_influence* per_corner, uint32_t nt, uint32_t n_bones)
{
    release(st);
    st.n_bones = n_bones;
    st.bytes = (size_t)nt * BYTES_PER_TRIANGLE + (size_t)n_bones * MATRIX_BYTES;
    bool ok = st.stage.arm(stream, tris_sh, nt) && dev::get(st.influences, (size_t)nt * INFLUENCE_BYTES) && dev::get(st.palette, (size_t)n_bones * MATRIX_BYTES) &&
              hipHostMalloc((void**)&st.host_palette, (size_t)n_bones * MATRIX_BYTES) == hipSuccess &&
              hipMemcpyAsync(st.influences, per_corner, (size_t)nt * INFLUENCE_BYTES, hipMemcpyHostToDevice, stream) == hipSuccess;
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
    hipLaunchKernelGGL(k_skin_triangles, dim3(dev::blocks_for(st.stage.n_tris, 256u)), dim3(256), 0, stream, (const float4*)st.stage.rest, (const uint2*)st.influences,
        (const float*)st.palette, st.stage.n_tris, st.n_bones, (float4*)st.stage.staged);
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
