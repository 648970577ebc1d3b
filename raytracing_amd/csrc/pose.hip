// pose.hip -- the scene's objects posed ON THE DEVICE from one 3x4 matrix per object (rt_scene_set_objects / rt_scene_pose).
//
// A rigid or affine move of an object is 12 floats, not 160 bytes per triangle: the scene keeps its rest pose and every triangle's object on the device,
// k_pose_triangles writes the posed triangles into a staging area in rt_triangle layout, and the refit (refit.hip) runs on that as on any other triangle array.
//
//   k_pose_triangles   one thread per triangle, 256 per block: rest + object -> staged (pose.h's arithmetic)
//
// The rest pose and the staging area are a moved::Stage (moved.hip makes the rest pose, once per rt_scene_set_objects).  k_pose_triangles is a pure stream,
// 164 bytes read and 160 written per triangle: a block moves its 256 triangles (40 KB, contiguous) through LDS as moved_tile.h describes, and each thread
// transforms its own triangle in LDS in between (positions and normals; the other lanes are not touched).  An object's 96 bytes come through the vector L1:
// neighbouring triangles share an object.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <vector>
#include "pose.h"
#include "pose_host.h"
#include "moved_tile.h"
#include "device_memory.h"

namespace pose
{
__global__ __launch_bounds__(256) void k_pose_triangles(const float4* __restrict__ rest, const uint32_t* __restrict__ ids, const Object* __restrict__ objects,
    uint32_t nt, uint32_t n_objects, float4* __restrict__ out)
{
    __shared__ float4 tile[256 * 10];
    const moved::Tile b = moved::block_tile(nt);
    moved::load_tile(b, rest, tile);
    __syncthreads();
    if (threadIdx.x < b.n)
    {
        const uint32_t id = ids[b.first + threadIdx.x];
        if (id < n_objects)                                        // (rt_scene_set_objects has checked every id)
            pose_triangle(objects[id], *reinterpret_cast<rt_triangle*>(&tile[threadIdx.x * 10u]));
    }
    __syncthreads();
    moved::store_tile(b, tile, out);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------
bool ids_in_range(const uint32_t* ids, uint32_t nt, uint32_t n_objects)
{
    for (uint32_t i = 0; i < nt; ++i) if (ids[i] >= n_objects) return false;
    return true;
}

bool matrices_finite(const float* m, uint32_t n_objects)
{
    for (size_t k = 0; k < (size_t)n_objects * 12; ++k) if (!std::isfinite(m[k])) return false;
    return true;
}

static void make_objects(const float* m, uint32_t n_objects, Object* out)
{
    for (uint32_t k = 0; k < n_objects; ++k) out[k] = make_object(m + (size_t)k * 12);
}

void release(State& st)
{
    st.stage.release(); dev::drop(st.ids); dev::drop(st.objects);
    if (st.host_objects) (void)hipHostFree(st.host_objects);
    st = State();
}

bool arm(hipStream_t stream, State& st, const float4* tris_sh, const uint32_t* ids, uint32_t nt, uint32_t n_objects)
{
    release(st);
    st.n_objects = n_objects;
    st.bytes = (size_t)nt * BYTES_PER_TRIANGLE + (size_t)n_objects * sizeof(Object);
    bool ok = st.stage.arm(stream, tris_sh, nt) && dev::get(st.ids, (size_t)nt * ID_BYTES) && dev::get(st.objects, (size_t)n_objects * sizeof(Object)) &&
              hipHostMalloc(&st.host_objects, (size_t)n_objects * sizeof(Object)) == hipSuccess &&
              hipMemcpyAsync(st.ids, ids, (size_t)nt * ID_BYTES, hipMemcpyHostToDevice, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    if (!ok) { (void)hipGetLastError(); release(st); }
    return ok;
}

bool run(hipStream_t stream, State& st, const float* matrices3x4)
{
    make_objects(matrices3x4, st.n_objects, (Object*)st.host_objects);
    if (hipMemcpyAsync(st.objects, st.host_objects, (size_t)st.n_objects * sizeof(Object), hipMemcpyHostToDevice, stream) != hipSuccess) return false;
    hipLaunchKernelGGL(k_pose_triangles, dim3(dev::blocks_for(st.stage.n_tris, 256u)), dim3(256), 0, stream, (const float4*)st.stage.rest, (const uint32_t*)st.ids,
        (const Object*)st.objects, st.stage.n_tris, st.n_objects, (float4*)st.stage.staged);
    return dev::clean();
}

void debug_host(const rt_triangle* rest, const uint32_t* ids, uint32_t nt, const float* matrices3x4, uint32_t n_objects, rt_triangle* out)
{
    std::vector<Object> objects(n_objects);
    make_objects(matrices3x4, n_objects, objects.data());
    for (uint32_t i = 0; i < nt; ++i)
    {
        rt_triangle t = rest[i];
        pose_triangle(objects[ids[i]], t);
        out[i] = t;
    }
}

bool debug_device(hipStream_t stream, const rt_triangle* rest, const uint32_t* ids, uint32_t nt, const float* matrices3x4, uint32_t n_objects, rt_triangle* out)
{
    std::vector<Object> objects(n_objects);
    make_objects(matrices3x4, n_objects, objects.data());
    dev::Temps tmp(stream);
    void* const d_rest = tmp.get(rest, (size_t)nt * sizeof(rt_triangle));
    void* const d_ids = tmp.get(ids, (size_t)nt * 4);
    void* const d_objects = tmp.get(objects.data(), (size_t)n_objects * sizeof(Object));
    void* const d_out = tmp.get(nullptr, (size_t)nt * sizeof(rt_triangle));
    const bool ok = d_rest && d_ids && d_objects && d_out;
    if (ok)
        hipLaunchKernelGGL(k_pose_triangles, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, (const float4*)d_rest, (const uint32_t*)d_ids, (const Object*)d_objects, nt, n_objects, (float4*)d_out);
    return tmp.finish(ok && dev::clean(), out, d_out, (size_t)nt * sizeof(rt_triangle));
}
} // namespace pose
