// moved.hip -- moved.h's Stage and k_rest_pose: once per rt_scene_set_*, the 128-byte shading records back into rt_triangle layout, one thread per triangle
// (DESIGN.md section 7g).  -ffp-contract=off like every other unit (there is no arithmetic here).
#include <hip/hip_runtime.h>
#include "moved.h"
#include "device_memory.h"

namespace moved
{
static_assert(sizeof(rt_triangle) == REST_BYTES && sizeof(rt_triangle) == STAGED_BYTES, "the rest pose and the staging area are rt_triangle arrays");

// THE rest-pose rule: a triangle's shading record q[0..7] -> its ten rt_triangle pieces o[0..9].  It is the inverse of what k_refit_triangles (refit.hip)
// and k_relayout_triangles write -- positions in q[0..2].xyz, normals in q[3..5].xyz, the six texture coordinates in the .w lanes of q[0..5] in corner
// order, mtl_index in q[6].x -- and has to follow any change to that record.  The .w lanes of positions and normals, texcoord.z and the padding are zero.
__device__ inline void rest_pieces(const float4* __restrict__ q, float4* __restrict__ o)
{
    const float4 a = q[0], b = q[1], c = q[2], n1 = q[3], n2 = q[4], n3 = q[5], m = q[6];
    o[0] = make_float4(a.x, a.y, a.z, 0.0f); o[1] = make_float4(a.w, b.w, 0.0f, 0.0f);   o[2] = make_float4(n1.x, n1.y, n1.z, 0.0f);
    o[3] = make_float4(b.x, b.y, b.z, 0.0f); o[4] = make_float4(c.w, n1.w, 0.0f, 0.0f);  o[5] = make_float4(n2.x, n2.y, n2.z, 0.0f);
    o[6] = make_float4(c.x, c.y, c.z, 0.0f); o[7] = make_float4(n2.w, n3.w, 0.0f, 0.0f); o[8] = make_float4(n3.x, n3.y, n3.z, 0.0f);
    o[9] = make_float4(m.x, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void k_rest_pose(const float4* __restrict__ tsh, uint32_t nt, float4* __restrict__ rest)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nt) rest_pieces(tsh + (size_t)i * 8, rest + (size_t)i * 10);
}

void Stage::release() { dev::drop(rest); dev::drop(staged); n_tris = 0; }

bool Stage::arm(hipStream_t stream, const float4* tris_sh, uint32_t nt)
{
    release();
    if (dev::get(rest, (size_t)nt * REST_BYTES) && dev::get(staged, (size_t)nt * STAGED_BYTES))
    {
        hipLaunchKernelGGL(k_rest_pose, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, tris_sh, nt, (float4*)rest);
        if (dev::clean()) { n_tris = nt; return true; }
    }
    release();
    return false;
}
} // namespace moved
