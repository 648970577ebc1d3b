// pose.h -- the arithmetic of rt_scene_pose: one 3x4 matrix per object, applied to a triangle of the rest pose.  k_pose_triangles and the
// host restatement (rt_debug_pose with ctx == NULL) both call the functions below, in binary32 with -ffp-contract=off, so the two agree bit for bit.
//
// A matrix is row-major: m[0..3] is row x (three linear terms, then the translation), m[4..7] row y, m[8..11] row z.
//   position   x' = ((m0 x + m1 y) + m2 z) + m3, likewise y and z; the .w lane is copied
//   normal     n' = ((C0 nx + C1 ny) + C2 nz) s per row, C = the cofactor matrix of the 3x3 part, s = -1 if det < 0 else +1 (so a mirror keeps the normal on the
//              side the winding says); l = (n'x^2 + n'y^2) + n'z^2; n' / sqrtf(l) if l > 0 and finite, else n' as transformed; the .w lane is copied
//   texcoords, mtl_index, padding: copied
//   an object whose 12 floats are bit for bit the identity's: its triangles are copied, not transformed
// C, det and s are made ONCE per object on the host (make_object); the library uploads them beside the matrix.
#pragma once
#include <stdint.h>
#include <string.h>
#include <cmath>
#include "rt_types.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define POSE_HD __host__ __device__ inline
#else
#define POSE_HD inline
#endif

namespace pose
{
// what the kernel reads per object: 96 bytes, shared by neighbouring triangles (they come through the L1 path)
struct Object
{
    float m[12];        // the matrix as given
    float c[9];         // cofactors of the 3x3 part, row-major
    float s;            // -1 if det < 0, else +1
    uint32_t identity;  // 1: m is bit for bit the identity's -> copy
    uint32_t pad;
};
static_assert(sizeof(Object) == 96, "pose::Object");

// host only: each cofactor a b - c d in the order written here, det along the first row
inline Object make_object(const float* m)
{
    static const float ident[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    Object o;
    for (int k = 0; k < 12; ++k) o.m[k] = m[k];
    o.c[0] = m[5] * m[10] - m[6] * m[9]; o.c[1] = m[6] * m[8] - m[4] * m[10]; o.c[2] = m[4] * m[9] - m[5] * m[8];
    o.c[3] = m[2] * m[9] - m[1] * m[10]; o.c[4] = m[0] * m[10] - m[2] * m[8]; o.c[5] = m[1] * m[8] - m[0] * m[9];
    o.c[6] = m[1] * m[6] - m[2] * m[5];  o.c[7] = m[2] * m[4] - m[0] * m[6];  o.c[8] = m[0] * m[5] - m[1] * m[4];
    const float det = (m[0] * o.c[0] + m[1] * o.c[1]) + m[2] * o.c[2];
    o.s = det < 0.0f ? -1.0f : 1.0f;
    o.identity = memcmp(m, ident, sizeof(ident)) == 0 ? 1u : 0u;
    o.pad = 0u;
    return o;
}

POSE_HD rt_float3 pose_point(const Object& o, const rt_float3& p)
{
    rt_float3 r;
    r.x = ((o.m[0] * p.x + o.m[1] * p.y) + o.m[2] * p.z) + o.m[3];
    r.y = ((o.m[4] * p.x + o.m[5] * p.y) + o.m[6] * p.z) + o.m[7];
    r.z = ((o.m[8] * p.x + o.m[9] * p.y) + o.m[10] * p.z) + o.m[11];
    r.w = p.w;
    return r;
}

POSE_HD rt_float3 pose_normal(const Object& o, const rt_float3& n)
{
    rt_float3 r;
    r.x = ((o.c[0] * n.x + o.c[1] * n.y) + o.c[2] * n.z) * o.s;
    r.y = ((o.c[3] * n.x + o.c[4] * n.y) + o.c[5] * n.z) * o.s;
    r.z = ((o.c[6] * n.x + o.c[7] * n.y) + o.c[8] * n.z) * o.s;
    r.w = n.w;
    const float l = (r.x * r.x + r.y * r.y) + r.z * r.z;
    if (l > 0.0f && l <= 3.402823466e+38f)          // finite (a NaN fails l > 0)
    {
        const float d = sqrtf(l);
        r.x = r.x / d; r.y = r.y / d; r.z = r.z / d;
    }
    return r;
}

POSE_HD void pose_vertex(const Object& o, rt_vertex& v)
{
    v.position = pose_point(o, v.position);
    v.normal = pose_normal(o, v.normal);
}

// in place; texcoords, mtl_index and padding stay
POSE_HD void pose_triangle(const Object& o, rt_triangle& t)
{
    if (o.identity) return;
    pose_vertex(o, t.v1); pose_vertex(o, t.v2); pose_vertex(o, t.v3);
}
} // namespace pose
