/* query.h -- the surface record of a ray query (rt_scene_trace's `surfaces`, rt_frame_pick, rt_debug_query_surface), stated once for
 * the kernel (query.hip: k_query_surface) and the host restatement (rt_debug_query_surface(NULL, ...)).  binary32 throughout, -ffp-contract=off, correctly
 * rounded divide and square root on both sides, so the two agree bit for bit.
 *
 * Of a hit (bu, bv) on a triangle with corners p1 p2 p3, shading normals n1 n2 n3 and texture coordinates uv1 uv2 uv3, in this order:
 *   w0 = 1 - bu - bv
 *   position  = p1 w0 + p2 bu + p3 bv           (k_sf_guide_values' operand order, filters.hip: the sums left to right)
 *   texcoord  = uv1 w0 + uv2 bu + uv3 bv
 *   shading normal   = normalize3(n1 w0 + n2 bu + n3 bv)      (three divides by the length; a zero blend gives NaN, as the guide pass's normal does)
 *   geometric normal = normalize3(cross3(p2 - p1, p3 - p1)), zeros when its squared length is 0 or not finite
 *   flags = 1 (hit) | 2 when dot3(direction, geometric normal) > 0 (the ray meets the back face)
 * A miss (primitive_id = RT_INVALID_ID) is that id and zeros. */
#ifndef RT_QUERY_H
#define RT_QUERY_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"

#define QS_FLAG_HIT 1u
#define QS_FLAG_BACK_FACE 2u

/* what query_surface reads of a triangle: the shading record's fields, or an rt_triangle's (rt_debug_query_surface) */
struct QsTriangle
{
    float p1[3], p2[3], p3[3];
    float n1[3], n2[3], n3[3];
    float uv1[2], uv2[2], uv3[2];
    uint32_t mtl_index;
};

RTD_FN QsTriangle qs_triangle(const rt_triangle& t)
{
    QsTriangle q;
    q.p1[0] = t.v1.position.x; q.p1[1] = t.v1.position.y; q.p1[2] = t.v1.position.z;
    q.p2[0] = t.v2.position.x; q.p2[1] = t.v2.position.y; q.p2[2] = t.v2.position.z;
    q.p3[0] = t.v3.position.x; q.p3[1] = t.v3.position.y; q.p3[2] = t.v3.position.z;
    q.n1[0] = t.v1.normal.x; q.n1[1] = t.v1.normal.y; q.n1[2] = t.v1.normal.z;
    q.n2[0] = t.v2.normal.x; q.n2[1] = t.v2.normal.y; q.n2[2] = t.v2.normal.z;
    q.n3[0] = t.v3.normal.x; q.n3[1] = t.v3.normal.y; q.n3[2] = t.v3.normal.z;
    q.uv1[0] = t.v1.texcoord.x; q.uv1[1] = t.v1.texcoord.y;
    q.uv2[0] = t.v2.texcoord.x; q.uv2[1] = t.v2.texcoord.y;
    q.uv3[0] = t.v3.texcoord.x; q.uv3[1] = t.v3.texcoord.y;
    q.mtl_index = t.mtl_index;
    return q;
}

RTD_FN rt_surface qs_miss(void)
{
    rt_surface s;
    for (int k = 0; k < 3; ++k) { s.position[k] = 0.0f; s.geometric_normal[k] = 0.0f; s.shading_normal[k] = 0.0f; }
    s.texcoord[0] = 0.0f; s.texcoord[1] = 0.0f;
    s.primitive_id = RT_INVALID_ID; s.mtl_index = 0u; s.object = 0u; s.t = 0.0f; s.flags = 0u;
    return s;
}

/* the surface of hit (bu, bv, t) on `tri`, met by a ray of direction d; object = the triangle's entry of rt_scene_set_objects' table (RT_INVALID_ID: none set) */
RTD_FN rt_surface query_surface(const QsTriangle& tri, const float d[3], float bu, float bv, float t, uint32_t primitive_id, uint32_t object)
{
    rt_surface s;
    const float w0 = 1.0f - bu - bv;
    float n[3], g[3];
    for (int k = 0; k < 3; ++k)
    {
        s.position[k] = tri.p1[k] * w0 + tri.p2[k] * bu + tri.p3[k] * bv;
        n[k] = tri.n1[k] * w0 + tri.n2[k] * bu + tri.n3[k] * bv;
    }
    for (int k = 0; k < 2; ++k) s.texcoord[k] = tri.uv1[k] * w0 + tri.uv2[k] * bu + tri.uv3[k] * bv;
    const float ln = __builtin_sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; ++k) s.shading_normal[k] = n[k] / ln;
    const float ax = tri.p2[0] - tri.p1[0], ay = tri.p2[1] - tri.p1[1], az = tri.p2[2] - tri.p1[2];
    const float bx = tri.p3[0] - tri.p1[0], by = tri.p3[1] - tri.p1[1], bz = tri.p3[2] - tri.p1[2];
    g[0] = ay * bz - az * by; g[1] = az * bx - ax * bz; g[2] = ax * by - ay * bx;
    const float l2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    if (l2 > 0.0f && __builtin_isfinite(l2))
    {
        const float lg = __builtin_sqrtf(l2);
        for (int k = 0; k < 3; ++k) s.geometric_normal[k] = g[k] / lg;
    }
    else
        for (int k = 0; k < 3; ++k) s.geometric_normal[k] = 0.0f;
    const float facing = d[0] * s.geometric_normal[0] + d[1] * s.geometric_normal[1] + d[2] * s.geometric_normal[2];
    s.primitive_id = primitive_id;
    s.mtl_index = tri.mtl_index;
    s.object = object;
    s.t = t;
    s.flags = QS_FLAG_HIT | (facing > 0.0f ? QS_FLAG_BACK_FACE : 0u);
    return s;
}

#endif /* RT_QUERY_H */
