// skin.h -- the arithmetic of rt_scene_skin: linear blend skinning, four bones per triangle CORNER, applied to a triangle of the rest
// pose.  k_skin_triangles and the host restatement (rt_debug_skin with ctx == NULL) both call the functions below, in binary32 with -ffp-contract=off, so the
// two agree bit for bit.
//
// A palette is num_bones row-major 3x4 matrices in rt_scene_pose's layout (pose.h).  A corner's rt_skin_influence names four of them and four weights.
//   blend      B[k] = ((w0 M[b0][k] + w1 M[b1][k]) + w2 M[b2][k]) + w3 M[b3][k], k = 0..11: this order, no slot skipped (an unused slot is weight 0 on any
//              valid bone: it adds a zero).  The weights are used as given; nothing normalises them.
//   identity   the 12 words of B bit for bit the identity's: position and normal are copied
//   otherwise  position through pose::pose_point with B; cofactors, det along the first row and s from B in the operand order of pose::make_object
//              (make_object below restates it for the device); normal through pose::pose_normal
//   the .w lanes, texture coordinates, mtl_index and padding: copied
// What follows from that:
//   * with every bone the identity, any weights that blend to exactly the identity give the rest pose back byte for byte: (1,0,0,0) does, and so does
//     (0.5,0.5,0,0) (0.5 + 0.5 = 1 and 0 + 0 = +0 exactly); weights whose sum only rounds near 1 are applied like any other matrix
//   * weights that sum to 0 collapse a corner to the origin with a zero normal (l = 0 is not normalised): finite, so accepted
//   * a non-finite result is refused by the refit's own read-only validation with the scene untouched, as for a pose
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // uint2, __uint_as_float: the decode at the end
#endif
#include "pose.h"

namespace skin
{
// the first of a corner's four terms, then one more per slot: acc = w0 m0, then acc = acc + w m
POSE_HD void blend_first(const float* m, float w, float* B) { for (int k = 0; k < 12; ++k) B[k] = w * m[k]; }
POSE_HD void blend_add(const float* m, float w, float* B) { for (int k = 0; k < 12; ++k) B[k] = B[k] + w * m[k]; }

// B = ((w0 m0 + w1 m1) + w2 m2) + w3 m3
POSE_HD void blend(const float* m0, const float* m1, const float* m2, const float* m3, const float* w, float* B)
{
    blend_first(m0, w[0], B); blend_add(m1, w[1], B); blend_add(m2, w[2], B); blend_add(m3, w[3], B);
}

POSE_HD uint32_t word_of(float f) { uint32_t u; memcpy(&u, &f, sizeof(u)); return u; }

// the 12 words of B are the identity's (+0.0 and 1.0 only: a -0.0 is another word)
POSE_HD bool is_identity(const float* B)
{
    uint32_t differ = 0u;
    for (int k = 0; k < 12; ++k) differ |= word_of(B[k]) ^ (k % 5 == 0 ? 0x3F800000u : 0u);
    return differ == 0u;
}

// pose::make_object for host AND device: each cofactor a b - c d in that order, det along the first row
POSE_HD pose::Object make_object(const float* m)
{
    pose::Object o;
    for (int k = 0; k < 12; ++k) o.m[k] = m[k];
    o.c[0] = m[5] * m[10] - m[6] * m[9]; o.c[1] = m[6] * m[8] - m[4] * m[10]; o.c[2] = m[4] * m[9] - m[5] * m[8];
    o.c[3] = m[2] * m[9] - m[1] * m[10]; o.c[4] = m[0] * m[10] - m[2] * m[8]; o.c[5] = m[1] * m[8] - m[0] * m[9];
    o.c[6] = m[1] * m[6] - m[2] * m[5];  o.c[7] = m[2] * m[4] - m[0] * m[6];  o.c[8] = m[0] * m[5] - m[1] * m[4];
    const float det = (m[0] * o.c[0] + m[1] * o.c[1]) + m[2] * o.c[2];
    o.s = det < 0.0f ? -1.0f : 1.0f;
    o.identity = is_identity(m) ? 1u : 0u;
    o.pad = 0u;
    return o;
}

// one corner: m0..m3 = the matrices of its four slots (12 floats each, wherever they live), w = its four weights
POSE_HD void skin_vertex(const float* m0, const float* m1, const float* m2, const float* m3, const float* w, rt_vertex& v)
{
    float B[12];
    blend(m0, m1, m2, m3, w, B);
    if (is_identity(B)) return;
    const pose::Object o = make_object(B);
    pose::pose_vertex(o, v);
}

#if defined(__HIPCC__)
// The device's decode of the influences, for the two kernels that skin (k_skin_triangles, k_morph_skin_triangles; shared by inclusion):
// a triangle's 72 bytes are nine 8-byte words; one corner from its three: (bone 0 | bone 1 << 16, bone 2 | bone 3 << 16), (w0, w1), (w2, w3)
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
#endif
} // namespace skin
