/* region.h -- every triangle a caller's convex region touches or encloses (rt_scene_overlap / rt_scene_overlap_buffer / rt_scene_select / rt_frame_pick_rect /
 * rt_debug_overlap / rt_debug_overlap_walk / rt_debug_select / rt_debug_rect_region), stated once for the kernels (region.hip: k_region,
 * k_region_brute, k_select) and the host (rt_debug_overlap(NULL, ...), rt_debug_overlap_walk, rt_debug_select(NULL, ...)).  binary32 throughout,
 * -ffp-contract=off, so the device and the host agree bit for bit.
 *
 * A REGION is the intersection of 1 to RT_REGION_MAX_PLANES half-spaces, plane k = (nx, ny, nz, d); normals need not have unit length.
 *   s_k(x) = ((nx x0 + ny x1) + nz x2) + d          every product and every sum rounded once, in this order (np_dot3's order, then + d)
 *   x is OUTSIDE plane k exactly when s_k(x) > 0: a corner on the plane is inside, and a NaN s is not outside.
 * A region is SEARCHED when 1 <= num_planes <= 8 and its 4 * num_planes coefficients are finite; `reserved` is ignored.
 *
 * CLASSIFICATION of a triangle, on the shading record's three corners (k_nearest's operands).  out_k = how many corners are outside plane k.
 *   rejected   some out_k == 3
 *   inside     every out_k == 0               (exact for the rounded s)
 *   crossing   anything else
 *   touching = inside or crossing.
 * This is the usual CONSERVATIVE cull, not an intersection test: a crossing triangle near an edge or a corner of the region may lie wholly outside it (no
 * single plane has all three corners outside, yet the triangle passes the region by).  A triangle that does intersect the region is never rejected.
 *
 * THE BOX TEST that prunes a walk.  For plane k take per axis c_a = n_a >= 0 ? lo_a : hi_a; the box is rejected exactly when s_k(c) > 0 for some k.
 * Why a rejected box holds only rejected triangles, in binary32 itself: let x be a corner with lo_a <= x_a <= hi_a on every axis.  For a fixed finite
 * n_a the rounded product n_a * t is monotone in t (non-decreasing for n_a >= 0, non-increasing otherwise), and c_a is the end of [lo_a, hi_a] at which it
 * is smallest, so fl(n_a c_a) <= fl(n_a x_a) per axis.  Rounded addition is monotone in each operand, so operand by operand c's evaluation lies at or below
 * x's: fl(p0 + p1), then fl(. + p2), then fl(. + d).  Infinities: a product of finite factors may overflow.  If c's evaluation meets +inf at some operand,
 * x's operand there is >= it, so +inf too; the only way to a NaN is (+inf) + (-inf), and if x's evaluation met a -inf or a NaN at an operand, c's operand
 * there is <= it: -inf, or c's evaluation was NaN already -- and from then on c's evaluation stays -inf or NaN, neither of which is > 0.  So s_k(c) > 0
 * implies s_k(x) > 0 (and not NaN) for all three corners of every triangle whose corners lie in the box: out_k == 3, plane k rejects them.  The decoded
 * 4-wide boxes hold their triangles' corners (wide_frame), as the child-pair boxes do.  Hence the touching set, the inside set and every count are a
 * statement about triangles and this header alone, whichever records, fold or order is walked.
 *
 * THE LIST keeps the touching triangles with the LOWEST primitive ids, ascending: an order that depends on no tree.  RgList is within.h's WnList keyed by
 * the id alone: right-aligned, static indices only.  Its keys are id + 1, so that 0 (a place not used) sorts before every member and 0xFFFFFFFF (an
 * empty place) after; ids stay below 2^31 (RT_LEAF_BIT).
 *
 * THE PLANES OF A PIXEL RECTANGLE, region_of_rect(camera, width, height, x0, y0, x1, y1, t_near, t_far), the rectangle inclusive.  dir(cx, cy) is the guide
 * pass's pixel direction (sf_guide_dir) evaluated at the pixel CORNER (cx, cy) instead of a centre:
 *   u = (float)cx * (1 / (float)width), v = (float)cy * (1 / (float)height)             (a centre has (float)px + 0.5f here)
 *   u = (u * 2 - 1) * tan_half_fov * aspect_ratio, v = (v * 2 - 1) * tan_half_fov, tan_half_fov = rt_tanf(0.5f * fov)
 *   right = cross(front, up); d = right * u + up * v + front per component, summed left to right; dir = d / sqrtf(dx dx + dy dy + dz dz)
 * cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  With X0 = x0, X1 = x1 + 1, Y0 = y0, Y1 = y1 + 1 the side planes are, in this order,
 *   left   n = cross(dir(X0, Y0), dir(X0, Y1))       top     n = cross(dir(X0, Y0), dir(X1, Y0))
 *   right  n = cross(dir(X1, Y0), dir(X1, Y1))       bottom  n = cross(dir(X0, Y1), dir(X1, Y1))
 * each negated when np_dot3(n, c) > 0 for c = the same direction function at ((float)X0 + (float)X1) * 0.5f, ((float)Y0 + (float)Y1) * 0.5f (so the
 * rectangle's centre direction is inside), and d = -np_dot3(n, position): the plane passes through the camera position.  Then, perpendicular to front,
 *   near (t_near > 0)        (-front, np_dot3(front, position) + t_near)
 *   far  (t_far finite)      ( front, -(np_dot3(front, position) + t_far))
 * 4 to 6 planes. */
#ifndef RT_REGION_H
#define RT_REGION_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"
#include "nearest.h"

/* the list's functions take it by reference: on the device they must be inlined, or the list would have an address and live in scratch */
#if defined(__HIPCC__)
#define RG_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RG_FN static inline
#endif

RTD_FN float region_plane(const float pl[4], const float x[3]) { return ((pl[0] * x[0] + pl[1] * x[1]) + pl[2] * x[2]) + pl[3]; }

/* decided before any walk */
RTD_FN bool region_searched(uint32_t num_planes, const float* planes /* [num_planes][4] */)
{
    if (num_planes < 1u || num_planes > RT_REGION_MAX_PLANES) return false;
    bool finite = true;
    for (uint32_t k = 0; k < 4u * num_planes; ++k) finite = finite && __builtin_isfinite(planes[k]);
    return finite;
}

/* the box test of one plane: true when the plane rejects the box */
RTD_FN bool region_plane_rejects_box(const float pl[4], const float lo[3], const float hi[3])
{
    const float c[3] = {pl[0] >= 0.0f ? lo[0] : hi[0], pl[1] >= 0.0f ? lo[1] : hi[1], pl[2] >= 0.0f ? lo[2] : hi[2]};
    return region_plane(pl, c) > 0.0f;
}

/* how many of a triangle's corners are outside one plane */
RTD_FN uint32_t region_corners_outside(const float pl[4], const float p1[3], const float p2[3], const float p3[3])
{
    return (region_plane(pl, p1) > 0.0f ? 1u : 0u) + (region_plane(pl, p2) > 0.0f ? 1u : 0u) + (region_plane(pl, p3) > 0.0f ? 1u : 0u);
}

/* A triangle's class against a searched region, as a member's flags: RT_REGION_REJECTED, or RT_REGION_MEMBER_INSIDE when every out_k == 0, or the bits
 * RT_REGION_MEMBER_CROSSING_SHIFT + k of the planes with 1 or 2 corners outside. */
#define RT_REGION_REJECTED 0xFFFFFFFFu
RTD_FN uint32_t region_classify(uint32_t num_planes, const float* planes, const float p1[3], const float p2[3], const float p3[3])
{
    uint32_t flags = 0u;
    bool rejected = false;
    for (uint32_t k = 0; k < num_planes; ++k)
    {
        const uint32_t out = region_corners_outside(planes + 4u * k, p1, p2, p3);
        rejected = rejected || out == 3u;
        if (out != 0u) flags |= 1u << (RT_REGION_MEMBER_CROSSING_SHIFT + k);
    }
    if (rejected) return RT_REGION_REJECTED;
    return flags != 0u ? flags : RT_REGION_MEMBER_INSIDE;
}

struct RgList { uint32_t key[RT_REGION_LIST_MAX]; };          /* id + 1; 0: a place not used; 0xFFFFFFFF: empty */

RTD_FN uint32_t rg_list_first(uint32_t max_list) { return RT_REGION_LIST_MAX - (max_list > 0u ? max_list : 1u); }

RG_FN void rg_list_clear(RgList& l, uint32_t max_list)
{
    const uint32_t first = rg_list_first(max_list);
    for (int k = 0; k < RT_REGION_LIST_MAX; ++k) l.key[k] = (uint32_t)k >= first ? 0xFFFFFFFFu : 0u;
}

/* prim into its place; the largest of the kept and the new leaves (within.h's chain, keyed by the id alone) */
RG_FN void rg_list_insert(RgList& l, uint32_t prim)
{
    const uint32_t key = prim + 1u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = RT_REGION_LIST_MAX - 1; k >= 0; --k)
    {
        const bool before = key < l.key[k];
        const bool before_prev = k > 0 && key < l.key[k - (k > 0 ? 1 : 0)];
        l.key[k] = before ? (before_prev ? l.key[k - (k > 0 ? 1 : 0)] : key) : l.key[k];
    }
}

RTD_FN rt_region_hits region_record(uint32_t count, uint32_t inside, uint32_t max_list, bool searched)
{
    rt_region_hits r;
    r.count = count; r.inside = inside;
    r.stored = count < max_list ? count : max_list;
    r.flags = searched ? RT_REGION_HITS_SEARCHED : 0u;
    return r;
}

/* ---- the planes of a pixel rectangle (host arithmetic; the comment above states every operand order) */

RTD_FN void region_cross3(const float a[3], const float b[3], float o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

/* the guide pass's direction through image position (fx, fy) in pixels: sf_guide_dir has fx = (float)px + 0.5f */
RTD_FN void region_image_dir(const rt_camera& cam, float tan_half_fov, uint32_t width, uint32_t height, float fx, float fy, float d[3])
{
    const float inv_width = 1.0f / (float)width, inv_height = 1.0f / (float)height;
    float x = fx * inv_width, y = fy * inv_height;
    x = (x * 2.0f - 1.0f) * tan_half_fov * cam.aspect_ratio;
    y = (y * 2.0f - 1.0f) * tan_half_fov;
    const float f[3] = {cam.front.x, cam.front.y, cam.front.z}, u[3] = {cam.up.x, cam.up.y, cam.up.z};
    float r[3];
    region_cross3(f, u, r);
    const float dx = r[0] * x + u[0] * y + f[0], dy = r[1] * x + u[1] * y + f[1], dz = r[2] * x + u[2] * y + f[2];
    const float l = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    d[0] = dx / l; d[1] = dy / l; d[2] = dz / l;
}

RTD_FN rt_region region_of_rect(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float t_near, float t_far)
{
    rt_region g;
    g.num_planes = 0u; g.reserved[0] = g.reserved[1] = g.reserved[2] = 0u;
    for (int k = 0; k < RT_REGION_MAX_PLANES; ++k) for (int c = 0; c < 4; ++c) g.planes[k][c] = 0.0f;
    const float th = rt_tanf(0.5f * cam.fov);
    const float X0 = (float)x0, X1 = (float)(x1 + 1u), Y0 = (float)y0, Y1 = (float)(y1 + 1u);
    const float pos[3] = {cam.position.x, cam.position.y, cam.position.z}, f[3] = {cam.front.x, cam.front.y, cam.front.z};
    float d00[3], d10[3], d01[3], d11[3], c[3];
    region_image_dir(cam, th, width, height, X0, Y0, d00);
    region_image_dir(cam, th, width, height, X1, Y0, d10);
    region_image_dir(cam, th, width, height, X0, Y1, d01);
    region_image_dir(cam, th, width, height, X1, Y1, d11);
    region_image_dir(cam, th, width, height, (X0 + X1) * 0.5f, (Y0 + Y1) * 0.5f, c);
    const float* side[4][2] = {{d00, d01}, {d00, d10}, {d10, d11}, {d01, d11}};
    for (int k = 0; k < 4; ++k)
    {
        float n[3];
        region_cross3(side[k][0], side[k][1], n);
        if (np_dot3(n, c) > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        float* pl = g.planes[g.num_planes++];
        pl[0] = n[0]; pl[1] = n[1]; pl[2] = n[2]; pl[3] = -np_dot3(n, pos);
    }
    const float along = np_dot3(f, pos);
    if (t_near > 0.0f)
    {
        float* pl = g.planes[g.num_planes++];
        pl[0] = -f[0]; pl[1] = -f[1]; pl[2] = -f[2]; pl[3] = along + t_near;
    }
    if (__builtin_isfinite(t_far))
    {
        float* pl = g.planes[g.num_planes++];
        pl[0] = f[0]; pl[1] = f[1]; pl[2] = f[2]; pl[3] = -(along + t_far);
    }
    return g;
}

#endif /* RT_REGION_H */
