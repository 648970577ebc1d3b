/* atlas.h -- which triangle every texel of a UV atlas shows, and where on it (rt_scene_atlas / rt_scene_atlas_bake / rt_debug_atlas),
 * stated once for the kernels (atlas.hip: k_atlas_cover, k_atlas_resolve, k_atlas_gutter) and the host restatement (rt_debug_atlas(NULL, ...)).  Integers
 * throughout: the two agree byte for byte whatever order the triangles are met in.
 *
 * The atlas: width x height texels, both 1 .. 16384, width * height <= 2^26; texel (x, y) has index y * width + x, row 0 is v = 0.  Its centre in fixed point
 * with 8 sub-texel bits is Px = 256 x + 128, Py = 256 y + 128.
 *
 * A corner (u, v) snaps to X = rintf(u * (float)(256 * width)), Y = rintf(v * (float)(256 * height)): one binary32 multiply each, rounded to the nearest even
 * integer, kept as int64.  A triangle is SKIPPED when a component is not finite, when some |X| or |Y| exceeds 2^24 (so every difference is below 2^26, every
 * edge function below 2^53, and every conversion to binary64 below is exact), or when its doubled area A = E(c1, c2, c3) is 0.
 *
 * E(a, b, p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x), exact and exactly antisymmetric in a, b.  With s = sign(A):
 *   w1 = s E(c2, c3, P), w2 = s E(c3, c1, P), w3 = s E(c1, c2, P)                (w1 + w2 + w3 = |A|)
 * A centre is COVERED when every w_i > 0, or w_i == 0 on an edge that owns its points: an edge traversed a -> b in the s-normalised orientation, with
 * (dx, dy) = s (b - a), owns when dy > 0 || (dy == 0 && dx < 0).  Of d and -d exactly one owns, and two triangles on opposite sides of a shared edge traverse
 * it in opposite directions once normalised, so every centre on it goes to exactly one of them whatever their winding.  Both windings rasterise.
 *
 * Per texel, over every triangle that passes the object filter and is not skipped: count = how many cover its centre (saturating at 65535 in the record),
 * primitive_id = the lowest covering id, and of that owner bu = (float)((double)w2 / (double)|A|), bv = (float)((double)w3 / (double)|A|) -- rt_hit's bc, the
 * weights of corners 2 and 3.  Only the centres inside the atlas exist: a triangle's texel box is clamped to the atlas before anything loops over it.
 *
 * The gutter: `gutter` passes (0 .. 4), each reading the records of the pass before and writing new ones.  A texel whose flags are 0 takes the record of the
 * first neighbour whose flags are not 0 -- a covered one or an earlier pass's gutter -- in the order left (x - 1), right (x + 1), up (y - 1), down (y + 1),
 * up-left, up-right, down-left, down-right; a neighbour outside the atlas does not count.  The copy has flags = RT_TEXEL_GUTTER and count = 0. */
#ifndef RT_ATLAS_H
#define RT_ATLAS_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"

#define RT_ATLAS_MAX_SIDE 16384u
#define RT_ATLAS_MAX_TEXELS (1u << 26)
#define RT_ATLAS_MAX_GUTTER 4u
#define RT_ATLAS_SNAP_BOUND 16777216.0f     /* 2^24 */

/* a triangle as the cover needs it: the snapped corners, |A|, s, and the texel box [x0, x1] x [y0, y1] clamped to the atlas (empty when x0 > x1 or y0 > y1) */
struct AtlasTri
{
    int32_t x[3], y[3];      /* |.| <= 2^24 */
    int32_t s;               /* sign(A) */
    int32_t x0, y0, x1, y1;
    int64_t area;            /* |A| > 0 */
};

RTD_FN int64_t atlas_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

/* the edge a -> b, already in the s-normalised orientation, owns the points on it */
RTD_FN bool atlas_owns(int64_t dx, int64_t dy) { return dy > 0 || (dy == 0 && dx < 0); }

RTD_FN int32_t atlas_min3(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
RTD_FN int32_t atlas_max3(int32_t a, int32_t b, int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }

/* uv = u1 v1 u2 v2 u3 v3.  false: the triangle is skipped */
RTD_FN bool atlas_setup(const float uv[6], uint32_t width, uint32_t height, AtlasTri* t)
{
    const float sx = (float)(256u * width), sy = (float)(256u * height);
    for (int k = 0; k < 3; ++k)
    {
        const float fx = __builtin_rintf(uv[2 * k] * sx), fy = __builtin_rintf(uv[2 * k + 1] * sy);
        /* written so that a NaN fails it: a non-finite component gives a NaN or an infinite product */
        if (!(__builtin_fabsf(fx) <= RT_ATLAS_SNAP_BOUND) || !(__builtin_fabsf(fy) <= RT_ATLAS_SNAP_BOUND)) return false;
        if (!__builtin_isfinite(uv[2 * k]) || !__builtin_isfinite(uv[2 * k + 1])) return false;
        t->x[k] = (int32_t)fx; t->y[k] = (int32_t)fy;
    }
    const int64_t a = atlas_edge(t->x[0], t->y[0], t->x[1], t->y[1], t->x[2], t->y[2]);
    if (a == 0) return false;
    t->s = a > 0 ? 1 : -1;
    t->area = a > 0 ? a : -a;
    /* the texels whose centres 256 x + 128 lie within [min, max]: x >= ceil((min - 128) / 256), x <= floor((max - 128) / 256); >> 8 floors a negative too */
    const int32_t lx = atlas_min3(t->x[0], t->x[1], t->x[2]), hx = atlas_max3(t->x[0], t->x[1], t->x[2]);
    const int32_t ly = atlas_min3(t->y[0], t->y[1], t->y[2]), hy = atlas_max3(t->y[0], t->y[1], t->y[2]);
    const int32_t bx0 = (lx - 128 + 255) >> 8, bx1 = (hx - 128) >> 8, by0 = (ly - 128 + 255) >> 8, by1 = (hy - 128) >> 8;
    t->x0 = bx0 > 0 ? bx0 : 0; t->y0 = by0 > 0 ? by0 : 0;
    t->x1 = bx1 < (int32_t)width - 1 ? bx1 : (int32_t)width - 1; t->y1 = by1 < (int32_t)height - 1 ? by1 : (int32_t)height - 1;
    return true;
}

/* w[i] of the centre of texel (x, y) */
RTD_FN void atlas_weights(const AtlasTri& t, int32_t x, int32_t y, int64_t w[3])
{
    const int64_t px = 256 * (int64_t)x + 128, py = 256 * (int64_t)y + 128;
    w[0] = t.s * atlas_edge(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
    w[1] = t.s * atlas_edge(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
    w[2] = t.s * atlas_edge(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
}

/* the rule: every w_i > 0, or 0 on an edge that owns.  w[i] belongs to the edge from corner i + 1 to corner i + 2 */
RTD_FN bool atlas_covered(const AtlasTri& t, const int64_t w[3])
{
    for (int i = 0; i < 3; ++i)
    {
        if (w[i] > 0) continue;
        if (w[i] < 0) return false;
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        if (!atlas_owns((int64_t)t.s * (t.x[b] - t.x[a]), (int64_t)t.s * (t.y[b] - t.y[a]))) return false;
    }
    return true;
}

RTD_FN bool atlas_covers(const AtlasTri& t, int32_t x, int32_t y)
{
    int64_t w[3];
    atlas_weights(t, x, y, w);
    return atlas_covered(t, w);
}

/* the owner's barycentrics at the centre of texel (x, y) */
RTD_FN void atlas_bc(const AtlasTri& t, int32_t x, int32_t y, float bc[2])
{
    int64_t w[3];
    atlas_weights(t, x, y, w);
    bc[0] = (float)((double)w[1] / (double)t.area);
    bc[1] = (float)((double)w[2] / (double)t.area);
}

RTD_FN rt_texel atlas_uncovered(void)
{
    rt_texel r;
    r.bc[0] = 0.0f; r.bc[1] = 0.0f; r.primitive_id = RT_INVALID_ID; r.count = 0u; r.flags = 0u;
    return r;
}

/* the eight neighbours in the gutter's order */
#define RT_ATLAS_NEIGHBOURS {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}}

/* why a description is refused (nullptr: it is fine) */
RTD_FN const char* atlas_desc_refusal(const rt_atlas_desc& d)
{
    if (d.width == 0u || d.height == 0u || d.width > RT_ATLAS_MAX_SIDE || d.height > RT_ATLAS_MAX_SIDE || (uint64_t)d.width * d.height > RT_ATLAS_MAX_TEXELS)
        return "width and height must be 1 .. 16384 with width * height <= 2^26";
    if (d.gutter > RT_ATLAS_MAX_GUTTER) return "gutter must be 0 .. 4";
    return nullptr;
}

#endif /* RT_ATLAS_H */
