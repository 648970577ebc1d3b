/* light_bake.h -- the arithmetic of a light bake (rt_scene_light_bake / rt_scene_light_bake_buffer / rt_scene_atlas_bake_light / rt_debug_light_bake_rays /
 * rt_debug_light_bake_reduce): the irradiance a point receives from the environment and from the scene's analytic lights, direct terms
 * only, stated once for the kernels (light_bake_kernels.h) and the host restatement.  binary32 throughout except rt_detmath.h's functions (binary64, rounded
 * once), -ffp-contract=off, correctly rounded divide and square root on both sides, so the two agree bit for bit.  tests/test_light_bake.py restates every
 * step in numpy.
 *
 * A point record, the rule by which it is SKIPPED, its frame and its biased origin are bake.h's bake_point / bake_frame, unchanged; with
 * RT_BAKE_FROM_SURFACES the record is an rt_surface.  The rotations (r1, r2) of point i are bake.h's bake_rotations(i, seed).
 *
 * Items.  M = the scene's light count, L = min(samples, 64).  A walked point has samples + M items; item r belongs to reduction slot r % L and a slot
 * handles its items in rising r.  An item either MAKES A RAY (origin = the biased origin, t_min = 0) or makes none: then its ray is all zeros, it adds
 * nothing and it is counted nowhere.
 *
 * Sky item (r < samples; light_bake_sky_item): makes no ray with RT_LIGHT_BAKE_NO_SKY.  Otherwise direction = bake_direction(f, r1, r2, k = r, samples),
 *   t_max = sky_distance.  When nothing lies in that range (a ray no query walks -- a non-finite component, an all-zero direction -- meets nothing):
 *   d = normalize3(direction) (l = sqrtf((x x + y y) + z z), three divides, as query.h's), d.z clamped to [-1, 1] (z > 1 ? 1 : z < -1 ? -1 : z), and the
 *   environment at d (light_bake_sky: shade_kernels.h's SampleSky, line for line, with its rule for NaN coordinates -- texel (0, 0), never an address
 *   outside the image) is added to the slot's sky sum, channel by channel; the ray counts in sky_unoccluded.
 *
 * Light item (r >= samples, light j = r - samples; light_bake_light_item): makes no ray with RT_LIGHT_BAKE_NO_LIGHTS.  Otherwise
 *   v  = light.origin - origin for a point light (RT_LIGHT_TYPE_POINT), light.origin for every other type (directional: the reference's else branch)
 *   d2 = (v.x v.x + v.y v.y) + v.z v.z
 *   c  = ((n.x v.x + n.y v.y) + n.z v.z) / sqrtf(d2)            (n: the frame's unit normal)
 *   no ray when a component of the origin, of v or of the radiance is not finite, when d2 is zero or not finite, or when !(c > 0);
 *   point:        direction v, t_max = 1 (the segment ends at the light),       E = (radiance / d2) * c   per channel
 *   directional:  direction normalize3(v), t_max = sky_distance,                E = radiance * c          per channel
 *   When nothing lies in the ray's range E is added to the slot's light sum and the item counts in lights_unshadowed.
 *
 * Reduction (light_bake_reduce_point's order): every slot starts both of its triples at +0; the L slot sums of each triple are combined by bake.h's halving
 * tree v[l] += v[l + s] for s = L/2 .. 1, l < s; S = v[0].  sky = S_sky * (RT_PI / (float)samples), the cosine-weighted estimator of irradiance;
 * lights = S_lights.  A skipped point: zeros, and both counts RT_INVALID_ID.
 *
 * Ray directions need not be unit length (a point light's is v): the walks take such rays.  M == 0 is allowed.  With equal samples, seed, bias and
 * radius == sky_distance the sky rays are the occlusion bake's, so sky_unoccluded = rt_scene_bake's unoccluded. */
#ifndef RT_LIGHT_BAKE_H
#define RT_LIGHT_BAKE_H

#include <stdint.h>
#include "rt_hip.h"
#include "rt_detmath.h"
#include "bake.h"

#define RT_LIGHT_BAKE_FLAGS_KNOWN (RT_BAKE_FROM_SURFACES | RT_LIGHT_BAKE_NO_SKY | RT_LIGHT_BAKE_NO_LIGHTS)

struct LightBakeItem
{
    float dir[3];
    float t_max;
    float E[3];        /* a light item's contribution when its ray is unoccluded; zeros for a sky item (its contribution is looked up when the ray has ended) */
    bool made;         /* false: no ray, nothing added, nothing counted */
};

RTD_FN LightBakeItem light_bake_no_ray()
{
    LightBakeItem it;
    for (int q = 0; q < 3; ++q) { it.dir[q] = 0.0f; it.E[q] = 0.0f; }
    it.t_max = 0.0f;
    it.made = false;
    return it;
}

RTD_FN void light_bake_normalize3(const float v[3], float out[3])
{
    const float l = __builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int q = 0; q < 3; ++q) out[q] = v[q] / l;
}

/* sky item k of a walked point */
RTD_FN LightBakeItem light_bake_sky_item(const BakeFrame& f, float r1, float r2, uint32_t k, uint32_t samples, uint32_t flags, float sky_distance)
{
    LightBakeItem it = light_bake_no_ray();
    if (flags & RT_LIGHT_BAKE_NO_SKY) return it;
    bake_direction(f, r1, r2, k, samples, it.dir);
    it.t_max = sky_distance;
    it.made = true;
    return it;
}

/* the light item of a walked point for the light (origin lo, radiance lr, type) */
RTD_FN LightBakeItem light_bake_light_item(const BakeFrame& f, const float lo[3], const float lr[3], uint32_t type, uint32_t flags, float sky_distance)
{
    LightBakeItem it = light_bake_no_ray();
    if (flags & RT_LIGHT_BAKE_NO_LIGHTS) return it;
    const bool point = type == RT_LIGHT_TYPE_POINT;
    float v[3];
    for (int q = 0; q < 3; ++q) v[q] = point ? lo[q] - f.origin[q] : lo[q];
    const float d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const float c = ((f.n[0] * v[0] + f.n[1] * v[1]) + f.n[2] * v[2]) / __builtin_sqrtf(d2);
    const bool finite = __builtin_isfinite(f.origin[0]) && __builtin_isfinite(f.origin[1]) && __builtin_isfinite(f.origin[2]) &&
                        __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]) &&
                        __builtin_isfinite(lr[0]) && __builtin_isfinite(lr[1]) && __builtin_isfinite(lr[2]);
    if (!(finite && d2 > 0.0f && __builtin_isfinite(d2) && c > 0.0f)) return it;
    if (point)
    {
        for (int q = 0; q < 3; ++q) { it.dir[q] = v[q]; it.E[q] = (lr[q] / d2) * c; }
        it.t_max = 1.0f;
    }
    else
    {
        light_bake_normalize3(v, it.dir);
        for (int q = 0; q < 3; ++q) it.E[q] = lr[q] * c;
        it.t_max = sky_distance;
    }
    it.made = true;
    return it;
}

/* The environment in the direction of an unoccluded sky ray: the direction normalised, its z clamped, then SampleSky's arithmetic (miss.cl:28-39 with the
 * OpenCL 1.2 linear / repeat / normalized sampler) on w x h RGBA texels.  T4: a 16-byte record with x, y, z (float4 on the device, rt_float4 on the host). */
template <class T4>
RTD_FN void light_bake_sky(const T4* env, int w, int h, const float direction[3], float rgb[3])
{
    float dir[3];
    light_bake_normalize3(direction, dir);
    dir[2] = dir[2] > 1.0f ? 1.0f : (dir[2] < -1.0f ? -1.0f : dir[2]);
    float cx = rt_atan2f(dir[0], dir[1]) + RT_PI;
    float cy = rt_acosf(dir[2]);
    cx = cx < 0.0f ? cx + RT_TWO_PI : cx;
    cx *= RT_INV_TWO_PI;
    cy *= RT_INV_PI;
    float u = (cx - __builtin_floorf(cx)) * (float)w;
    float v = (cy - __builtin_floorf(cy)) * (float)h;
    float fu = __builtin_floorf(u - 0.5f);
    float fv = __builtin_floorf(v - 0.5f);
    /* NaN coordinates: texel (0, 0), NaN weights, a NaN sample -- never an address outside the image */
    int i0 = fu != fu ? 0 : (int)fu, j0 = fv != fv ? 0 : (int)fv;
    int i1 = i0 + 1, j1 = j0 + 1;
    if (i0 < 0) i0 = w + i0;
    if (i1 > w - 1) i1 = i1 - w;
    if (j0 < 0) j0 = h + j0;
    if (j1 > h - 1) j1 = j1 - h;
    float a = (u - 0.5f) - fu;
    float b = (v - 0.5f) - fv;
    float wa0 = 1.0f - a, wb0 = 1.0f - b;
    const T4 t00 = env[(size_t)j0 * w + i0];
    const T4 t10 = env[(size_t)j0 * w + i1];
    const T4 t01 = env[(size_t)j1 * w + i0];
    const T4 t11 = env[(size_t)j1 * w + i1];
    float w00 = wa0 * wb0, w10 = a * wb0, w01 = wa0 * b, w11 = a * b;
    rgb[0] = w00 * t00.x + w10 * t10.x + w01 * t01.x + w11 * t11.x;
    rgb[1] = w00 * t00.y + w10 * t10.y + w01 * t01.y + w11 * t11.y;
    rgb[2] = w00 * t00.z + w10 * t10.z + w01 * t01.z + w11 * t11.z;
}

/* what the reduced sums of a walked point become */
RTD_FN void light_bake_finish(const float S_sky[3], uint32_t samples, float sky[3])
{
    const float scale = RT_PI / (float)samples;
    for (int q = 0; q < 3; ++q) sky[q] = S_sky[q] * scale;
}

#endif /* RT_LIGHT_BAKE_H */
