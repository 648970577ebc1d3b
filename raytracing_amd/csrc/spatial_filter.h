/* spatial_filter.h -- one pass of the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) for one pixel, shared by the
 * kernel k_sf_pass (filters.hip) and the host restatement behind rt_debug_filter(NULL, ...).  Both are compiled with
 * -ffp-contract=off and no fast-math and evaluate the exponential with rt_detmath.h's rt_expf, so they agree bit for bit.
 *
 * The filter, per pixel p of the whole image (width x height):
 *   h_p  HDR colour: k_resolve's colour branch before Reinhard (radiance / sample count; undivided with RT_OPT_DENOISER == 1)
 *   a_p, n_p, z_p  first-hit albedo, unit normal, depth; p is VALID iff z_p < RT_MAX_RENDER_DIST
 *   pass-through  p is invalid, a channel of h_p is not finite, or h_p / a_p overflows: every pass copies h_p, nothing is demodulated or
 *        remodulated, the output is h_p (a NaN pixel stays NaN and does not spread)
 *   demodulation (RT_FILTER_DEMODULATE), per channel: c = a >= 1e-3f ? h / a : h; without the flag c = h
 *   pass i = 0 .. N-1, step s = 1 << i, taps q = p + (s j, s k), j, k in -2 .. 2, hw = b[j+2] b[k+2], b = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *        a tap outside the image, invalid or with a non-finite channel contributes nothing;
 *        E = |c_p - c_q|^2 inv_c + (1 - dot(n_p, n_q)) inv_n + |z_p - z_q| inv_z / (z_p max(|dx|, |dy|))   (last term 0 for q = p)
 *        inv_c = 4^i / sigma_color^2, inv_n = 1 / sigma_normal, inv_z = 1 / sigma_depth (host floats)
 *        w = hw rt_expf(-E);  c'_p = sum w c_q / sum w, accumulated in float, dy-major from -2 to +2, in the form
 *        c'_p = c_p + sum w (c_q - c_p) / sum w (the same weighted mean; a flat region stays exactly flat, pass after pass)
 *   remodulation with the same rule (c' a), then (rt_frame_filter) Reinhard x / (x + 1) per channel; alpha 1.
 * Every sum, product and comparison below is written in the order stated: changing one changes bits. */
#ifndef RT_SPATIAL_FILTER_H
#define RT_SPATIAL_FILTER_H

#include <stdint.h>
#include "rt_types.h"
#include "rt_detmath.h"

struct alignas(16) sf_f4 { float x, y, z, w; };

#define SF_FIRST 1u       /* this pass reads h (col = the radiance sum / the caller's HDR image) and demodulates */
#define SF_LAST 2u        /* this pass remodulates */
#define SF_DIVIDE 4u      /* the first pass divides the radiance sum by spp */
#define SF_DEMOD 8u       /* RT_FILTER_DEMODULATE */
#define SF_TONEMAP 16u    /* the last pass applies Reinhard and writes alpha 1 */
#define SF_ALBEDO_MIN 1e-3f

struct SfPass
{
    const sf_f4* col;     /* the first pass: h (before the division by spp); later passes: the previous pass's c */
    const sf_f4* alb;     /* albedo guide (rgb) */
    const sf_f4* nz;      /* normal guide (xyz) + depth (w) */
    const sf_f4* src;     /* the first pass's col: the last pass writes h_p itself for a pass-through pixel */
    sf_f4* out;
    uint32_t width, height;
    uint32_t step;        /* 1 << i */
    uint32_t flags;       /* SF_* */
    float spp;
    float inv_c, inv_n, inv_z;
};

RTD_FN int sf_finite3(sf_f4 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

/* h_p itself: src[i], divided by spp under SF_DIVIDE */
RTD_FN sf_f4 sf_h(const sf_f4* src, uint32_t flags, float spp, uint32_t i)
{
    sf_f4 v = src[i];
    if (flags & SF_DIVIDE) { v.x = v.x / spp; v.y = v.y / spp; v.z = v.z / spp; }
    return v;
}

/* c of pixel i as a pass with these flags reads it from col (SF_FIRST: h, demodulated under SF_DEMOD); *through = pixel i passes through
 * (invalid or a non-finite channel of h) */
RTD_FN sf_f4 sf_load(const sf_f4* col, const sf_f4* alb, uint32_t flags, float spp, uint32_t i, float z, int* through)
{
    if (!(flags & SF_FIRST))
    {
        const sf_f4 v = col[i];
        *through = !(z < RT_MAX_RENDER_DIST) || !sf_finite3(v);
        return v;
    }
    const sf_f4 v = sf_h(col, flags, spp, i);
    *through = !(z < RT_MAX_RENDER_DIST) || !sf_finite3(v);
    if (!*through && (flags & SF_DEMOD))
    {
        const sf_f4 a = alb[i];
        sf_f4 c = v;
        if (a.x >= SF_ALBEDO_MIN) c.x = v.x / a.x;
        if (a.y >= SF_ALBEDO_MIN) c.y = v.y / a.y;
        if (a.z >= SF_ALBEDO_MIN) c.z = v.z / a.z;
        if (!sf_finite3(c)) *through = 1;     /* h / a overflowed: stored as it is (non-finite: later passes see a pass-through pixel too) */
        return c;
    }
    return v;
}

/* the remodulation: c' a per channel where a >= SF_ALBEDO_MIN */
RTD_FN sf_f4 sf_remodulate(sf_f4 r, sf_f4 a)
{
    if (a.x >= SF_ALBEDO_MIN) r.x = r.x * a.x;
    if (a.y >= SF_ALBEDO_MIN) r.y = r.y * a.y;
    if (a.z >= SF_ALBEDO_MIN) r.z = r.z * a.z;
    return r;
}

/* Reinhard x / (x + 1) per colour channel; .w as it is */
RTD_FN sf_f4 sf_reinhard(sf_f4 r)
{
    r.x = r.x / (r.x + 1.0f); r.y = r.y / (r.y + 1.0f); r.z = r.z / (r.z + 1.0f);
    return r;
}

/* the taps q = (x + step j, y + step k), j, k in -r .. r, k outer and j inner, of a width x height image: body(j, k, q's index) for each one
 * inside the image */
template <class F> RTD_FN void sf_stencil(uint32_t x, uint32_t y, uint32_t width, uint32_t height, int r, int step, F&& body)
{
    for (int k = -r; k <= r; ++k)
    {
        const int qy = (int)y + step * k;
        if (qy < 0 || qy >= (int)height) continue;
        for (int j = -r; j <= r; ++j)
        {
            const int qx = (int)x + step * j;
            if (qx < 0 || qx >= (int)width) continue;
            body(j, k, (uint32_t)qy * width + (uint32_t)qx);
        }
    }
}

/* the normal term 1 - dot(n_p, n_q) of guides gp, gq (normal xyz + depth w) */
RTD_FN float sf_normal_term(sf_f4 gp, sf_f4 gq) { return 1.0f - (gp.x * gq.x + gp.y * gq.y + gp.z * gq.z); }

/* the depth term |z_p - z_q| inv_z / (z_p step max(|j|, |k|)) of tap (j, k); 0 for the centre tap */
RTD_FN float sf_depth_term(sf_f4 gp, sf_f4 gq, float inv_z, int step, int j, int k)
{
    if (j == 0 && k == 0) return 0.0f;
    const int m = (j < 0 ? -j : j) > (k < 0 ? -k : k) ? (j < 0 ? -j : j) : (k < 0 ? -k : k);
    return __builtin_fabsf(gp.w - gq.w) * inv_z / (gp.w * (float)(step * m));
}

/* the guide pass's ray direction through the centre of pixel (px, py): raygen_ray (raygen_kernels.h) with both random offsets 0.5 and no lens,
 * cross3(front, up) and normalize3 (device_math.h) written out */
RTD_FN void sf_guide_dir(const rt_camera& cam, float tan_half_fov, uint32_t width, uint32_t height, uint32_t px, uint32_t py, float d[3])
{
    float inv_width = 1.0f / (float)width;
    float inv_height = 1.0f / (float)height;
    float x = ((float)px + 0.5f) * inv_width;
    float y = ((float)py + 0.5f) * inv_height;
    x = (x * 2.0f - 1.0f) * tan_half_fov * cam.aspect_ratio;
    y = (y * 2.0f - 1.0f) * tan_half_fov;
    const float fx = cam.front.x, fy = cam.front.y, fz = cam.front.z, ux = cam.up.x, uy = cam.up.y, uz = cam.up.z;
    const float rx = fy * uz - fz * uy, ry = fz * ux - fx * uz, rz = fx * uy - fy * ux;
    const float dx = rx * x + ux * y + fx, dy = ry * x + uy * y + fy, dz = rz * x + uz * y + fz;
    const float l = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    d[0] = dx / l; d[1] = dy / l; d[2] = dz / l;
}

/* the value pass P writes for pixel (x, y) */
RTD_FN sf_f4 sf_filter_pixel(const SfPass& P, uint32_t x, uint32_t y)
{
    const float b[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const uint32_t i = y * P.width + x;
    const sf_f4 gp = P.nz[i];
    int through = 0;
    const sf_f4 cp = sf_load(P.col, P.alb, P.flags, P.spp, i, gp.w, &through);
    sf_f4 r = cp;
    if (!through)
    {
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
        const int s = (int)P.step;
        sf_stencil(x, y, P.width, P.height, 2, s, [&](int j, int k, uint32_t qi) {
            const sf_f4 gq = P.nz[qi];
            int qthrough = 0;
            const sf_f4 cq = sf_load(P.col, P.alb, P.flags, P.spp, qi, gq.w, &qthrough);
            if (qthrough) return;
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            const float dc2 = dr * dr + dg * dg + db * db;
            const float e = dc2 * P.inv_c + sf_normal_term(gp, gq) * P.inv_n + sf_depth_term(gp, gq, P.inv_z, s, j, k);
            const float w = b[j + 2] * b[k + 2] * rt_expf(-e);
            sw = sw + w;
            sx = sx + w * (cq.x - cp.x); sy = sy + w * (cq.y - cp.y); sz = sz + w * (cq.z - cp.z);
        });
        if (sw > 0.0f) { r.x = cp.x + sx / sw; r.y = cp.y + sy / sw; r.z = cp.z + sz / sw; }   /* sw == 0 only if every weight underflowed (absurd sigmas): c_p stays */
    }
    if (P.flags & SF_LAST)
    {
        if (through || !sf_finite3(r)) r = sf_h(P.src, P.flags, P.spp, i);    /* h_p exactly: what pass-through means, whatever the passes carried */
        else if (P.flags & SF_DEMOD) r = sf_remodulate(r, P.alb[i]);
        if (P.flags & SF_TONEMAP)
        {
            r = sf_reinhard(r);
            r.w = 1.0f;
        }
    }
    return r;
}

#endif /* RT_SPATIAL_FILTER_H */
