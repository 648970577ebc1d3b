/* spatial_filter.h -- one pass of the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) for one pixel, shared by the
 * kernel k_sf_pass (spatial_filter.hip) and the host restatement behind rt_debug_filter(NULL, ...).  Both are compiled with
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

/* c of pixel i as pass P reads it; *through = pixel i passes through (invalid or a non-finite channel of h) */
RTD_FN sf_f4 sf_load(const SfPass& P, uint32_t i, float z, int* through)
{
    sf_f4 v = P.col[i];
    if (!(P.flags & SF_FIRST))
    {
        *through = !(z < RT_MAX_RENDER_DIST) || !sf_finite3(v);
        return v;
    }
    if (P.flags & SF_DIVIDE) { v.x = v.x / P.spp; v.y = v.y / P.spp; v.z = v.z / P.spp; }
    *through = !(z < RT_MAX_RENDER_DIST) || !sf_finite3(v);
    if (!*through && (P.flags & SF_DEMOD))
    {
        const sf_f4 a = P.alb[i];
        sf_f4 c = v;
        if (a.x >= SF_ALBEDO_MIN) c.x = v.x / a.x;
        if (a.y >= SF_ALBEDO_MIN) c.y = v.y / a.y;
        if (a.z >= SF_ALBEDO_MIN) c.z = v.z / a.z;
        if (!sf_finite3(c)) *through = 1;     /* h / a overflowed: stored as it is (non-finite: later passes see a pass-through pixel too) */
        return c;
    }
    return v;
}

/* the value pass P writes for pixel (x, y) */
RTD_FN sf_f4 sf_filter_pixel(const SfPass& P, uint32_t x, uint32_t y)
{
    const float b[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const uint32_t i = y * P.width + x;
    const sf_f4 gp = P.nz[i];
    int through = 0;
    const sf_f4 cp = sf_load(P, i, gp.w, &through);
    sf_f4 r = cp;
    if (!through)
    {
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
        const int s = (int)P.step;
        for (int k = -2; k <= 2; ++k)
        {
            const int qy = (int)y + s * k;
            if (qy < 0 || qy >= (int)P.height) continue;
            for (int j = -2; j <= 2; ++j)
            {
                const int qx = (int)x + s * j;
                if (qx < 0 || qx >= (int)P.width) continue;
                const uint32_t qi = (uint32_t)qy * P.width + (uint32_t)qx;
                const sf_f4 gq = P.nz[qi];
                int qthrough = 0;
                const sf_f4 cq = sf_load(P, qi, gq.w, &qthrough);
                if (qthrough) continue;
                const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                const float dc2 = dr * dr + dg * dg + db * db;
                const float dn = 1.0f - (gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
                float ez = 0.0f;
                if (j != 0 || k != 0)
                {
                    const int m = (j < 0 ? -j : j) > (k < 0 ? -k : k) ? (j < 0 ? -j : j) : (k < 0 ? -k : k);
                    ez = __builtin_fabsf(gp.w - gq.w) * P.inv_z / (gp.w * (float)(s * m));
                }
                const float e = dc2 * P.inv_c + dn * P.inv_n + ez;
                const float w = b[j + 2] * b[k + 2] * rt_expf(-e);
                sw = sw + w;
                sx = sx + w * (cq.x - cp.x); sy = sy + w * (cq.y - cp.y); sz = sz + w * (cq.z - cp.z);
            }
        }
        if (sw > 0.0f) { r.x = cp.x + sx / sw; r.y = cp.y + sy / sw; r.z = cp.z + sz / sw; }   /* sw == 0 only if every weight underflowed (absurd sigmas): c_p stays */
    }
    if (P.flags & SF_LAST)
    {
        through = through || !sf_finite3(r);
        if (through)
        {
            r = P.src[i];                     /* h_p exactly: what pass-through means, whatever the passes carried for it */
            if (P.flags & SF_DIVIDE) { r.x = r.x / P.spp; r.y = r.y / P.spp; r.z = r.z / P.spp; }
        }
        else if (P.flags & SF_DEMOD)
        {
            const sf_f4 a = P.alb[i];
            if (a.x >= SF_ALBEDO_MIN) r.x = r.x * a.x;
            if (a.y >= SF_ALBEDO_MIN) r.y = r.y * a.y;
            if (a.z >= SF_ALBEDO_MIN) r.z = r.z * a.z;
        }
        if (P.flags & SF_TONEMAP)
        {
            r.x = r.x / (r.x + 1.0f); r.y = r.y / (r.y + 1.0f); r.z = r.z / (r.z + 1.0f);
            r.w = 1.0f;
        }
    }
    return r;
}

#endif /* RT_SPATIAL_FILTER_H */
