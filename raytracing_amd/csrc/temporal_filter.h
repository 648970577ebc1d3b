/* temporal_filter.h -- the spatiotemporal variance-guided filter (SVGF, Schied et al. HPG 2017) for one pixel, shared by the kernels of
 * filters.hip and their host restatement behind rt_debug_filter_temporal(NULL, ...).  Both are compiled with -ffp-contract=off and
 * no fast-math and evaluate the exponential with rt_detmath.h's rt_expf, so they agree bit for bit.  spatial_filter.h's rules, and its functions
 * that state them, hold unchanged where they apply: h_p, demodulation by albedo >= 1e-3 (sf_load), the pass-through pixels, the B3 taps 2^i apart,
 * the normal and depth terms, the c_p + sum w (c_q - c_p) / sum w form of every weighted mean.
 *
 * Per call, per pixel p of the whole image (width x height):
 *   1. reproject: X = cam.position + z_p d_p (d_p: sf_guide_dir, the guide pass's pixel-centre direction); X is projected through the
 *      previous call's camera with ProjectScreen's arithmetic (aov_kernels.h) to the continuous pixel (u W - 0.5, v H - 0.5); X behind that
 *      camera, or a position outside (-1, W) x (-1, H), misses.  Bilinear 2 x 2 taps; a tap counts iff its bilinear weight is > 0, it lies
 *      inside the image, its history length is > 0 (it was valid at the previous call), |z_prev,q - |X - prev.position|| <= TF_DEPTH_TOL
 *      |X - prev.position| and dot(n_p, n_prev,q) >= TF_NORMAL_MIN.  The counting weights are renormalised; no tap counts = a miss.
 *      TF_IDENTITY (same camera bytes, same scene): one tap, p itself, weight 1, counting iff its history length is > 0.
 *      TF_NO_HISTORY: every pixel misses.
 *      Moved geometry (prev_pos / prev_n set: the first hit in the pose BEFORE the last refit, tf_guide_motion; only under TF_REPROJECT, also with a
 *      standing camera): a pixel with prev_pos.w != 0 takes X = prev_pos.xyz instead of cam.position + z_p d_p, and its normal test reads
 *      dot(prev_n, n_prev,q) >= TF_NORMAL_MIN.  Nothing else changes: the previous call's guides saw the previous pose, so |X - prev.position| against
 *      z_prev,q compares like with like.  prev_pos.w == 0 (no motion known), or both images null: the rule above, bit for bit.
 *   2. accumulate: c_p demodulated, l = 0.2126 r + 0.7152 g + 0.0722 b.  Hit: L' = min(L_h + 1, TF_MAX_LEN) (L_h the largest length among
 *      the counting taps), alpha = max(alpha_color, 1 / L'), alpha_m = max(alpha_moments, 1 / L'); colour C_h + alpha (c_p - C_h), moments
 *      M_h + alpha_m ((l, l^2) - M_h); alpha == 1 takes c_p exactly (alpha_m == 1 (l, l^2) exactly).  Miss: L' = 1, c_p, (l, l^2).
 *      A pass-through pixel stores colour 0 and moments (0, 0, L' = 0): nothing reprojects from it, and every later stage passes it through.
 *   3. variance: L' >= TF_MOMENTS_MIN_LEN: max(0, mu2 - mu1^2); else over the (2 TF_VAR_RADIUS + 1)^2 neighbours at step 1 with L' > 0,
 *      w = rt_expf(-(dn inv_n + ez)) (the a-trous normal and depth terms, no colour term, no spatial kernel), m = moments_p + sum w
 *      (moments_q - moments_p) / sum w, var = max(0, m2 - m1^2).  The variance travels in the .w channel of the ping-pong images.
 *   4. pass i = 0 .. N-1 (step 2^i, the B3 taps): g_p = the 3 x 3 {1/4, 1/2, 1/4} Gaussian of the variance over the neighbours with L' > 0,
 *      renormalised; E = |l_p - l_q| / (sigma_luminance sqrt(g_p) + TF_LUM_EPS) + dn inv_n + ez; w = hw rt_expf(-E);
 *      c' = c_p + sum w (c_q - c_p) / sum w, var' = sum w^2 var_q / (sum w)^2.  Pass 0's colour is the stored history (no pass: step 2's).
 *   5. finish: pass-through (L' == 0 or a non-finite result), and a pixel whose result is its own c_p (alpha == 1 or a miss, and no pass),
 *      output h_p itself; others are remodulated (spatial_filter.h's rule); rt_frame_filter_temporal then applies Reinhard.  Alpha 1.
 * Every sum, product and comparison below is written in the order stated: changing one changes bits. */
#ifndef RT_TEMPORAL_FILTER_H
#define RT_TEMPORAL_FILTER_H

#include "spatial_filter.h"

#define TF_DEPTH_TOL 0.1f          /* a reprojected tap's depth may differ by this fraction of |X - prev.position| */
#define TF_NORMAL_MIN 0.9f         /* ... and its normal must keep dot(n_p, n_prev,q) >= this */
#define TF_MOMENTS_MIN_LEN 4.0f    /* a history this long estimates the variance from its own moments */
#define TF_VAR_RADIUS 3            /* else the 7 x 7 spatial estimate */
#define TF_MAX_LEN 1024.0f         /* the history length saturates here */
#define TF_LUM_EPS 1e-4f           /* keeps the luminance term finite where the variance is 0 */

#define TF_NO_HISTORY 0u
#define TF_IDENTITY 1u
#define TF_REPROJECT 2u

struct TfAccum
{
    const sf_f4* col;       /* h: the radiance sum (SF_DIVIDE) or the caller's HDR image */
    const sf_f4* alb;
    const sf_f4* nz;        /* this call's guides: unit normal + depth */
    const sf_f4* prev_nz;   /* the previous call's */
    const sf_f4* hist;      /* the previous call's colour history (rgb) and moments (mu1, mu2, L) */
    const sf_f4* mom;
    sf_f4* out_col;         /* the accumulated colour; .w = 1 where it is c_p itself */
    sf_f4* out_mom;         /* the new moments and length */
    rt_camera cam, prev;
    float tan_cam, tan_prev;   /* rt_tanf(0.5 fov) of each, on the host */
    uint32_t width, height;
    uint32_t mode;          /* TF_NO_HISTORY, TF_IDENTITY, TF_REPROJECT */
    uint32_t flags;         /* SF_DIVIDE, SF_DEMOD */
    float spp, alpha_color, alpha_moments;
    const sf_f4* prev_pos;  /* moved geometry: where each first hit was before the last refit (xyz, w = 1; w = 0: no motion known), or null */
    const sf_f4* prev_n;    /* ... and its unit normal there (w 0); null iff prev_pos is */
};

struct TfVar
{
    const sf_f4* acc;       /* the accumulated colour */
    const sf_f4* mom;       /* the new moments and length */
    const sf_f4* nz;
    sf_f4* out;             /* (colour, variance) */
    uint32_t width, height;
    float inv_n, inv_z;
};

struct TfPass
{
    const sf_f4* col;       /* (colour, variance); with zero passes: the accumulated colour (.w 1: c_p itself) */
    const sf_f4* mom;       /* L' > 0 marks the pixels that filter */
    const sf_f4* alb;
    const sf_f4* nz;
    const sf_f4* src;       /* h, for the pixels that output h_p */
    sf_f4* out;
    sf_f4* hist;            /* non-null: the colour history is written here too (pass 0, or the finish of zero passes) */
    uint32_t width, height;
    uint32_t step;          /* 1 << i; 0 = no filtering, only the finish (zero passes) */
    uint32_t flags;         /* SF_LAST, SF_DIVIDE, SF_DEMOD, SF_TONEMAP */
    float spp;
    float sigma_l, inv_n, inv_z;
};

RTD_FN float tf_lum(sf_f4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
RTD_FN float tf_max(float a, float b) { return a < b ? b : a; }
RTD_FN float tf_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

/* ProjectScreen (aov_kernels.h) of X through cam, as a continuous pixel position; 0 when X is not in front of the camera */
RTD_FN int tf_project(const rt_camera& cam, float tan_half_fov, uint32_t width, uint32_t height, const float X[3], float* sx, float* sy)
{
    const float px = X[0] - cam.position.x, py = X[1] - cam.position.y, pz = X[2] - cam.position.z;
    const float l = __builtin_sqrtf(px * px + py * py + pz * pz);
    const float dx = px / l, dy = py / l, dz = pz / l;
    const float fx = cam.front.x, fy = cam.front.y, fz = cam.front.z, ux = cam.up.x, uy = cam.up.y, uz = cam.up.z;
    const float den = tf_dot(fx, fy, fz, dx, dy, dz);
    if (!(den > 0.0f)) return 0;
    const float ix = dx / den, iy = dy / den, iz = dz / den;
    const float rx = fy * uz - fz * uy, ry = fz * ux - fx * uz, rz = fx * uy - fy * ux;
    float u = tf_dot(rx, ry, rz, ix, iy, iz) / (tan_half_fov * cam.aspect_ratio);
    float v = tf_dot(ux, uy, uz, ix, iy, iz) / (tan_half_fov);
    u = u * 0.5f + 0.5f;
    v = v * 0.5f + 0.5f;
    *sx = u * (float)width - 0.5f;
    *sy = v * (float)height - 0.5f;
    return 1;
}

/* where a first hit at barycentrics (bu, bv) was in another pose of its triangle: rec = that pose's three positions and three shading normals
 * (the xyz of the shading record's q0 .. q5), interpolated in k_sf_guide_values' operand order.  pos = (X', 1), nrm = (n', 0). */
RTD_FN void tf_guide_motion(const sf_f4* rec, float bu, float bv, sf_f4* pos, sf_f4* nrm)
{
    const sf_f4 p1 = rec[0], p2 = rec[1], p3 = rec[2], n1 = rec[3], n2 = rec[4], n3 = rec[5];
    const float w0 = 1.0f - bu - bv;
    pos->x = p1.x * w0 + p2.x * bu + p3.x * bv; pos->y = p1.y * w0 + p2.y * bu + p3.y * bv; pos->z = p1.z * w0 + p2.z * bu + p3.z * bv;
    pos->w = 1.0f;
    const float nx = n1.x * w0 + n2.x * bu + n3.x * bv, ny = n1.y * w0 + n2.y * bu + n3.y * bv, nz = n1.z * w0 + n2.z * bu + n3.z * bv;
    const float l = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
    nrm->x = nx / l; nrm->y = ny / l; nrm->z = nz / l; nrm->w = 0.0f;
}

/* steps 1 and 2 for pixel (x, y) */
RTD_FN void tf_accumulate_pixel(const TfAccum& A, uint32_t x, uint32_t y)
{
    const uint32_t i = y * A.width + x;
    const sf_f4 gp = A.nz[i];
    int through = 0;
    const sf_f4 c = sf_load(A.col, A.alb, SF_FIRST | A.flags, A.spp, i, gp.w, &through);
    if (through)
    {
        const sf_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        A.out_col[i] = zero; A.out_mom[i] = zero;
        return;
    }
    const float l = tf_lum(c);
    int hit = 0;
    float lh = 0.0f;
    sf_f4 ch = c, mh = c;
    if (A.mode == TF_IDENTITY)
    {
        const sf_f4 m = A.mom[i];
        if (m.z > 0.0f) { hit = 1; lh = m.z; ch = A.hist[i]; mh = m; }
    }
    else if (A.mode == TF_REPROJECT)
    {
        float d[3], X[3];
        float npx = gp.x, npy = gp.y, npz = gp.z;              /* the normal the taps are tested against */
        int moved = 0;
        if (A.prev_pos)
        {
            const sf_f4 pp = A.prev_pos[i];
            if (pp.w != 0.0f)
            {
                const sf_f4 pn = A.prev_n[i];
                moved = 1;
                X[0] = pp.x; X[1] = pp.y; X[2] = pp.z;
                npx = pn.x; npy = pn.y; npz = pn.z;
            }
        }
        if (!moved)
        {
            sf_guide_dir(A.cam, A.tan_cam, A.width, A.height, x, y, d);
            X[0] = A.cam.position.x + gp.w * d[0]; X[1] = A.cam.position.y + gp.w * d[1]; X[2] = A.cam.position.z + gp.w * d[2];
        }
        const float ex = X[0] - A.prev.position.x, ey = X[1] - A.prev.position.y, ez = X[2] - A.prev.position.z;
        const float dist = __builtin_sqrtf(ex * ex + ey * ey + ez * ez);
        float sx = 0.0f, sy = 0.0f;
        if (tf_project(A.prev, A.tan_prev, A.width, A.height, X, &sx, &sy) && sx > -1.0f && sx < (float)A.width && sy > -1.0f && sy < (float)A.height)
        {
            const float x0f = __builtin_floorf(sx), y0f = __builtin_floorf(sy);
            const float fx = sx - x0f, fy = sy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;
            float sw = 0.0f;
            sf_f4 sc = {0.0f, 0.0f, 0.0f, 0.0f}, sm = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int t = 0; t < 4; ++t)
            {
                const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                const float bw = ((t & 1) ? fx : 1.0f - fx) * ((t >> 1) ? fy : 1.0f - fy);
                if (!(bw > 0.0f) || qx < 0 || qx >= (int)A.width || qy < 0 || qy >= (int)A.height) continue;
                const uint32_t qi = (uint32_t)qy * A.width + (uint32_t)qx;
                const sf_f4 mq = A.mom[qi];
                if (!(mq.z > 0.0f)) continue;
                const sf_f4 gq = A.prev_nz[qi];
                if (!(__builtin_fabsf(gq.w - dist) <= TF_DEPTH_TOL * dist)) continue;
                if (!(tf_dot(npx, npy, npz, gq.x, gq.y, gq.z) >= TF_NORMAL_MIN)) continue;
                const sf_f4 cq = A.hist[qi];
                if (!hit) { hit = 1; ch = cq; mh = mq; }
                sw = sw + bw;
                sc.x = sc.x + bw * (cq.x - ch.x); sc.y = sc.y + bw * (cq.y - ch.y); sc.z = sc.z + bw * (cq.z - ch.z);
                sm.x = sm.x + bw * (mq.x - mh.x); sm.y = sm.y + bw * (mq.y - mh.y);
                lh = tf_max(lh, mq.z);
            }
            if (hit)
            {
                ch.x = ch.x + sc.x / sw; ch.y = ch.y + sc.y / sw; ch.z = ch.z + sc.z / sw;
                mh.x = mh.x + sm.x / sw; mh.y = mh.y + sm.y / sw;
            }
        }
    }
    sf_f4 r = c, m;
    m.x = l; m.y = l * l; m.z = 1.0f; m.w = 0.0f;
    r.w = 1.0f;
    if (hit)
    {
        const float len = lh + 1.0f < TF_MAX_LEN ? lh + 1.0f : TF_MAX_LEN;
        const float inv = 1.0f / len;
        const float a = tf_max(A.alpha_color, inv), am = tf_max(A.alpha_moments, inv);
        if (a != 1.0f)
        {
            r.x = ch.x + a * (c.x - ch.x); r.y = ch.y + a * (c.y - ch.y); r.z = ch.z + a * (c.z - ch.z);
            r.w = 0.0f;
        }
        if (am != 1.0f) { m.x = mh.x + am * (l - mh.x); m.y = mh.y + am * (l * l - mh.y); }
        m.z = len;
    }
    A.out_col[i] = r;
    A.out_mom[i] = m;
}

/* step 3 for pixel (x, y) */
RTD_FN sf_f4 tf_variance_pixel(const TfVar& V, uint32_t x, uint32_t y)
{
    const uint32_t i = y * V.width + x;
    const sf_f4 m = V.mom[i];
    sf_f4 r = V.acc[i];
    r.w = 0.0f;
    if (!(m.z > 0.0f)) return r;
    float m1 = m.x, m2 = m.y;
    if (m.z < TF_MOMENTS_MIN_LEN)
    {
        const sf_f4 gp = V.nz[i];
        float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
        sf_stencil(x, y, V.width, V.height, TF_VAR_RADIUS, 1, [&](int j, int k, uint32_t qi) {
            const sf_f4 mq = V.mom[qi];
            if (!(mq.z > 0.0f)) return;
            const sf_f4 gq = V.nz[qi];
            // sf_depth_term at step 1, written out: through the function, clang splits this kernel's guide loads and it runs ~5 % slower
            float ez = 0.0f;
            if (j != 0 || k != 0)
            {
                const int mm = (j < 0 ? -j : j) > (k < 0 ? -k : k) ? (j < 0 ? -j : j) : (k < 0 ? -k : k);
                ez = __builtin_fabsf(gp.w - gq.w) * V.inv_z / (gp.w * (float)mm);
            }
            const float w = rt_expf(-(sf_normal_term(gp, gq) * V.inv_n + ez));
            sw = sw + w;
            s1 = s1 + w * (mq.x - m.x); s2 = s2 + w * (mq.y - m.y);
        });
        if (sw > 0.0f) { m1 = m.x + s1 / sw; m2 = m.y + s2 / sw; }
    }
    const float var = m2 - m1 * m1;
    r.w = var > 0.0f ? var : 0.0f;
    return r;
}

/* step 4 (step > 0) and, with SF_LAST, step 5 for pixel (x, y) */
RTD_FN sf_f4 tf_pass_pixel(const TfPass& P, uint32_t x, uint32_t y)
{
    const float b[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float g3[3] = {0.25f, 0.5f, 0.25f};
    const uint32_t i = y * P.width + x;
    const int valid = P.mom[i].z > 0.0f;
    const sf_f4 cp = P.col[i];
    sf_f4 r = cp;
    int own = 0;                                                 // the result is c_p itself
    if (P.step == 0) own = cp.w != 0.0f;
    else if (valid)
    {
        float gw = 0.0f, gs = 0.0f;
        sf_stencil(x, y, P.width, P.height, 1, 1, [&](int j, int k, uint32_t qi) {
            if (!(P.mom[qi].z > 0.0f)) return;
            const float kw = g3[j + 1] * g3[k + 1];
            gw = gw + kw;
            gs = gs + kw * P.col[qi].w;
        });
        const float den = P.sigma_l * __builtin_sqrtf(gs / gw) + TF_LUM_EPS;
        const float lp = tf_lum(cp);
        const sf_f4 gp = P.nz[i];
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
        const int s = (int)P.step;
        sf_stencil(x, y, P.width, P.height, 2, s, [&](int j, int k, uint32_t qi) {
            if (!(P.mom[qi].z > 0.0f)) return;
            const sf_f4 cq = P.col[qi];
            const sf_f4 gq = P.nz[qi];
            const float e = __builtin_fabsf(lp - tf_lum(cq)) / den + sf_normal_term(gp, gq) * P.inv_n + sf_depth_term(gp, gq, P.inv_z, s, j, k);
            const float w = b[j + 2] * b[k + 2] * rt_expf(-e);
            sw = sw + w;
            sx = sx + w * (cq.x - cp.x); sy = sy + w * (cq.y - cp.y); sz = sz + w * (cq.z - cp.z);
            sv = sv + (w * w) * cq.w;
        });
        if (sw > 0.0f) { r.x = cp.x + sx / sw; r.y = cp.y + sy / sw; r.z = cp.z + sz / sw; r.w = sv / (sw * sw); }
    }
    if (P.hist)
    {
        sf_f4 h = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) { h.x = r.x; h.y = r.y; h.z = r.z; }
        P.hist[i] = h;
    }
    if (P.flags & SF_LAST)
    {
        if (!valid || own || !sf_finite3(r)) r = sf_h(P.src, P.flags, P.spp, i);       // h_p exactly
        else if (P.flags & SF_DEMOD) r = sf_remodulate(r, P.alb[i]);
        if (P.flags & SF_TONEMAP) r = sf_reinhard(r);
        r.w = 1.0f;
    }
    return r;
}

#endif /* RT_TEMPORAL_FILTER_H */
