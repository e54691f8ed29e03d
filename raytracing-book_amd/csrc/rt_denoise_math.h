// rt_denoise_math.h — the arithmetic of the variance-guided a-trous preview filter (rt.h rt_denoise),
// in RT_HD functions that the kernels (rt_denoise.hip) and the host reference (rt_denoise_host.cpp)
// both include, so the two give the same bits: f32, no contraction, only + - * / sqrtf fabsf and
// g_max.  This file fixes the order of every operation; rt.h states the definition.
//
// A pixel of a level is {r, g, b, V}.  A bad pixel (y or M2.w of the input not finite) carries
// V = -1: a good pixel's V is never negative (level 0 clamps it at +0, every later level is a sum
// of non-negative terms over a positive divisor), so `V < 0` is the bad flag.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>

#include "rt/rt_glsl.h"

struct alignas(16) rt_dn4 { float x, y, z, w; };

#define RT_DN_H0 0.140625f   /* 9/64 = h[0] * h[0], the centre tap's weight */

RT_HD int dn_finite(float v) { return fabsf(v) <= FLT_MAX; }
RT_HD float dn_lum(const rt_dn4 c) { return (c.x + c.y) + c.z; }
RT_HD int dn_bad(const rt_dn4 c) { return c.w < 0.0f; }
// h = (1/16, 1/4, 3/8, 1/4, 1/16) for d = -2 .. 2; the 3x3 weights (1, 2, 1) for d = -1 .. 1
RT_HD float dn_h5(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
RT_HD float dn_k3(int d) { return d == 0 ? 2.0f : 1.0f; }
RT_HD int dn_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Level 0: {rgb, V_0 = g_max(0, M2.w / ((float)n * (float)(n - 1)))}, or the bad flag.
RT_HD rt_dn4 dn_level0(const rt_dn4 img, float m2w, int n) {
    rt_dn4 o = img;
    if (!(dn_finite(dn_lum(img)) && dn_finite(m2w))) {
        o.w = -1.0f;
        return o;
    }
    o.w = g_max(0.0f, m2w / ((float)n * (float)(n - 1)));
    return o;
}

// Level 0 over a reprojected view (rt.h rt_denoise_reprojected): R = {r, g, b, n} the view, s2 the
// per-sample variance of y that came with it (< 0 or NaN: unknown), ai the first-hit albedo_id words.
// A pixel is bad when y(R) is not finite or n is not > 0.  Known s2: V_0 = s2 / n.  Otherwise the spread
// of y over the 5x5 taps at spacing 1 (row-major, dy outer, centre included) that lie in the image, are
// not bad and carry p's id word (a skipped tap is read at the clamped position and leaves the sums
// untouched):  cnt = cnt + 1; sy = sy + y(q);  m = sy / cnt;  then e = y(q) - m; sd = sd + e * e over the
// same taps;  V_0 = cnt < 2 ? +0 : (sd / (cnt - 1)) / n.
RT_HD int dn_rp_bad(const rt_dn4 r) { return !(dn_finite(dn_lum(r)) && r.w > 0.0f); }
RT_HD rt_dn4 dn_level0_reprojected(const rt_dn4* __restrict__ rgbn, const float* __restrict__ s2,
                                   const rt_dn4* __restrict__ ai, int W, int H, int x, int y) {
    const size_t p = (size_t)y * W + x;
    const rt_dn4 R = rgbn[p];
    rt_dn4 o = R;
    if (dn_rp_bad(R)) {
        o.w = -1.0f;
        return o;
    }
    const float s = s2[p];
    if (s >= 0.0f && dn_finite(s)) {
        o.w = s / R.w;
        return o;
    }
    const unsigned idp = rt_f2u(ai[p].w);
    float yq[25];
    unsigned ok = 0u;
    float cnt = 0.0f, sy = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int t = (dy + 2) * 5 + (dx + 2);
            const int qx = x + dx, qy = y + dy;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t q = (size_t)dn_clampi(qy, H - 1) * W + dn_clampi(qx, W - 1);
            const rt_dn4 rq = rgbn[q];
            const bool use = in && !dn_rp_bad(rq) && rt_f2u(ai[q].w) == idp;
            yq[t] = dn_lum(rq);
            ok |= use ? 1u << t : 0u;
            cnt = use ? cnt + 1.0f : cnt;
            sy = use ? sy + yq[t] : sy;
        }
    }
    const float m = sy / cnt;
    float sd = 0.0f;
#pragma unroll
    for (int t = 0; t < 25; t++) {
        const float e = yq[t] - m;
        sd = (ok >> t & 1u) ? sd + e * e : sd;
    }
    o.w = cnt < 2.0f ? 0.0f : (sd / (cnt - 1.0f)) / R.w;
    return o;
}

// Vb(p): taps (dy, dx) in {-1, 0, 1}^2 at spacing 1, row-major; for each tap in the image and good
//   acc = acc + (k3[dy] * k3[dx]) * V(q);  ws = ws + k3[dy] * k3[dx];     Vb = acc / ws.
// A skipped tap is read at the clamped position and leaves acc and ws untouched.  Bad p: +0.
RT_HD float dn_vb(const rt_dn4* __restrict__ src, int W, int H, int x, int y) {
    if (src[(size_t)y * W + x].w < 0.0f) return 0.0f;
    float acc = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const float v = src[(size_t)dn_clampi(qy, H - 1) * W + dn_clampi(qx, W - 1)].w;
            const bool use = in && !(v < 0.0f);
            const float w = dn_k3(dy) * dn_k3(dx);
            acc = use ? acc + w * v : acc;
            ws = use ? ws + w : ws;
        }
    }
    return acc / ws;
}

// The guides of rt_denoise_guided (rt.h): the first-hit buffers normal_depth = (N, t) and albedo_id =
// (A, id bits), one float4 each per pixel, and the three strengths.  A pixel is guide-good when its
// N, t and A are all finite; it is a miss when its id word is RT_FEATURE_MISS.
struct rt_dn_guides {
    const rt_dn4* nd;
    const rt_dn4* ai;
    float kn, kz, ka;
};
RT_HD int dn_guide_good(const rt_dn4 nd, const rt_dn4 ai) {
    return dn_finite(nd.x) && dn_finite(nd.y) && dn_finite(nd.z) && dn_finite(nd.w) && dn_finite(ai.x) &&
           dn_finite(ai.y) && dn_finite(ai.z);
}
RT_HD int dn_guide_hit(const rt_dn4 ai) { return rt_f2u(ai.w) != 0xFFFFFFFFu; }
// The guide factor g of tap q of pixel p (rt.h): 1 when either is not guide-good, 0 across a hit / miss
// boundary, else (gn * gz) * ga, a term whose k is exactly 0 being exactly 1 and gn, gz being 1 between
// two misses.
RT_HD float dn_guide_weight(const rt_dn4 ndp, const rt_dn4 aip, const rt_dn4 ndq, const rt_dn4 aiq, float kn, float kz,
                            float ka) {
    if (!(dn_guide_good(ndp, aip) && dn_guide_good(ndq, aiq))) return 1.0f;
    const int hp = dn_guide_hit(aip), hq = dn_guide_hit(aiq);
    if (hp != hq) return 0.0f;
    float gn = 1.0f, gz = 1.0f, ga = 1.0f;
    if (hp && kn != 0.0f) gn = g_max(0.0f, 1.0f - kn * (1.0f - ((ndp.x * ndq.x + ndp.y * ndq.y) + ndp.z * ndq.z)));
    if (hp && kz != 0.0f) gz = g_max(0.0f, 1.0f - kz * (fabsf(ndp.w - ndq.w) / (g_max(ndp.w, ndq.w) + 1e-30f)));
    if (ka != 0.0f)
        ga = g_max(0.0f, 1.0f - ka * ((fabsf(aip.x - aiq.x) + fabsf(aip.y - aiq.y)) + fabsf(aip.z - aiq.z)));
    return (gn * gz) * ga;
}

// One level at p with step s: taps (dy, dx) in {-2 .. 2}^2 row-major, q = p + s * (dx, dy), the
// centre and taps outside the image or bad skipped (read at the clamped position, sums untouched):
//   d  = fabsf(y(p) - y(q)) / (k * sqrtf(Vb(p) + Vb(q)) + 1e-30f)
//   w  = (h[dy] * h[dx]) * g_max(0, 1 - d)            (GUIDED: that times dn_guide_weight(p, q))
//   sw = sw + w;  sc = sc + w * (C(q) - C(p)) per channel;  sv = sv + (w * w) * V(q)
// then den = h0 + sw,  C' = C(p) + sc / den,  V' = ((h0 * h0) * V(p) + sv) / (den * den).
// A bad p is returned as it is.  GUIDED = false compiles to rt_denoise's filter as it was.
template <bool GUIDED>
RT_HD rt_dn4 dn_filter_t(const rt_dn4* __restrict__ src, const float* __restrict__ vb, int W, int H, int x, int y, int s,
                         float k, const rt_dn_guides& G) {
    const size_t p = (size_t)y * W + x;
    const rt_dn4 cp = src[p];
    if (dn_bad(cp)) return cp;
    const float yp = dn_lum(cp), vbp = vb[p];
    rt_dn4 ndp = cp, aip = cp;
    if (GUIDED) {
        ndp = G.nd[p];
        aip = G.ai[p];
    }
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + s * dx, qy = y + s * dy;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t q = (size_t)dn_clampi(qy, H - 1) * W + dn_clampi(qx, W - 1);
            const rt_dn4 cq = src[q];
            const float vbq = vb[q];
            const bool use = in && !dn_bad(cq);
            const float d = fabsf(yp - dn_lum(cq)) / (k * sqrtf(vbp + vbq) + 1e-30f);
            float w = (dn_h5(dy) * dn_h5(dx)) * g_max(0.0f, 1.0f - d);
            if (GUIDED) w = w * dn_guide_weight(ndp, aip, G.nd[q], G.ai[q], G.kn, G.kz, G.ka);
            sw = use ? sw + w : sw;
            sr = use ? sr + w * (cq.x - cp.x) : sr;
            sg = use ? sg + w * (cq.y - cp.y) : sg;
            sb = use ? sb + w * (cq.z - cp.z) : sb;
            sv = use ? sv + (w * w) * cq.w : sv;
        }
    }
    const float den = RT_DN_H0 + sw;
    rt_dn4 o;
    o.x = cp.x + sr / den;
    o.y = cp.y + sg / den;
    o.z = cp.z + sb / den;
    o.w = ((RT_DN_H0 * RT_DN_H0) * cp.w + sv) / (den * den);
    return o;
}
RT_HD rt_dn4 dn_filter(const rt_dn4* __restrict__ src, const float* __restrict__ vb, int W, int H, int x, int y, int s,
                       float k) {
    const rt_dn_guides none = {nullptr, nullptr, 0.0f, 0.0f, 0.0f};
    return dn_filter_t<false>(src, vb, W, H, x, y, s, k, none);
}
RT_HD rt_dn4 dn_filter_guided(const rt_dn4* __restrict__ src, const float* __restrict__ vb, int W, int H, int x, int y,
                              int s, float k, const rt_dn_guides& G) {
    return dn_filter_t<true>(src, vb, W, H, x, y, s, k, G);
}

// The filter's parameters after defaults and checks (rt_denoise_host.cpp rt_denoise_resolve).
struct rt_dn_resolved { int levels; float k; };
// The guide strengths after defaults and checks (rt_denoise_host.cpp guide_resolve).
struct rt_guide_resolved { float kn, kz, ka; };
// With all three strengths exactly 0 no guide applies at all (g = 1 on every tap, the hit / miss rule
// included): the filter is rt_denoise's, bit for bit.
RT_HD int dn_guides_on(const rt_guide_resolved g) { return g.kn != 0.0f || g.ka != 0.0f || g.kz != 0.0f; }
