// rt_reproject_math.h — the arithmetic of temporal reprojection (rt.h rt_reproject), in RT_HD functions
// that the kernel (rt_reproject.hip) and the host reference (rt_reproject_host.cpp) both include, so the
// two give the same bits: f32, no contraction, only + - * / fabsf floorf g_max g_min and comparisons.
// This file fixes the order of every operation; rt.h states the definition.
//
// A pixel of the history and of the result is {r, g, b, n}: the mean and the frames behind it.
#pragma once

#include "rt/rt_types.h"
#include "rt_denoise_math.h"   // rt_dn4, dn_finite, dn_guide_good, dn_guide_hit, dn_clampi

// What one rt_reproject call works with beside the buffers: the current and the history camera block,
// the history view's matrix M (rows a, b, c: rt.h) and the resolved parameters.
struct rt_rp_view {
    rt_camera_ubo cam, cam_h;
    float M[9];
    float cos_min, kz, max_history;
    int W, H;
};

RT_HD float rp_dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// rt_features.hip's pixel_base: (up_left + pixel_delta_u * fx) + pixel_delta_v * fy, per component
RT_HD v3 rp_pixel_base(const rt_camera_ubo& C, float fx, float fy) {
    return add3(add3(ld3(C.up_left), scale3(ld3(C.pixel_delta_u), fx)), scale3(ld3(C.pixel_delta_v), fy));
}
RT_HD int rp_rgb_finite(const rt_dn4 c) { return dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z); }

// rt_history_capture from the image: {rgb, n = (float)count}, n = 0 where a component of rgb is not finite.
RT_HD rt_dn4 rp_history_pixel(const rt_dn4 img, int count) {
    rt_dn4 o = img;
    o.w = rp_rgb_finite(img) ? (float)count : 0.0f;
    return o;
}

// The per-sample variance of y = (r + g) + b that travels with the history (rt.h rt_set_history_variance):
// g_max(0, M2.w / (n - 1)) with rp_history_pixel's n, or -1 = unknown (fewer than two frames, M2.w not
// finite).  Every "known" test is written `s2 >= 0`, so a NaN is unknown.
RT_HD float rp_history_s2(const rt_dn4 img, float m2w, int count) {
    const float n = rp_rgb_finite(img) ? (float)count : 0.0f;
    if (n >= 2.0f && dn_finite(m2w)) return g_max(0.0f, m2w / (n - 1.0f));
    return -1.0f;
}

// The result at current pixel (x, y): img its image word, count its tile's frame count, nd / ai its
// first-hit words; hc / hnd / hai the history's {r, g, b, n} and first-hit buffers (V.W x V.H each).
// VAR: the variance is carried too (m2w the pixel's M2.w, hs2 the history's s2, one float per pixel; the
// result's s2 goes to *s2_out).  The {r, g, b, n_out} word comes out of the same operations either way;
// VAR = false compiles to rt_reproject as it was and touches none of the three.
// MISS (rt.h rt_set_reproject_misses): a guide-good pixel whose centre ray hits nothing is reprojected by
// its direction (steps 2m and 4m); a hit pixel's operations are the same under either value, and
// MISS = false compiles to the code as it was.
template <bool VAR, bool MISS = false>
RT_HD rt_dn4 rp_pixel_t(const rt_dn4 img, int count, const rt_dn4 nd, const rt_dn4 ai, const rt_dn4* __restrict__ hc,
                        const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai, const rt_rp_view& V, int x, int y,
                        float m2w, const float* __restrict__ hs2, float* __restrict__ s2_out) {
    const int W = V.W, H = V.H;
    rt_dn4 out = img;
    const float n_c = rp_rgb_finite(img) ? (float)count : 0.0f;
    out.w = n_c;
    float s2_c = -1.0f;
    if (VAR) {
        s2_c = rp_history_s2(img, m2w, count);
        *s2_out = s2_c;   // what every `return out` below leaves: not reprojected, or rejected
    }
    // 1. first-hit words that are not finite, or (without MISS) a miss: nothing to reproject
    if (!dn_guide_good(nd, ai)) return out;
    const bool hit = dn_guide_hit(ai);
    if (!MISS && !hit) return out;
    // 2. the world point the pixel's centre ray lands on
    const v3 o = ld3(V.cam.camera_pos), o_h = ld3(V.cam_h.camera_pos);
    const v3 d = sub3(rp_pixel_base(V.cam, (float)x, (float)y), o);
    v3 w = d;   // 2m. a miss: the direction itself stands for the point at infinity
    if (!MISS || hit) {
        const v3 P = mk3(o.x + d.x * nd.w, o.y + d.y * nd.w, o.z + d.z * nd.w);
        // 3. into the history view
        w = sub3(P, o_h);
    }
    const float a = (V.M[0] * w.x + V.M[1] * w.y) + V.M[2] * w.z;
    const float b = (V.M[3] * w.x + V.M[4] * w.y) + V.M[5] * w.z;
    const float c = (V.M[6] * w.x + V.M[7] * w.y) + V.M[8] * w.z;
    if (!(c > 0.0f)) return out;
    const float fx = a / c, fy = b / c;
    if (!(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H)) return out;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float ax = fx - x0, ay = fy - y0;
    const int ix = (int)x0, iy = (int)y0;   // -1 .. W - 1, -1 .. H - 1
    // 4. the four taps
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
    float ss = 0.0f, sws = 0.0f;   // VAR: the taps whose s2 is known, and their weights
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = ix + i, qy = iy + j;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const int cx = dn_clampi(qx, W - 1), cy = dn_clampi(qy, H - 1);
            const size_t q = (size_t)cy * W + cx;
            const rt_dn4 hq = hc[q], ndq = hnd[q], aiq = hai[q];
            const float u = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            bool use = in && hq.w > 0.0f && dn_guide_good(ndq, aiq);
            if (!MISS || hit) {
                use = use && dn_guide_hit(aiq) && rt_f2u(aiq.w) == rt_f2u(ai.w);
                use = use && (nd.x * ndq.x + nd.y * ndq.y) + nd.z * ndq.z >= V.cos_min;
                if (V.kz != 0.0f) {
                    const v3 dq = sub3(rp_pixel_base(V.cam_h, (float)cx, (float)cy), o_h);
                    const float t_exp = rp_dot(w, dq) / rp_dot(dq, dq);
                    use = use && fabsf(t_exp - ndq.w) <= V.kz * t_exp;
                }
            } else {
                // 4m. a miss tap under p's background: the miss's id test; no cos_min and no kz test
                use = use && !dn_guide_hit(aiq) && rt_f2u(aiq.x) == rt_f2u(ai.x) && rt_f2u(aiq.y) == rt_f2u(ai.y) &&
                      rt_f2u(aiq.z) == rt_f2u(ai.z);
            }
            sw = use ? sw + u : sw;
            sr = use ? sr + u * hq.x : sr;
            sg = use ? sg + u * hq.y : sg;
            sb = use ? sb + u * hq.z : sb;
            sn = use ? sn + u * hq.w : sn;
            if (VAR) {
                const float s = hs2[q];
                const bool kn = use && s >= 0.0f;
                ss = kn ? ss + u * s : ss;
                sws = kn ? sws + u : sws;
            }
        }
    }
    // 5. the history estimate
    if (!(sw > 0.0f)) return out;
    const float hr = sr / sw, hg = sg / sw, hb = sb / sw;
    const float n_hist = g_min(sn / sw, V.max_history);
    float s2_hist = -1.0f;
    if (VAR) s2_hist = sws > 0.0f ? ss / sws : -1.0f;
    // 6. blended with the pixel's own frames by the counts
    if (n_c == 0.0f) {
        out.x = hr;
        out.y = hg;
        out.z = hb;
        out.w = n_hist;
        if (VAR) *s2_out = s2_hist;
        return out;
    }
    const float n_out = n_c + n_hist, alpha = n_hist / n_out;
    out.x = img.x + alpha * (hr - img.x);
    out.y = img.y + alpha * (hg - img.y);
    out.z = img.z + alpha * (hb - img.z);
    out.w = n_out;
    if (VAR) {
        // s2 blends like a colour channel: the count-weighted mean of the two per-sample variances
        if (!(s2_c >= 0.0f)) *s2_out = s2_hist;
        else if (!(s2_hist >= 0.0f)) *s2_out = s2_c;
        else *s2_out = s2_c + alpha * (s2_hist - s2_c);
    }
    return out;
}
RT_HD rt_dn4 rp_pixel(const rt_dn4 img, int count, const rt_dn4 nd, const rt_dn4 ai, const rt_dn4* __restrict__ hc,
                      const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai, const rt_rp_view& V, int x, int y) {
    return rp_pixel_t<false>(img, count, nd, ai, hc, hnd, hai, V, x, y, 0.0f, nullptr, nullptr);
}
RT_HD rt_dn4 rp_pixel_var(const rt_dn4 img, int count, const rt_dn4 nd, const rt_dn4 ai, const rt_dn4* __restrict__ hc,
                          const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai, const rt_rp_view& V, int x, int y,
                          float m2w, const float* __restrict__ hs2, float* __restrict__ s2_out) {
    return rp_pixel_t<true>(img, count, nd, ai, hc, hnd, hai, V, x, y, m2w, hs2, s2_out);
}
// ... and with the misses reprojected by direction (rt_set_reproject_misses)
RT_HD rt_dn4 rp_pixel_miss(const rt_dn4 img, int count, const rt_dn4 nd, const rt_dn4 ai, const rt_dn4* __restrict__ hc,
                           const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai, const rt_rp_view& V, int x, int y) {
    return rp_pixel_t<false, true>(img, count, nd, ai, hc, hnd, hai, V, x, y, 0.0f, nullptr, nullptr);
}
RT_HD rt_dn4 rp_pixel_miss_var(const rt_dn4 img, int count, const rt_dn4 nd, const rt_dn4 ai, const rt_dn4* __restrict__ hc,
                               const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai, const rt_rp_view& V, int x, int y,
                               float m2w, const float* __restrict__ hs2, float* __restrict__ s2_out) {
    return rp_pixel_t<true, true>(img, count, nd, ai, hc, hnd, hai, V, x, y, m2w, hs2, s2_out);
}

// The parameters after defaults and checks (rt_reproject_host.cpp reproject_resolve).
struct rt_rp_resolved { float cos_min, kz, max_history; };
