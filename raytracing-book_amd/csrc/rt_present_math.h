// rt_present_math.h — the arithmetic of the presented frame (rt.h rt_present), in RT_HD functions that the
// kernel (rt_present.hip) and the host function (rt_present_host.cpp) both include, so the two give the
// same bits: f32, no contraction, one multiplication per channel, rintf (round half to even) and
// comparisons.  This file fixes the order of every operation; rt.h states the definition.
//
// The gamma table is not computed here: it is rt_gamma_lut.h's, built on the host, and reaches these
// functions as 256 bytes (host memory, a device buffer or LDS).
#pragma once

#include <math.h>
#include <stdint.h>

#include "rt/rt_glsl.h"
#include "rt_denoise_math.h"   // rt_dn4

// The colour to show and the float copy's w.  MOVED: the filtered buffer D where the reprojected word's
// count did not grow over the tile's (a NaN count is fresh), the reprojected view R elsewhere.
RT_HD rt_dn4 pr_moved(const rt_dn4 R, const rt_dn4 D, int count) {
    const float n_t = (float)count;
    const bool fresh = !(R.w > n_t);
    rt_dn4 o = fresh ? D : R;
    o.w = fresh ? 1.0f : 0.0f;
    return o;
}

// e.c = c.c * exposure (1.0f keeps every finite value's bits and a NaN a NaN); w passes through
RT_HD rt_dn4 pr_expose(const rt_dn4 c, float exposure) {
    rt_dn4 e;
    e.x = c.x * exposure;
    e.y = c.y * exposure;
    e.z = c.z * exposure;
    e.w = c.w;
    return e;
}

// glGetTexImage's float -> unorm8 (image_io.cpp unorm8): NaN and <= 0 -> 0, >= 1 -> 255, else round to
// nearest, ties to even
RT_HD int pr_code(float f) {
    if (!(f > 0.0f)) return 0;
    if (f >= 1.0f) return 255;
    return (int)rintf(f * 255.0f);
}

// the pixel's word: r | g << 8 | b << 16 | 0xFF << 24, each byte the table's entry of the channel's code
RT_HD uint32_t pr_pack(const rt_dn4 e, const uint8_t* lut) {
    const uint32_t r = lut[pr_code(e.x)], g = lut[pr_code(e.y)], b = lut[pr_code(e.z)];
    return r | (g << 8) | (b << 16) | (0xFFu << 24);
}
