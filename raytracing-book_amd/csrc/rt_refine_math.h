// rt_refine_math.h — the arithmetic of the per-tile reach record (rt.h rt_reach_tiles), in RT_HD functions that
// the kernel (rt_refine.hip) and the host function (rt_refine_host.cpp) both include, so the two give the same
// bits: f32, no contraction, only +, comparisons, fabsf and g_min.  This file fixes what a lane contributes
// and how two partial results combine; the order of the combination is the xor butterfly (32, 16, 8, 4, 2, 1)
// over lanes ty * 8 + tx, which the kernel runs with shuffles and the host function over a 64-entry array.
// The noise record (rt.h rt_noise_tiles) follows the same plan with its own lane function below.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rt/rt_glsl.h"
#include "rt_denoise_math.h"   // dn_finite

// what the pixel's count n gives its tile; in: the lane's pixel lies in the image
struct rf_lane {
    float v_min, v_sum;
    int is_short;
};

RT_HD rf_lane rf_lane_of(int in, float n, float min_count) {
    const int good = in && n > 0.0f && dn_finite(n);   // a NaN is not good
    rf_lane l;
    l.v_min = good ? n : INFINITY;
    l.v_sum = good ? n : 0.0f;
    l.is_short = in && !(n >= min_count);   // a NaN and a count of 0 are short
    return l;
}

// one butterfly step: the lane's value with its partner's (lane ^ off)
RT_HD float rf_sum_step(float mine, float other) { return mine + other; }
RT_HD float rf_min_step(float mine, float other) { return g_min(mine, other); }

// min_count > 0 and finite
RT_HD int rf_min_count_ok(float min_count) { return min_count > 0.0f && dn_finite(min_count); }

// The noise record (rt.h rt_noise_tiles): what the pixel's reprojected word (r, g, b, n) and its variance word s2
// give its tile; f32, no contraction, only +, /, comparisons and fabsf.  The butterfly's step is rf_sum_step.
struct rf_noise_lane {
    float v, yv;
    int known, thin, bad;
};

RT_HD rf_noise_lane rf_noise_lane_of(int in, float r, float g, float b, float n, float s2, float min_count) {
    const float y = (r + g) + b;
    const int good = in && dn_finite(y) && n > 0.0f && dn_finite(n);
    const int known = good && s2 >= 0.0f && dn_finite(s2);
    rf_noise_lane l;
    l.known = known;
    l.thin = good && (!known || !(n >= min_count));
    l.bad = in && !good;
    l.v = known ? s2 / n : 0.0f;   // the variance of the pixel's mean
    l.yv = good ? y : 0.0f;
    return l;
}
