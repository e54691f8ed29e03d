// rt_refine_math.h — the arithmetic of the per-tile reach record (rt.h rt_reach_tiles), in RT_HD functions that
// the kernel (rt_refine.hip) and the host function (rt_refine_host.cpp) both include, so the two give the same
// bits: f32, no contraction, only +, comparisons, fabsf and g_min.  This file fixes what a lane contributes
// and how two partial results combine; the order of the combination is the xor butterfly (32, 16, 8, 4, 2, 1)
// over lanes ty * 8 + tx, which the kernel runs with shuffles and the host function over a 64-entry array.
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
