// rt_refine.h — what the reach records' units share with the rest of the C ABI (rt_refine.hip,
// rt_refine_host.cpp, rt_capi.hip, rt_present.hip).  Internal to the libraries; no device header needed.
#pragma once

#include "rt/rt.h"

// rt_refine_params checked and resolved (min_count 0 = automatic, min_pixels 0 = 1)
struct rt_rf_resolved {
    float min_count;
    int extra_frames, min_pixels, max_tiles;
};

// rt_noise_refine_params checked and resolved (min_count 0 = automatic, 2)
struct rt_nz_resolved {
    float target_noise, min_count;
    int batch_frames, max_rounds;
};

namespace rt_impl __attribute__((visibility("hidden"))) {

// RT_OK, or RT_ERR_INVALID_ARG: a target_noise or min_count that is negative or not finite, batch_frames < 1,
// max_rounds < 0, reserved not 0
int noise_refine_resolve(const rt_noise_refine_params* p, rt_nz_resolved* out);
// RT_OK, or RT_ERR_INVALID_ARG: extra_frames < 0, min_pixels outside 0 .. 64, max_tiles < 0, a min_count that
// is negative or not finite, reserved not 0
int refine_resolve(const rt_refine_params* p, rt_rf_resolved* out);
// rt_resize, rt_destroy: the record buffer freed, no records held (the caller has made the device current
// and its stream idle)
void refine_free(rt_ctx* c);
// rt_render_moved's steps 1-5 and its steps 6-7 (rt_present.hip), which rt_render_moved_refined runs around
// its own
int moved_to_reprojected(rt_ctx* c, const float camera[28], int n_frames, const float* rand_factors,
                         const rt_reproject_params* reproject);
int moved_filter_present(rt_ctx* c, const rt_denoise_params* denoise, const rt_guide_params* guides,
                         const rt_present_params* present);

}  // namespace rt_impl
