// rt_denoise.h — what the preview filter's units share with the rest of the C ABI (rt_denoise.hip,
// rt_denoise_host.cpp, rt_features.hip, rt_capi.hip).  Internal to the libraries; no device header needed.
#pragma once

#include "rt/rt.h"

struct rt_dn_resolved;
struct rt_guide_resolved;

namespace rt_impl __attribute__((visibility("hidden"))) {

// params (NULL = defaults) checked and resolved; RT_OK or RT_ERR_INVALID_ARG
int denoise_resolve(const rt_denoise_params* p, rt_dn_resolved* out);
// the guide strengths likewise (NULL = RT_GUIDE_DEFAULT_*)
int guide_resolve(const rt_guide_params* p, rt_guide_resolved* out);
// rt_resize, rt_set_moments(0), rt_destroy: the filter's buffers freed, no result held
// (the caller has made the device current and its stream idle)
void denoise_free(rt_ctx* c);
// rt_resize, rt_destroy: the first-hit buffers and the pass's own link and argument copies freed
// (rt_features.hip; the same precondition)
void features_free(rt_ctx* c);

}  // namespace rt_impl
