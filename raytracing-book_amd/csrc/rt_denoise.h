// rt_denoise.h — what the preview filter's units share with the rest of the C ABI (rt_denoise.hip,
// rt_denoise_host.cpp, rt_capi.hip).  Internal to the libraries; no device header needed.
#pragma once

#include "rt/rt.h"

struct rt_dn_resolved;

namespace rt_impl __attribute__((visibility("hidden"))) {

// params (NULL = defaults) checked and resolved; RT_OK or RT_ERR_INVALID_ARG
int denoise_resolve(const rt_denoise_params* p, rt_dn_resolved* out);
// rt_resize, rt_set_moments(0), rt_destroy: the filter's buffers freed, no result held
// (the caller has made the device current and its stream idle)
void denoise_free(rt_ctx* c);

}  // namespace rt_impl
