// rt_present.h — what the presented frame's units share with the rest of the C ABI (rt_present.hip,
// rt_present_host.cpp, rt_capi.hip).  Internal to the libraries; no device header needed.
#pragma once

#include "rt/rt.h"

// rt_present_params checked and resolved (NULL = RT_PRESENT_IMAGE, exposure 1, no float copy)
struct rt_pr_resolved {
    int source;
    float exposure;
    bool keep_float;
};

namespace rt_impl __attribute__((visibility("hidden"))) {

// RT_OK, or RT_ERR_INVALID_ARG: a source that is none of the four, an exposure that is not finite and > 0,
// reserved not 0
int present_resolve(const rt_present_params* p, rt_pr_resolved* out);
// rt_resize, rt_destroy: the presented buffers and the table's copy freed, nothing held, a bound buffer let go
// (the caller has made the device current and its stream idle)
void present_free(rt_ctx* c);

}  // namespace rt_impl
