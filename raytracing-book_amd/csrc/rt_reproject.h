// rt_reproject.h — what temporal reprojection's units share with the rest of the C ABI (rt_reproject.hip,
// rt_reproject_host.cpp, rt_capi.hip).  Internal to the libraries; no device header needed.
#pragma once

#include "rt/rt.h"
#include "rt/rt_types.h"

struct rt_rp_resolved;

namespace rt_impl __attribute__((visibility("hidden"))) {

// params (NULL = RT_REPROJECT_DEFAULT_*) checked and resolved; RT_OK or RT_ERR_INVALID_ARG
int reproject_resolve(const rt_reproject_params* p, rt_rp_resolved* out);
// the history view's matrix M of rt.h from its camera block; RT_ERR_INVALID_ARG if det is 0 or not finite
int reproject_matrix(const rt_camera_ubo& cam, float M[9]);
// rt_upload_buffer, rt_upload_texture: the history is dropped (its ids meant another scene's surfaces);
// the buffers stay for the next capture
void history_drop(rt_ctx* c);
// rt_resize, rt_destroy: the history, the result and the count copy freed, none held
// (the caller has made the device current and its stream idle)
void reproject_free(rt_ctx* c);

}  // namespace rt_impl
