// rt_reproject.hip — temporal reprojection (rt.h rt_history_capture / rt_reproject / rt_read_reprojected):
// what the image had accumulated before a camera move, gathered into the new view.  Nothing here touches
// the render kernels, the image, the moments, the counts, the features or the filter's buffers: the
// history and the result are buffers of their own.
//
// reproject_kernel: one lane per pixel, a wave = one 8x8 tile (features_kernel's tile), four tiles per
// workgroup; no LDS, no atomics.  A tile's world points land in a compact patch of the history view, so
// a wave's four-tap gathers (three float4 buffers) fall into a few neighbouring rows of each; the caches
// serve the overlap between lanes.  Per pixel it reads 3 float4 of its own and up to 12 of the history
// and writes one.  The camera blocks, M and the parameters travel by value in the kernel arguments.  The
// arithmetic is rt_reproject_math.h's, shared with rt_reproject_host, which the result equals bit for bit.
// history_kernel builds the history's {r, g, b, n} from the image and the per-tile counts; the first-hit
// buffers are copied device to device.
//
// rt_set_history_variance(ctx, 1) switches both calls to instantiations of their own, history_var_kernel and
// reproject_var_kernel, which carry the per-sample variance s2 of y beside the pixel: one more float read
// per pixel (M2.w) and per tap (the history's s2, in the cache line of a neighbouring lane's), one more
// written.  With the switch off the two kernels above are the ones launched, with nothing else allocated.
//
// rt_set_reproject_misses(ctx, 1) switches rt_reproject to reproject_miss_kernel / reproject_miss_var_kernel, the
// same body with rp_pixel_t's MISS on: a pixel that hits nothing is gathered by its ray's direction from the
// history's misses under the same background.  Off, the kernels above run as they always did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rt/rt.h"
#include "rt_ctx.h"
#include "rt_reproject.h"
#include "rt_reproject_math.h"

namespace {

static_assert(sizeof(rt_dn4) == sizeof(float4), "a history pixel is one float4");

constexpr int kTilesPerBlock = 4;   // 256 threads: four waves, one 8x8 tile each

// the lane's pixel and its tile, or false for a lane outside the image (partial tiles)
__device__ __forceinline__ bool tile_pixel(int W, int H, int& x, int& y, int& tile) {
    const int tiles_x = (W + 7) >> 3, n_tiles = tiles_x * ((H + 7) >> 3);
    tile = (int)blockIdx.x * kTilesPerBlock + (int)(threadIdx.x >> 6);
    if (tile >= n_tiles) return false;
    const int lane = (int)(threadIdx.x & 63u);
    x = (tile % tiles_x) * 8 + (lane & 7);
    y = (tile / tiles_x) * 8 + (lane >> 3);
    return x < W && y < H;
}

__global__ void __launch_bounds__(256) history_kernel(const rt_dn4* __restrict__ image, const int32_t* __restrict__ counts,
                                                      int W, int H, rt_dn4* __restrict__ dst) {
    int x, y, tile;
    if (!tile_pixel(W, H, x, y, tile)) return;
    const size_t p = (size_t)y * W + x;
    dst[p] = rp_history_pixel(image[p], counts[tile]);
}

__global__ void __launch_bounds__(256) reproject_kernel(const rt_dn4* __restrict__ image, const int32_t* __restrict__ counts,
                                                        const rt_dn4* __restrict__ nd, const rt_dn4* __restrict__ ai,
                                                        const rt_dn4* __restrict__ hc, const rt_dn4* __restrict__ hnd,
                                                        const rt_dn4* __restrict__ hai, rt_rp_view V,
                                                        rt_dn4* __restrict__ dst) {
    int x, y, tile;
    if (!tile_pixel(V.W, V.H, x, y, tile)) return;
    const size_t p = (size_t)y * V.W + x;
    dst[p] = rp_pixel(image[p], counts[tile], nd[p], ai[p], hc, hnd, hai, V, x, y);
}

// rt_set_history_variance: the history's pixel and its s2 from the image, M2.w and the counts
__global__ void __launch_bounds__(256) history_var_kernel(const rt_dn4* __restrict__ image, const rt_dn4* __restrict__ moments,
                                                          const int32_t* __restrict__ counts, int W, int H,
                                                          rt_dn4* __restrict__ dst, float* __restrict__ dst_s2) {
    int x, y, tile;
    if (!tile_pixel(W, H, x, y, tile)) return;
    const size_t p = (size_t)y * W + x;
    const rt_dn4 img = image[p];
    const int n = counts[tile];
    dst[p] = rp_history_pixel(img, n);
    dst_s2[p] = rp_history_s2(img, moments[p].w, n);
}

// ... and the gather that carries it: reproject_kernel's operations for the result word, s2 beside it
__global__ void __launch_bounds__(256) reproject_var_kernel(const rt_dn4* __restrict__ image, const rt_dn4* __restrict__ moments,
                                                            const int32_t* __restrict__ counts, const rt_dn4* __restrict__ nd,
                                                            const rt_dn4* __restrict__ ai, const rt_dn4* __restrict__ hc,
                                                            const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai,
                                                            const float* __restrict__ hs2, rt_rp_view V,
                                                            rt_dn4* __restrict__ dst, float* __restrict__ dst_s2) {
    int x, y, tile;
    if (!tile_pixel(V.W, V.H, x, y, tile)) return;
    const size_t p = (size_t)y * V.W + x;
    float s2;
    dst[p] = rp_pixel_var(image[p], counts[tile], nd[p], ai[p], hc, hnd, hai, V, x, y, moments[p].w, hs2, &s2);
    dst_s2[p] = s2;
}

// rt_set_reproject_misses: the two gathers above with the misses reprojected by direction.  The same launch
// shape and the same reads; a miss lane skips the point and the depth test and compares the background's bits.
__global__ void __launch_bounds__(256) reproject_miss_kernel(const rt_dn4* __restrict__ image, const int32_t* __restrict__ counts,
                                                             const rt_dn4* __restrict__ nd, const rt_dn4* __restrict__ ai,
                                                             const rt_dn4* __restrict__ hc, const rt_dn4* __restrict__ hnd,
                                                             const rt_dn4* __restrict__ hai, rt_rp_view V,
                                                             rt_dn4* __restrict__ dst) {
    int x, y, tile;
    if (!tile_pixel(V.W, V.H, x, y, tile)) return;
    const size_t p = (size_t)y * V.W + x;
    dst[p] = rp_pixel_miss(image[p], counts[tile], nd[p], ai[p], hc, hnd, hai, V, x, y);
}

__global__ void __launch_bounds__(256) reproject_miss_var_kernel(const rt_dn4* __restrict__ image, const rt_dn4* __restrict__ moments,
                                                                 const int32_t* __restrict__ counts, const rt_dn4* __restrict__ nd,
                                                                 const rt_dn4* __restrict__ ai, const rt_dn4* __restrict__ hc,
                                                                 const rt_dn4* __restrict__ hnd, const rt_dn4* __restrict__ hai,
                                                                 const float* __restrict__ hs2, rt_rp_view V,
                                                                 rt_dn4* __restrict__ dst, float* __restrict__ dst_s2) {
    int x, y, tile;
    if (!tile_pixel(V.W, V.H, x, y, tile)) return;
    const size_t p = (size_t)y * V.W + x;
    float s2;
    dst[p] = rp_pixel_miss_var(image[p], counts[tile], nd[p], ai[p], hc, hnd, hai, V, x, y, moments[p].w, hs2, &s2);
    dst_s2[p] = s2;
}

}  // namespace

namespace rt_impl {

void history_drop(rt_ctx* c) { c->hs_valid = false; }

void reproject_free(rt_ctx* c) {
    for (Device& d : c->devs) {
        dev_free(d.hs_px);
        dev_free(d.hs_nd);
        dev_free(d.hs_ai);
        dev_free(d.rp_out);
        dev_free(d.rp_counts);
        dev_free(d.hs_s2);
        dev_free(d.rp_s2);
    }
    c->rp_counts.clear();
    c->hs_valid = c->rp_valid = false;
    c->hs_w = c->hs_h = 0;
}

// the per-tile counts on the device, copied when they differ from the ones it holds
int reproject_upload_counts(rt_ctx* c, Device& d, int nt, const char* what) {
    std::vector<int32_t> counts = c->tile_frames;
    if (counts.empty()) counts.assign((size_t)nt, c->moments_frames);
    if ((int)counts.size() != nt) return set_err(c, RT_ERR_STATE, std::string(what) + ": the tile counts do not match the image");
    if (counts != c->rp_counts || !d.rp_counts.ptr) {
        c->rp_counts.clear();
        int r;
        if ((r = ensure(c, d, d.rp_counts, (size_t)nt * sizeof(int32_t)))) return r;
        if ((r = h2d(c, d, d.rp_counts.ptr, counts.data(), (size_t)nt * sizeof(int32_t)))) return r;
        c->rp_counts.swap(counts);
    }
    return RT_OK;
}

}  // namespace rt_impl

using namespace rt_impl;

namespace {

// what both calls need of the context; `what` names the call in the message
int reproject_ready(rt_ctx* c, const char* what) {
    const std::string w(what);
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, w + " needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, w + ": not under rt_set_partition");
    if (c->width <= 0 || !c->devs[0].image_ptr) return set_err(c, RT_ERR_STATE, w + ": no image (rt_resize first)");
    return RT_OK;
}

int features_ready(rt_ctx* c, const char* what) {
    const Device& d = c->devs[0];
    if (!(c->ft_valid && d.ft_nd.ptr && d.ft_ai.ptr))
        return set_err(c, RT_ERR_STATE,
                       std::string(what) + ": no first-hit features held for the current scene and camera (rt_render_features first)");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_history_capture(rt_ctx* c, int source) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (source != RT_HISTORY_FROM_IMAGE && source != RT_HISTORY_FROM_REPROJECTED)
        return set_err(c, RT_ERR_INVALID_ARG, "rt_history_capture: source is RT_HISTORY_FROM_IMAGE or RT_HISTORY_FROM_REPROJECTED");
    int r = reproject_ready(c, "rt_history_capture");
    if (r) return r;
    Device& d = c->devs[0];
    const bool from_image = source == RT_HISTORY_FROM_IMAGE;
    if (from_image) {
        if (!c->moments || !d.m2.ptr)
            return set_err(c, RT_ERR_STATE, "rt_history_capture: the tile counts need rt_set_moments(ctx, 1) first");
        if (c->moments_frames < 1 && c->tile_frames.empty())
            return set_err(c, RT_ERR_STATE, "rt_history_capture: no tile holds a frame (rt_render from frame 1 first)");
    } else if (!c->rp_valid || !d.rp_out.ptr || (c->hist_var && !d.rp_s2.ptr)) {
        return set_err(c, RT_ERR_STATE, "rt_history_capture: no reprojected result held (rt_reproject first)");
    }
    if ((r = features_ready(c, "rt_history_capture"))) return r;
    if (!c->have_cam) return set_err(c, RT_ERR_STATE, "rt_set_camera before rt_history_capture");
    float M[9];
    if (reproject_matrix(c->cam, M))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_history_capture: the camera's pixel deltas and view corner are not independent");
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows;
    const size_t n = (size_t)W * H, bytes = n * sizeof(rt_dn4);
    const int nt = ((W + 7) / 8) * ((H + 7) / 8);
    c->hs_valid = false;
    if ((r = ensure(c, d, d.hs_px, bytes))) return r;
    if ((r = ensure(c, d, d.hs_nd, bytes))) return r;
    if ((r = ensure(c, d, d.hs_ai, bytes))) return r;
    if (c->hist_var && (r = ensure(c, d, d.hs_s2, n * sizeof(float)))) return r;
    if (from_image) {
        if ((r = reproject_upload_counts(c, d, nt, "rt_history_capture"))) return r;
        if (c->hist_var)
            hipLaunchKernelGGL(history_var_kernel, dim3((unsigned)((nt + kTilesPerBlock - 1) / kTilesPerBlock)), dim3(256), 0,
                               d.stream, (const rt_dn4*)d.image_ptr, (const rt_dn4*)d.m2.ptr, (const int32_t*)d.rp_counts.ptr, W,
                               H, (rt_dn4*)d.hs_px.ptr, (float*)d.hs_s2.ptr);
        else
            hipLaunchKernelGGL(history_kernel, dim3((unsigned)((nt + kTilesPerBlock - 1) / kTilesPerBlock)), dim3(256), 0,
                               d.stream, (const rt_dn4*)d.image_ptr, (const int32_t*)d.rp_counts.ptr, W, H, (rt_dn4*)d.hs_px.ptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return set_err(c, RT_ERR_DEVICE, std::string("rt_history_capture launch failed: ") + hipGetErrorString(e));
    } else {
        HIPCHK(c, hipMemcpyAsync(d.hs_px.ptr, d.rp_out.ptr, bytes, hipMemcpyDeviceToDevice, d.stream));
        if (c->hist_var)
            HIPCHK(c, hipMemcpyAsync(d.hs_s2.ptr, d.rp_s2.ptr, n * sizeof(float), hipMemcpyDeviceToDevice, d.stream));
    }
    HIPCHK(c, hipMemcpyAsync(d.hs_nd.ptr, d.ft_nd.ptr, bytes, hipMemcpyDeviceToDevice, d.stream));
    HIPCHK(c, hipMemcpyAsync(d.hs_ai.ptr, d.ft_ai.ptr, bytes, hipMemcpyDeviceToDevice, d.stream));
    c->hs_cam = c->cam;
    for (int k = 0; k < 9; k++) c->hs_M[k] = M[k];
    c->hs_w = W;
    c->hs_h = H;
    c->hs_valid = true;
    return RT_OK;
}

int rt_reproject(rt_ctx* c, const rt_reproject_params* params) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_rp_resolved prm;
    if (reproject_resolve(params, &prm))
        return set_err(c, RT_ERR_INVALID_ARG,
                       "rt_reproject: cos_min in [-1, 1], kz >= 0 and finite, max_history > 0 and finite, reserved 0");
    int r = reproject_ready(c, "rt_reproject");
    if (r) return r;
    Device& d = c->devs[0];
    if (!c->hs_valid || !d.hs_px.ptr || !d.hs_nd.ptr || !d.hs_ai.ptr || (c->hist_var && !d.hs_s2.ptr))
        return set_err(c, RT_ERR_STATE, "rt_reproject: no history held (rt_history_capture first)");
    if (c->hs_w != c->width || c->hs_h != d.local_rows)
        return set_err(c, RT_ERR_STATE, "rt_reproject: the image's size is not the history's (rt_history_capture again)");
    if (!c->moments || !d.m2.ptr)
        return set_err(c, RT_ERR_STATE, "rt_reproject: the tile counts need rt_set_moments(ctx, 1) first");
    if ((r = features_ready(c, "rt_reproject"))) return r;
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows;
    const size_t n = (size_t)W * H;
    const int nt = ((W + 7) / 8) * ((H + 7) / 8);
    c->rp_valid = false;
    if ((r = ensure(c, d, d.rp_out, n * sizeof(rt_dn4)))) return r;
    if (c->hist_var && (r = ensure(c, d, d.rp_s2, n * sizeof(float)))) return r;
    if ((r = reproject_upload_counts(c, d, nt, "rt_reproject"))) return r;
    rt_rp_view V;
    V.cam = c->cam;
    V.cam_h = c->hs_cam;
    for (int k = 0; k < 9; k++) V.M[k] = c->hs_M[k];
    V.cos_min = prm.cos_min;
    V.kz = prm.kz;
    V.max_history = prm.max_history;
    V.W = W;
    V.H = H;
    const dim3 grid((unsigned)((nt + kTilesPerBlock - 1) / kTilesPerBlock));
    if (c->hist_var)
        hipLaunchKernelGGL(c->rp_misses ? reproject_miss_var_kernel : reproject_var_kernel, grid, dim3(256), 0, d.stream,
                           (const rt_dn4*)d.image_ptr, (const rt_dn4*)d.m2.ptr, (const int32_t*)d.rp_counts.ptr,
                           (const rt_dn4*)d.ft_nd.ptr, (const rt_dn4*)d.ft_ai.ptr, (const rt_dn4*)d.hs_px.ptr,
                           (const rt_dn4*)d.hs_nd.ptr, (const rt_dn4*)d.hs_ai.ptr, (const float*)d.hs_s2.ptr, V,
                           (rt_dn4*)d.rp_out.ptr, (float*)d.rp_s2.ptr);
    else
        hipLaunchKernelGGL(c->rp_misses ? reproject_miss_kernel : reproject_kernel, grid, dim3(256), 0, d.stream,
                           (const rt_dn4*)d.image_ptr, (const int32_t*)d.rp_counts.ptr, (const rt_dn4*)d.ft_nd.ptr,
                           (const rt_dn4*)d.ft_ai.ptr, (const rt_dn4*)d.hs_px.ptr, (const rt_dn4*)d.hs_nd.ptr,
                           (const rt_dn4*)d.hs_ai.ptr, V, (rt_dn4*)d.rp_out.ptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string("rt_reproject launch failed: ") + hipGetErrorString(e));
    c->rp_ft_gen = c->ft_gen;
    c->rp_gen++;   // another result: a denoised buffer made from the one before is not this one's (rt_present)
    c->rp_valid = true;
    return RT_OK;
}

int rt_read_reprojected(rt_ctx* c, float* rgbn) {
    if (!c || !rgbn) return RT_ERR_INVALID_ARG;
    if (!c->rp_valid || c->devs.size() != 1 || !c->devs[0].rp_out.ptr)
        return set_err(c, RT_ERR_STATE, "rt_read_reprojected: no reprojected result held (rt_reproject first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, rgbn, d.rp_out.ptr, (size_t)d.local_rows * c->width * 16);
}

int rt_set_history_variance(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID_ARG;
    if ((on != 0) == c->hist_var) return RT_OK;
    c->hist_var = on != 0;
    c->hs_valid = c->rp_valid = false;   // what is held was made under the other value
    return RT_OK;
}

int rt_set_reproject_misses(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID_ARG;
    if ((on != 0) == c->rp_misses) return RT_OK;
    c->rp_misses = on != 0;
    c->rp_valid = false;   // the result was made under the other value; the history is the same under both
    return RT_OK;
}

int rt_read_reprojected_variance(rt_ctx* c, float* s2) {
    if (!c || !s2) return RT_ERR_INVALID_ARG;
    if (!c->rp_valid || !c->hist_var || c->devs.size() != 1 || !c->devs[0].rp_s2.ptr)
        return set_err(c, RT_ERR_STATE,
                       "rt_read_reprojected_variance: no reprojected result with variance held (rt_set_history_variance(ctx, 1) "
                       "and rt_reproject first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, s2, d.rp_s2.ptr, (size_t)d.local_rows * c->width * sizeof(float));
}

}  // extern "C"
