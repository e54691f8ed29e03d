// rt_denoise.hip — the variance-guided a-trous preview filter (rt.h rt_denoise / rt_read_denoised).
// Nothing here touches the render kernels or the image: a prologue builds level 0 {r, g, b, V_0}
// from the image, M2.w and a device copy of the per-tile frame counts, then every level runs two
// passes over ping-pong float4 buffers: vb_kernel (the 3x3-averaged variance, one float per pixel)
// and filter_kernel (the 5x5 taps at step 2^level).  One thread per pixel, a wave = 64 consecutive
// pixels of a row, so every tap of a wave is one contiguous float4 row segment; taps come straight
// from global memory at every step (the caches serve the reuse between neighbours; an LDS tile with
// halo for steps 1 and 2 measured no faster, the level being bound by its 24 divisions and square
// roots per pixel: DESIGN.md §4).  The arithmetic is rt_denoise_math.h's, shared with the host
// reference, which the result equals bit for bit.  rt_denoise_guided runs the same passes with
// dn_filter_guided_kernel, whose taps also read the first-hit buffers (rt_features.hip) for the guide factor.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "rt/rt.h"
#include "rt_ctx.h"
#include "rt_denoise.h"
#include "rt_denoise_math.h"

namespace {

static_assert(sizeof(rt_dn4) == sizeof(float4), "a level's pixel is one float4");

constexpr int kBX = 64, kBY = 4;   // a workgroup: 4 waves, one row segment each

__global__ void __launch_bounds__(256) dn_prologue_kernel(const rt_dn4* __restrict__ image,
                                                          const rt_dn4* __restrict__ moments,
                                                          const int32_t* __restrict__ counts, int W, int H,
                                                          rt_dn4* __restrict__ dst) {
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const int tiles_x = (W + 7) >> 3;
    dst[p] = dn_level0(image[p], moments[p].w, counts[(size_t)(y >> 3) * tiles_x + (x >> 3)]);
}

// rt_denoise_reprojected's level 0, from the reprojected view {r, g, b, n}, its s2 and the ids: one whole
// float4 and one float per pixel where s2 is known; only the lanes whose s2 is unknown (fresh pixels after
// a move) walk the 5x5 neighbourhood, whose rows are the wave's own row segment and its four neighbours.
__global__ void __launch_bounds__(256) dn_prologue_reprojected_kernel(const rt_dn4* __restrict__ rgbn,
                                                                      const float* __restrict__ s2,
                                                                      const rt_dn4* __restrict__ ai, int W, int H,
                                                                      rt_dn4* __restrict__ dst) {
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    dst[(size_t)y * W + x] = dn_level0_reprojected(rgbn, s2, ai, W, H, x, y);
}

__global__ void __launch_bounds__(256) dn_vb_kernel(const rt_dn4* __restrict__ src, float* __restrict__ vb, int W, int H) {
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    vb[(size_t)y * W + x] = dn_vb(src, W, H, x, y);
}

// FINAL: the last level stores w = 1 where the others keep V (a bad pixel's flag included).
template <bool FINAL>
__global__ void __launch_bounds__(256) dn_filter_kernel(const rt_dn4* __restrict__ src, const float* __restrict__ vb,
                                                        rt_dn4* __restrict__ dst, int W, int H, int s, float k) {
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    rt_dn4 o = dn_filter(src, vb, W, H, x, y, s, k);
    if (FINAL) o.w = 1.0f;
    dst[(size_t)y * W + x] = o;
}

// rt_denoise_guided's level: the same taps, each weight times dn_guide_weight of the first-hit buffers
template <bool FINAL>
__global__ void __launch_bounds__(256) dn_filter_guided_kernel(const rt_dn4* __restrict__ src, const float* __restrict__ vb,
                                                               rt_dn4* __restrict__ dst, int W, int H, int s, float k,
                                                               rt_dn_guides G) {
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    rt_dn4 o = dn_filter_guided(src, vb, W, H, x, y, s, k, G);
    if (FINAL) o.w = 1.0f;
    dst[(size_t)y * W + x] = o;
}

}  // namespace

namespace rt_impl {

void denoise_free(rt_ctx* c) {
    for (Device& d : c->devs) {
        dev_free(d.dn_px[0]);
        dev_free(d.dn_px[1]);
        dev_free(d.dn_vb);
        dev_free(d.dn_counts);
    }
    c->dn_counts.clear();
    c->dn_result = -1;
}

}  // namespace rt_impl

using namespace rt_impl;

namespace {

// The levels over level 0 in Device::dn_px[0] (queued by the caller): vb and filter passes over the
// ping-pong buffers; the buffer that holds the result becomes rt_ctx::dn_result.  guides NULL or all 0:
// the unguided kernels.  `what` names the call in a launch error.
int run_levels(rt_ctx* c, Device& d, int W, int H, const rt_dn_resolved& prm, const rt_guide_resolved* guides, const char* what) {
    const bool guided = guides && dn_guides_on(*guides);
    const dim3 block(kBX, kBY), grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
    rt_dn4* buf[2] = {(rt_dn4*)d.dn_px[0].ptr, (rt_dn4*)d.dn_px[1].ptr};
    int cur = 0;
    rt_dn_guides G = {nullptr, nullptr, 0.0f, 0.0f, 0.0f};
    if (guided) G = {(const rt_dn4*)d.ft_nd.ptr, (const rt_dn4*)d.ft_ai.ptr, guides->kn, guides->kz, guides->ka};
    for (int lv = 0; lv < prm.levels; lv++, cur ^= 1) {
        hipLaunchKernelGGL(dn_vb_kernel, grid, block, 0, d.stream, (const rt_dn4*)buf[cur], (float*)d.dn_vb.ptr, W, H);
        if (guided && lv + 1 == prm.levels)
            hipLaunchKernelGGL(dn_filter_guided_kernel<true>, grid, block, 0, d.stream, (const rt_dn4*)buf[cur],
                               (const float*)d.dn_vb.ptr, buf[cur ^ 1], W, H, 1 << lv, prm.k, G);
        else if (guided)
            hipLaunchKernelGGL(dn_filter_guided_kernel<false>, grid, block, 0, d.stream, (const rt_dn4*)buf[cur],
                               (const float*)d.dn_vb.ptr, buf[cur ^ 1], W, H, 1 << lv, prm.k, G);
        else if (lv + 1 == prm.levels)
            hipLaunchKernelGGL(dn_filter_kernel<true>, grid, block, 0, d.stream, (const rt_dn4*)buf[cur],
                               (const float*)d.dn_vb.ptr, buf[cur ^ 1], W, H, 1 << lv, prm.k);
        else
            hipLaunchKernelGGL(dn_filter_kernel<false>, grid, block, 0, d.stream, (const rt_dn4*)buf[cur],
                               (const float*)d.dn_vb.ptr, buf[cur ^ 1], W, H, 1 << lv, prm.k);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string(what) + " launch failed: " + hipGetErrorString(e));
    c->dn_result = cur;
    return RT_OK;
}

// rt_denoise (guides NULL) and rt_denoise_guided (the resolved strengths; all 0: the unguided kernels)
int run_denoise(rt_ctx* c, const rt_denoise_params* params, const rt_guide_resolved* guides) {
    rt_dn_resolved prm;
    if (denoise_resolve(params, &prm))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_denoise: levels 1..5, k > 0 and finite, reserved 0");
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "rt_denoise needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, "rt_denoise: not under rt_set_partition");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "no image");
    if (!c->moments) return set_err(c, RT_ERR_STATE, "rt_set_moments(ctx, 1) first");
    Device& d = c->devs[0];
    if (!d.m2.ptr || !d.image_ptr) return set_err(c, RT_ERR_STATE, "no image");
    if (guides && !(c->ft_valid && d.ft_nd.ptr && d.ft_ai.ptr))
        return set_err(c, RT_ERR_STATE, "rt_denoise_guided: no first-hit features held (rt_render_features first)");
    if (c->moments_frames < 2)   // the smallest tile count (rt_ctx.h)
        return set_err(c, RT_ERR_STATE,
                       c->moments_frames < 1 ? "the moments are invalid: render from frame 1 (or rt_write_moments)"
                                             : "rt_denoise needs at least two frames in every tile");
    const int W = c->width, H = d.local_rows;
    const int tiles_x = (W + 7) / 8, nt = tiles_x * ((H + 7) / 8);
    const size_t n = (size_t)W * H;
    HIPCHK(c, hipSetDevice(d.id));
    int r;
    if ((r = ensure(c, d, d.dn_px[0], n * sizeof(rt_dn4)))) return r;
    if ((r = ensure(c, d, d.dn_px[1], n * sizeof(rt_dn4)))) return r;
    if ((r = ensure(c, d, d.dn_vb, n * sizeof(float)))) return r;
    // the per-tile counts on the device, copied when they differ from the ones it holds
    std::vector<int32_t> counts = c->tile_frames;
    if (counts.empty()) counts.assign((size_t)nt, c->moments_frames);
    if ((int)counts.size() != nt) return set_err(c, RT_ERR_STATE, "rt_denoise: the tile counts do not match the image");
    if (counts != c->dn_counts || !d.dn_counts.ptr) {
        c->dn_counts.clear();
        if ((r = ensure(c, d, d.dn_counts, (size_t)nt * sizeof(int32_t)))) return r;
        if ((r = h2d(c, d, d.dn_counts.ptr, counts.data(), (size_t)nt * sizeof(int32_t)))) return r;
        c->dn_counts.swap(counts);
    }
    c->dn_result = -1;
    c->dn_rp_gen = 0;
    const dim3 block(kBX, kBY), grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
    hipLaunchKernelGGL(dn_prologue_kernel, grid, block, 0, d.stream, (const rt_dn4*)d.image_ptr, (const rt_dn4*)d.m2.ptr,
                       (const int32_t*)d.dn_counts.ptr, W, H, (rt_dn4*)d.dn_px[0].ptr);
    return run_levels(c, d, W, H, prm, guides, "rt_denoise");
}

// rt_denoise_reprojected: level 0 from the reprojected view and its s2, then the same levels
int run_denoise_reprojected(rt_ctx* c, const rt_denoise_params* params, const rt_guide_resolved& guides) {
    rt_dn_resolved prm;
    if (denoise_resolve(params, &prm))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_denoise_reprojected: levels 1..5, k > 0 and finite, reserved 0");
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "rt_denoise_reprojected needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, "rt_denoise_reprojected: not under rt_set_partition");
    Device& d = c->devs[0];
    if (!c->hist_var || !c->rp_valid || !d.rp_out.ptr || !d.rp_s2.ptr)
        return set_err(c, RT_ERR_STATE,
                       "rt_denoise_reprojected: no reprojected result with variance held (rt_set_history_variance(ctx, 1) and "
                       "rt_reproject first)");
    if (!(c->ft_valid && d.ft_nd.ptr && d.ft_ai.ptr))
        return set_err(c, RT_ERR_STATE,
                       "rt_denoise_reprojected: no first-hit features held for the current scene and camera (rt_render_features "
                       "and rt_reproject first)");
    if (c->ft_gen != c->rp_ft_gen)
        return set_err(c, RT_ERR_STATE,
                       "rt_denoise_reprojected: the first-hit features were rendered again since the result was made (rt_reproject "
                       "again)");
    const int W = c->width, H = d.local_rows;
    const size_t n = (size_t)W * H;
    HIPCHK(c, hipSetDevice(d.id));
    int r;
    if ((r = ensure(c, d, d.dn_px[0], n * sizeof(rt_dn4)))) return r;
    if ((r = ensure(c, d, d.dn_px[1], n * sizeof(rt_dn4)))) return r;
    if ((r = ensure(c, d, d.dn_vb, n * sizeof(float)))) return r;
    c->dn_result = -1;
    c->dn_rp_gen = 0;
    const dim3 block(kBX, kBY), grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
    hipLaunchKernelGGL(dn_prologue_reprojected_kernel, grid, block, 0, d.stream, (const rt_dn4*)d.rp_out.ptr,
                       (const float*)d.rp_s2.ptr, (const rt_dn4*)d.ft_ai.ptr, W, H, (rt_dn4*)d.dn_px[0].ptr);
    if ((r = run_levels(c, d, W, H, prm, &guides, "rt_denoise_reprojected"))) return r;
    c->dn_rp_gen = c->rp_gen;   // the buffer holds this result, filtered (rt_present's RT_PRESENT_MOVED)
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise(rt_ctx* c, const rt_denoise_params* params) {
    if (!c) return RT_ERR_INVALID_ARG;
    return run_denoise(c, params, nullptr);
}

int rt_denoise_guided(rt_ctx* c, const rt_denoise_params* params, const rt_guide_params* guides) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_guide_resolved g;
    if (guide_resolve(guides, &g))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_denoise_guided: kn, kz, ka >= 0 and finite, reserved 0");
    return run_denoise(c, params, &g);
}

int rt_denoise_reprojected(rt_ctx* c, const rt_denoise_params* params, const rt_guide_params* guides) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_guide_resolved g;
    if (guide_resolve(guides, &g))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_denoise_reprojected: kn, kz, ka >= 0 and finite, reserved 0");
    return run_denoise_reprojected(c, params, g);
}

int rt_read_denoised(rt_ctx* c, float* rgba) {
    if (!c || !rgba) return RT_ERR_INVALID_ARG;
    if (c->dn_result < 0 || c->devs.size() != 1 || !c->devs[0].dn_px[c->dn_result].ptr)
        return set_err(c, RT_ERR_STATE, "rt_read_denoised: no filtered image held (rt_denoise first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, rgba, d.dn_px[c->dn_result].ptr, (size_t)d.local_rows * c->width * 16);
}

}  // extern "C"
