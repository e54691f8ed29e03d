// rt_present.hip — the presented frame (rt.h rt_present / rt_read_presented / rt_bind_device_present) and the
// one call per pose over it (rt_render_moved).  Nothing here touches the render kernels, the image, the
// moments, the counts, the features, the history, the reprojected result or the filter's buffers: the
// frame and its float copy are buffers of their own, allocated by the first rt_present.
//
// present_kernel: one lane per pixel, 64x4 workgroups, a wave = 64 consecutive pixels of a row (the dn_*
// kernels' shape; only the tile count looks at the 8x8 grid), partial rows guarded, no atomics.  Per pixel
// it reads one whole float4 (RT_PRESENT_MOVED: two, and the tile's count), stores one dword and, with
// keep_float, one float4.  Instantiated by <source, keep_float>, so every source reads only its own
// buffers.  The arithmetic is rt_present_math.h's, shared with rt_present_host, which the frame equals bit
// for bit.  The 256-byte gamma table (rt_gamma_lut.h) is built on the host and copied to a device buffer
// once; the lanes index it there (two cache lines that every wave of the launch shares).  The -DRT_AB_KNOBS
// library also holds the instantiations that stage the table into LDS per workgroup (64 lanes, one dword
// each, one barrier), chosen by RT_PRESENT_LUT=lds in the environment: tools/present_cost.py times both
// (profiles/present_cost.json).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "rt/rt.h"
#include "rt_ctx.h"
#include "rt_gamma_lut.h"
#include "rt_present.h"
#include "rt_present_math.h"
#include "rt_refine.h"

namespace {

static_assert(sizeof(rt_dn4) == sizeof(float4), "a source pixel is one float4");

constexpr int kBX = 64, kBY = 4;   // a workgroup: 4 waves, one row segment each

// src: the source's buffer (RT_PRESENT_MOVED: the reprojected result); dn and counts: the denoised buffer and
// the per-tile frame counts, read by RT_PRESENT_MOVED alone; dstf: the float copy, written with KEEP_FLOAT alone
template <int SOURCE, bool KEEP_FLOAT, bool LDS_TABLE>
__global__ void __launch_bounds__(256) present_kernel(const rt_dn4* __restrict__ src, const rt_dn4* __restrict__ dn,
                                                      const int32_t* __restrict__ counts, const uint8_t* __restrict__ lut,
                                                      int W, int H, float exposure, uint32_t* __restrict__ dst,
                                                      rt_dn4* __restrict__ dstf) {
    const uint8_t* table = lut;
    if constexpr (LDS_TABLE) {   // before the guard: every lane of the workgroup reaches the barrier
        __shared__ alignas(4) uint8_t s_lut[256];
        if (threadIdx.y == 0) ((uint32_t*)s_lut)[threadIdx.x] = ((const uint32_t*)lut)[threadIdx.x];
        __syncthreads();
        table = s_lut;
    }
    const int x = (int)blockIdx.x * kBX + (int)threadIdx.x, y = (int)blockIdx.y * kBY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    rt_dn4 c = src[p];
    if (SOURCE == RT_PRESENT_MOVED) {
        const int tiles_x = (W + 7) >> 3;
        c = pr_moved(c, dn[p], counts[(size_t)(y >> 3) * tiles_x + (x >> 3)]);
    } else {
        c.w = 1.0f;
    }
    const rt_dn4 e = pr_expose(c, exposure);
    dst[p] = pr_pack(e, table);
    if (KEEP_FLOAT) dstf[p] = e;
}

struct Launch {
    const rt_dn4 *src, *dn;
    const int32_t* counts;
    const uint8_t* lut;
    int W, H;
    float exposure;
    uint32_t* dst;
    rt_dn4* dstf;
};

template <int SOURCE, bool KEEP_FLOAT, bool LDS_TABLE>
void launch_one(const Launch& a, hipStream_t stream) {
    const dim3 block(kBX, kBY), grid((unsigned)((a.W + kBX - 1) / kBX), (unsigned)((a.H + kBY - 1) / kBY));
    hipLaunchKernelGGL((present_kernel<SOURCE, KEEP_FLOAT, LDS_TABLE>), grid, block, 0, stream, a.src, a.dn, a.counts, a.lut, a.W,
                       a.H, a.exposure, a.dst, a.dstf);
}

template <bool LDS_TABLE>
void launch_by(int source, bool keep, const Launch& a, hipStream_t stream) {
#define RT_PR_CASE(S)                                           \
    case S:                                                     \
        if (keep) launch_one<S, true, LDS_TABLE>(a, stream);    \
        else launch_one<S, false, LDS_TABLE>(a, stream);        \
        break;
    switch (source) {
        RT_PR_CASE(RT_PRESENT_IMAGE)
        RT_PR_CASE(RT_PRESENT_DENOISED)
        RT_PR_CASE(RT_PRESENT_REPROJECTED)
        RT_PR_CASE(RT_PRESENT_MOVED)
    }
#undef RT_PR_CASE
}

}  // namespace

namespace rt_impl {

void present_free(rt_ctx* c) {
    for (Device& d : c->devs) {
        dev_free(d.pr_out);
        dev_free(d.pr_float);
        dev_free(d.pr_lut);
        d.pr_ptr = nullptr;
        d.pr_bound = false;
    }
    c->pr_valid = c->pr_float_valid = false;
}

}  // namespace rt_impl

using namespace rt_impl;

namespace {

// what every call here needs of the context; `what` names the call in the message
int present_ready(rt_ctx* c, const char* what) {
    const std::string w(what);
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, w + " needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, w + ": not under rt_set_partition");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, w + ": no image (rt_resize first)");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_present(rt_ctx* c, const rt_present_params* params) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_pr_resolved prm;
    if (present_resolve(params, &prm))
        return set_err(c, RT_ERR_INVALID_ARG,
                       "rt_present: source is one of RT_PRESENT_*, exposure > 0 and finite, reserved 0");
    int r = present_ready(c, "rt_present");
    if (r) return r;
    Device& d = c->devs[0];
    const bool rp_held = c->rp_valid && d.rp_out.ptr;
    const rt_dn4 *src = nullptr, *dn = nullptr;
    switch (prm.source) {
        case RT_PRESENT_IMAGE:
            if (!d.image_ptr) return set_err(c, RT_ERR_STATE, "rt_present: no image (rt_resize first)");
            src = (const rt_dn4*)d.image_ptr;
            break;
        case RT_PRESENT_DENOISED:
            if (c->dn_result < 0 || !d.dn_px[c->dn_result].ptr)
                return set_err(c, RT_ERR_STATE, "rt_present: no filtered image held (rt_denoise first)");
            src = (const rt_dn4*)d.dn_px[c->dn_result].ptr;
            break;
        case RT_PRESENT_REPROJECTED:
            if (!rp_held) return set_err(c, RT_ERR_STATE, "rt_present: no reprojected result held (rt_reproject first)");
            src = (const rt_dn4*)d.rp_out.ptr;
            break;
        default:   // RT_PRESENT_MOVED
            if (!rp_held) return set_err(c, RT_ERR_STATE, "rt_present: no reprojected result held (rt_reproject first)");
            if (!c->moments || !d.m2.ptr)
                return set_err(c, RT_ERR_STATE, "rt_present: the tile counts need rt_set_moments(ctx, 1) first");
            if (c->dn_result < 0 || !d.dn_px[c->dn_result].ptr || c->dn_rp_gen == 0 || c->dn_rp_gen != c->rp_gen)
                return set_err(c, RT_ERR_STATE,
                               "rt_present: the denoised buffer was not written by rt_denoise_reprojected from the reprojected "
                               "result now held (rt_denoise_reprojected first)");
            src = (const rt_dn4*)d.rp_out.ptr;
            dn = (const rt_dn4*)d.dn_px[c->dn_result].ptr;
            break;
    }
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows;
    const size_t n = (size_t)W * H;
    c->pr_valid = c->pr_float_valid = false;
    if (!d.pr_bound) {
        if ((r = ensure(c, d, d.pr_out, n * sizeof(uint32_t)))) return r;
        d.pr_ptr = d.pr_out.ptr;
    }
    if (prm.keep_float && (r = ensure(c, d, d.pr_float, n * sizeof(rt_dn4)))) return r;
    if (!d.pr_lut.ptr) {
        if ((r = ensure(c, d, d.pr_lut, 256))) return r;
        if ((r = h2d(c, d, d.pr_lut.ptr, rt_gamma_table().v, 256))) {
            dev_free(d.pr_lut);
            return r;
        }
    }
    if (prm.source == RT_PRESENT_MOVED &&
        (r = reproject_upload_counts(c, d, ((W + 7) / 8) * ((H + 7) / 8), "rt_present")))
        return r;
    const Launch a = {src, dn, (const int32_t*)d.rp_counts.ptr, (const uint8_t*)d.pr_lut.ptr, W, H, prm.exposure,
                      (uint32_t*)d.pr_ptr, prm.keep_float ? (rt_dn4*)d.pr_float.ptr : nullptr};
    bool lds_table = false;
#ifdef RT_AB_KNOBS
    // A/B build only (tools/present_cost.py): the table staged into LDS per workgroup
    if (const char* v = std::getenv("RT_PRESENT_LUT")) lds_table = std::strcmp(v, "lds") == 0;
    if (lds_table) launch_by<true>(prm.source, prm.keep_float, a, d.stream);
#endif
    if (!lds_table) launch_by<false>(prm.source, prm.keep_float, a, d.stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string("rt_present launch failed: ") + hipGetErrorString(e));
    c->pr_valid = true;
    c->pr_float_valid = prm.keep_float;
    return RT_OK;
}

int rt_read_presented(rt_ctx* c, uint8_t* rgba8) {
    if (!c || !rgba8) return RT_ERR_INVALID_ARG;
    if (!c->pr_valid || c->devs.size() != 1 || !c->devs[0].pr_ptr)
        return set_err(c, RT_ERR_STATE, "rt_read_presented: no presented frame held (rt_present first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, rgba8, d.pr_ptr, (size_t)d.local_rows * c->width * 4);
}

int rt_read_presented_float(rt_ctx* c, float* rgbw) {
    if (!c || !rgbw) return RT_ERR_INVALID_ARG;
    if (!c->pr_valid || !c->pr_float_valid || c->devs.size() != 1 || !c->devs[0].pr_float.ptr)
        return set_err(c, RT_ERR_STATE,
                       "rt_read_presented_float: no float copy held (rt_present with keep_float first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, rgbw, d.pr_float.ptr, (size_t)d.local_rows * c->width * 16);
}

int rt_bind_device_present(rt_ctx* c, void* ptr, size_t nbytes) {
    if (!c) return RT_ERR_INVALID_ARG;
    int r = present_ready(c, "rt_bind_device_present");
    if (r) return r;
    Device& d = c->devs[0];
    if (ptr && nbytes < (size_t)d.local_rows * c->width * 4)
        return set_err(c, RT_ERR_INVALID_ARG, "rt_bind_device_present: device buffer too small");
    if (ptr && ((uintptr_t)ptr & 3u))
        return set_err(c, RT_ERR_INVALID_ARG, "rt_bind_device_present: device buffer not 4-byte aligned");
    c->pr_valid = c->pr_float_valid = false;   // the frame held was the other buffer's
    d.pr_ptr = ptr ? ptr : d.pr_out.ptr;
    d.pr_bound = ptr != nullptr;
    return RT_OK;
}

int rt_render_moved(rt_ctx* c, const float camera[28], int n_frames, const float* rand_factors,
                    const rt_reproject_params* reproject, const rt_denoise_params* denoise, const rt_guide_params* guides,
                    const rt_present_params* present) {
    if (!c) return RT_ERR_INVALID_ARG;
    int r;
    if ((r = moved_to_reprojected(c, camera, n_frames, rand_factors, reproject))) return r;
    return moved_filter_present(c, denoise, guides, present);
}

}  // extern "C"

namespace rt_impl {

// rt_render_moved's steps 1 to 5
int moved_to_reprojected(rt_ctx* c, const float camera[28], int n_frames, const float* rand_factors,
                         const rt_reproject_params* reproject) {
    int r;
    // a result made from the feature buffers now held, and those current: it is the pose's being left
    const bool result_here = c->rp_valid && c->ft_valid && c->rp_ft_gen == c->ft_gen;
    if ((r = rt_history_capture(c, result_here ? RT_HISTORY_FROM_REPROJECTED : RT_HISTORY_FROM_IMAGE))) return r;
    if ((r = rt_set_camera(c, camera))) return r;
    if ((r = rt_render(c, 1, n_frames, rand_factors))) return r;
    if ((r = rt_render_features(c))) return r;
    return rt_reproject(c, reproject);
}

// ... and its steps 6 and 7
int moved_filter_present(rt_ctx* c, const rt_denoise_params* denoise, const rt_guide_params* guides,
                         const rt_present_params* present) {
    int r;
    if (c->hist_var && (r = rt_denoise_reprojected(c, denoise, guides))) return r;
    rt_present_params p;
    if (present) {
        p = *present;
    } else {
        std::memset(&p, 0, sizeof(p));
        p.source = c->hist_var ? RT_PRESENT_MOVED : RT_PRESENT_REPROJECTED;
        p.exposure = 1.0f;
    }
    return rt_present(c, &p);
}

}  // namespace rt_impl
