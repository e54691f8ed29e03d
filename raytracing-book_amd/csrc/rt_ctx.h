// rt_ctx.h — the context behind the C ABI's rt_ctx handle and the device helpers its
// translation units share (rt_capi.hip, rt_comm.hip, rt_debug.hip, rt_denoise.hip, rt_features.hip, rt_reproject.hip, rt_present.hip, rt_refine.hip).  Internal to the libraries.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include <rccl/rccl.h>   // types only: librccl (~570 MB) is dlopen'ed by the first gather that uses it

#include "rt/rt.h"
#include "rt/rt_debug.h"
#include "rt/rt_types.h"
#include "rt_args.h"
#include "rt_device.h"
#include "rt_prep.h"

namespace rt_impl __attribute__((visibility("hidden"))) {

struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
};

struct Device {
    int id = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool timed = false;
    DevBuf nodes, spheres, quads, boxes, media, lights, tex[8];
    DevBuf dquads, dboxes;   // intersection-only face records (rt_device.h)
    DevBuf dboxc;            // compact canonical box records (RT_BOXC_F4 per box)
    DevBuf perlin_pk;        // the Perlin table re-laid out (rt_kernel.hip perlin_noise_pk), when it qualifies
    DevBuf image;            // internal image
    DevBuf args;             // rt_kernel_args slot in device memory
    DevBuf stats;            // diagnostic counters (rt_debug_enable_stats)
    DevBuf census;           // the stats twin's leaf census (rt_debug_enable_stats(ctx, 2))
    DevBuf node_hits;        // the stats twin's node-hit count (rt_debug_count_node_hits)
    int census_cap = 0, census_waves = 0;
    DevBuf counter;          // persistent-kernel work-unit counter [0] and fault word [1]
    DevBuf tile_done;        // ordered chunks: chunks published per 8x8 tile
    DevBuf samples;          // staged chunks: per-frame colours [frames][local pixels]
    DevBuf sflags;           // sparse staging: per staged sample, 1 where its colour was stored
    DevBuf m2;               // rt_set_moments: per-pixel float4 second moments [local_rows][W] (rt_moments.hip)
    DevBuf tile_sums;        // ... and their per-tile sums (rt_read_tile_sums)
    DevBuf tile_list;        // rt_set_active_tiles: the active tiles' indices, ascending (int32)
    DevBuf dn_px[2];         // rt_denoise: the levels' ping-pong {r, g, b, V} float4 per pixel (rt_denoise.hip) ...
    DevBuf dn_vb;            // ... the level's 3x3-averaged variance, one float per pixel ...
    DevBuf dn_counts;        // ... and the per-tile frame counts (int32, rt_ctx::dn_counts holds the same)
    DevBuf ft_nd, ft_ai;     // rt_render_features: normal_depth and albedo_id, float4 [local_rows][W] each (rt_features.hip) ...
    DevBuf ft_links;         // ... the pass's plain link buffer (SceneState::links) ...
    DevBuf ft_args;          // ... and its own rt_kernel_args (no LDS tables; rt_ctx::ft_args_host holds the same)
    DevBuf hs_px, hs_nd, hs_ai;   // rt_history_capture: the history's {r, g, b, n} and first-hit buffers, float4 [local_rows][W] each (rt_reproject.hip) ...
    DevBuf rp_out;           // ... rt_reproject's result {r, g, b, n_out} ...
    DevBuf rp_counts;        // ... and its copy of the per-tile frame counts (int32, rt_ctx::rp_counts holds the same)
    DevBuf hs_s2, rp_s2;     // rt_set_history_variance: the history's and the result's per-sample variance of y, one float per pixel
    DevBuf pr_out, pr_float; // rt_present: the frame's internal buffer, one rgba8 dword per pixel, and its float4 copy (rt_present.hip) ...
    DevBuf pr_lut;           // ... and the 256-byte gamma table (rt_gamma_lut.h), copied once
    void* pr_ptr = nullptr;  // ... the active frame buffer (internal or bound: rt_bind_device_present)
    bool pr_bound = false;
    DevBuf rf_tiles;         // rt_reach_tiles: one rt_tile_reach per 8x8 tile (rt_refine.hip)
    DevBuf nz_tiles;         // rt_noise_tiles: one rt_tile_noise per 8x8 tile (rt_refine.hip)
    DevBuf wbuf;             // pooled units (ordered / one chunk): per resident wave 64 x chunk_frames colours
    DevBuf finfo;            // exact near-first walk tables (variant 61)
    DevBuf f2inner, f2leaves;
    DevBuf links;            // link-format BVH (variant 0/37)
    int fast_gen = -1;       // rt_ctx::fast_gen these copies belong to
    static constexpr int kRing = 8;
    rt_kernel_args* ring = nullptr;   // pinned host staging slots for async arg uploads
    hipEvent_t ring_ev[kRing] = {};
    int ring_pos = 0;
    float* image_ptr = nullptr;  // active image (internal or bound)
    bool image_bound = false;
    int rank = 0, world = 1;     // stripe assignment of this device
    int local_rows = 0, padded_rows = 0;
    ncclComm_t comm = nullptr;   // RCCL communicator of a device gather (rank = this device's slot / process rank)
    DevBuf gather, full;         // device 0 / rank 0: the gathered stripe blocks, the de-interleaved image
};

}  // namespace rt_impl

using rt_impl::Device;
using rt_impl::FastTables;

// The scene, its options and frame counts are the base (rt_args.h: host-only, what rt_args.cpp works
// on); the context adds the devices and the bookkeeping of what was launched, gathered and filtered.
struct rt_ctx : rt_impl::SceneState {
    std::vector<Device> devs;
    std::string err;
    uint64_t last_ns = 0;
    int variant_no_stats = -1;   // the variant active before rt_debug_enable_stats(c, 1), restored by (c, 0)
    int last_launch[RT_LI_N] = {0};
    int first_leaf_last[4] = {0};   // rt_debug_first_leaf: the last launch's (armed, leaf link, type byte, prims)
    bool launched = false;
    // rt_denoise: which of Device::dn_px holds the filtered image (-1: none held), and the per-tile
    // counts last copied to Device::dn_counts (copied again only when they change)
    int dn_result = -1;
    std::vector<int32_t> dn_counts;
    // rt_render_features: the buffers hold the current scene's and camera's first hits (false: none held,
    // or stale since an upload, a camera or a BVH-mode change); ft_links_ok: Device::ft_links holds the
    // current tree's links (cleared with ft_valid); the argument block last copied to Device::ft_args
    bool ft_valid = false, ft_links_ok = false;
    uint32_t ft_gen = 0;   // counts the rt_render_features passes queued: which pass the buffers hold
    std::vector<uint8_t> ft_args_host;
    // rt_history_capture: a history is held (Device::hs_*), of this size, made with this camera block,
    // whose matrix M is hs_M (rt.h); rt_reproject: a result is held (Device::rp_out), and the per-tile
    // counts last copied to Device::rp_counts (copied again only when they change)
    bool hs_valid = false, rp_valid = false;
    int hs_w = 0, hs_h = 0;
    rt_camera_ubo hs_cam{};
    float hs_M[9] = {0};
    std::vector<int32_t> rp_counts;
    // rt_set_history_variance: the history and the result carry s2 (Device::hs_s2, rp_s2) while on; a held
    // history or result was made under the current value (a change drops both).  rp_ft_gen: the ft_gen of the
    // feature buffers the held result was made from (rt_denoise_reprojected filters over the same ones)
    bool hist_var = false;
    uint32_t rp_ft_gen = 0;
    // rt_set_reproject_misses: rt_reproject launches the instances that reproject misses by direction; a held
    // result was made under the current value (a change drops it and keeps the history)
    bool rp_misses = false;
    // rp_gen counts the rt_reproject results made (the held one is the rp_gen-th); dn_rp_gen: the rp_gen of the
    // result rt_denoise_reprojected wrote the denoised buffer from, 0 when another filter call wrote it or none did
    uint32_t rp_gen = 0, dn_rp_gen = 0;
    // rt_present: a frame is held in Device::pr_ptr, and a float copy of it in Device::pr_float
    bool pr_valid = false, pr_float_valid = false;
    // rt_reach_tiles: the rp_gen of the result the reach records in Device::rf_tiles were made from, 0 when none are held
    uint32_t rf_rp_gen = 0;
    // rt_noise_tiles: likewise for the noise records in Device::nz_tiles
    uint32_t nz_rp_gen = 0;
    // the first device's staged colours of the last launch (rt_debug_read_samples): frames, sparse flags
    int staged_frames = 0;
    bool staged_sparse = false;
    // gathers (rt_read_image of a multi-device context, rt_gather_image): RT_GATHER_*
    int gather_path = -1;
    bool comm_tried = false;     // ncclCommInitAll of a multi-device context attempted
    bool proc_comm = false;      // rt_comm_init: one rank of a multi-process communicator
    bool comm_nonblocking = false;   // ... made non-blocking (ncclConfig_t.blocking = 0)
    int comm_timeout_ms = 120000;    // rt_comm_set_timeout: deadline of rt_comm_init / rt_gather_image (0: none)
};

namespace rt_impl __attribute__((visibility("hidden"))) {

inline int set_err(rt_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}

#define HIPCHK(ctx, call)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return set_err(ctx, RT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

// Every host<->device transfer and fill is ordered on the device's render stream
// (which may be non-blocking or caller-owned) and completed before returning, so
// it can neither overlap a queued render nor race the next one.
inline int h2d(rt_ctx* c, Device& d, void* dst, const void* src, size_t n) {
    if (!n) return RT_OK;
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return RT_OK;
}
inline int d2h(rt_ctx* c, Device& d, void* dst, const void* src, size_t n) {
    if (!n) return RT_OK;
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return RT_OK;
}

inline int dev_alloc_copy(rt_ctx* c, Device& d, DevBuf& b, const void* src, size_t n) {
    HIPCHK(c, hipSetDevice(d.id));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    if (b.ptr && b.bytes < n) {
        HIPCHK(c, hipFree(b.ptr));
        b.ptr = nullptr;
        b.bytes = 0;
    }
    if (!b.ptr && n > 0) {
        HIPCHK(c, hipMalloc(&b.ptr, n));
        b.bytes = n;
    }
    return h2d(c, d, b.ptr, src, n);
}

inline void dev_free(DevBuf& b) {
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.bytes = 0;
}

inline int alloc_image(rt_ctx* c, Device& d) {
    HIPCHK(c, hipSetDevice(d.id));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    d.local_rows = local_rows_of(c->height, d.rank, d.world, c->stripe_rows);
    d.padded_rows = padded_rows_of(c->height, d.world, c->stripe_rows);
    size_t bytes = (size_t)d.padded_rows * c->width * 16;
    dev_free(d.image);
    if (bytes) {
        HIPCHK(c, hipMalloc(&d.image.ptr, bytes));
        d.image.bytes = bytes;
        HIPCHK(c, hipMemsetAsync(d.image.ptr, 0, bytes, d.stream));
        HIPCHK(c, hipStreamSynchronize(d.stream));
    }
    d.image_ptr = (float*)d.image.ptr;
    d.image_bound = false;
    return RT_OK;
}

// The second-moment buffer of the current image size, zero-filled; the moments become invalid.
inline int alloc_moments(rt_ctx* c, Device& d) {
    HIPCHK(c, hipSetDevice(d.id));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    c->moments_frames = 0;
    c->tile_frames.clear();
    dev_free(d.m2);
    dev_free(d.tile_sums);
    const size_t bytes = (size_t)d.local_rows * c->width * 16;
    if (!bytes) return RT_OK;
    HIPCHK(c, hipMalloc(&d.m2.ptr, bytes));
    d.m2.bytes = bytes;
    HIPCHK(c, hipMemsetAsync(d.m2.ptr, 0, bytes, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return RT_OK;
}

inline int ensure(rt_ctx* c, Device& d, DevBuf& b, size_t n) {
    if (b.bytes >= n) return RT_OK;
    dev_free(b);
    HIPCHK(c, hipSetDevice(d.id));
    HIPCHK(c, hipMalloc(&b.ptr, n));
    b.bytes = n;
    return RT_OK;
}

// the device's copies of the scene in the kernel arguments (a.perlin_packed decides perlin_pk)
inline void bind_scene(const Device& d, rt_kernel_args& a) {
    a.nodes = (const rt_dnode*)d.nodes.ptr;
    a.spheres = (const rt_sphere*)d.spheres.ptr;
    a.quads = (const rt_quad*)d.quads.ptr;
    a.boxes = (const rt_box*)d.boxes.ptr;
    a.dquads = (const float4*)d.dquads.ptr;
    a.dboxes = (const float4*)d.dboxes.ptr;
    a.dboxc = (const float4*)d.dboxc.ptr;
    a.perlin_pk = a.perlin_packed ? (const float4*)d.perlin_pk.ptr : nullptr;
    a.media = (const rt_medium*)d.media.ptr;
    a.lights = (const int32_t*)d.lights.ptr;
    for (int t = 0; t < 8; t++) a.tex[t].data = d.tex[t].ptr;
}

// validate(SceneState&) of rt_args.h with its error text in the context
inline int validate(rt_ctx* c) { return validate(*c, &c->err); }
// rt_comm.hip (the RCCL table and its state stay in that unit)
int device_gather(rt_ctx* c);
void comm_destroy(Device& d);   // rt_destroy: frees the device's communicator, if any
// rt_reproject.hip: the current per-tile frame counts (nt of them) in Device::rp_counts, copied when they differ
// from the ones it holds; `what` names the caller in the message (rt_present's RT_PRESENT_MOVED reads them too)
int reproject_upload_counts(rt_ctx* c, Device& d, int nt, const char* what);

}  // namespace rt_impl
