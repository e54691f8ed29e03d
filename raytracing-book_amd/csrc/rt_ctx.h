// rt_ctx.h — the context behind the C ABI's rt_ctx handle and the device helpers its
// translation units share (rt_capi.hip, rt_comm.hip, rt_debug.hip).  Internal to the libraries.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include <rccl/rccl.h>   // types only: librccl (~570 MB) is dlopen'ed by the first gather that uses it

#include "rt/rt.h"
#include "rt/rt_debug.h"
#include "rt/rt_types.h"
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

struct rt_ctx {
    std::vector<Device> devs;
    std::string err;
    // host copies of what the kernel needs
    std::vector<uint8_t> host_buf[6];
    bool uploaded[6] = {false, false, false, false, false, false};
    int tex_format[8] = {0}, tex_w[8] = {0}, tex_h[8] = {0};
    rt_camera_ubo cam{};
    bool have_cam = false;
    int max_depth = 5;
    float background[3] = {0, 0, 0};
    float sqrt_spp = 1.0f, recip_sqrt_spp = 1.0f;
    int width = 0, height = 0;
    int proc_rank = 0, proc_world = 1, stripe_rows = 16;
    int n_dnodes = 0;
    std::vector<rt_dnode> dnodes;   // host copy of the threaded BVH (fast-walk tables are built from it)
    // the BVH the link walk runs on (rt_set_bvh_mode): the uploaded one (RT_BVH_REFERENCE), or the
    // binned-SAH tree built from its prims at validation (RT_BVH_SAH, non-parity fast mode, bvh_sah.h)
    int bvh_mode = RT_BVH_REFERENCE;
    int n_link_nodes = 0;
    std::vector<uint8_t> sah_bvh;   // the SAH tree in the reference's node format (rt_debug_walk_bvh)
    std::vector<rt_dnode> walk_dn;  // threaded nodes of the BVH the link walk uses (reference or SAH)
    // the links the launch walks: c->links, or (option box_vnodes) the same with every all-box leaf's
    // box pre-tests as nodes of the walk (build_links with vbox); rebuilt when the margin changes
    std::vector<float4> walk_links;
    int n_walk_nodes = 0;
    bool walk_v = false;
    float walk_v_margin = -1.0f;
    bool walk_stale = true;
    std::vector<float4> boxc_host;  // the compact box records (host copy of Device::dboxc)
    bool box_vnodes = true;         // option box_vnodes
    bool box_interior = true;       // option box_interior
    bool zero_dir_end = true;       // option zero_dir_end (rt_kernel.hip render_stream)
    bool first_leaf = true;         // option first_leaf: a walk that starts at the spine's leaf tests it where
                                    // it begins (rt_kernel.hip render_stream; the RT_OPT_BOXQ kernels)
    int first_leaf_last[4] = {0};   // rt_debug_first_leaf: the last launch's (armed, leaf link, type byte, prims)
    bool collapse = true;           // option collapse: the walk leaves out inner nodes (plan_collapse)
    int rebuild = 2;                // option rebuild: the walk's inner nodes rebuilt over its leaves (rebuild_inner mode)
    bool walk_r = false;            // walk_links were built on the rebuilt inner nodes
    int walk_rmode = 0;             // ... of this mode
    std::vector<rt_dnode> rb_dn;    // rebuild_inner(walk_dn, rb_mode), kept across camera moves
    int rb_mode = -1;               // -1: not built for the current walk_dn
    bool walk_c = false;            // walk_links were built with a collapse plan ...
    rt_camera_ubo walk_cam{};       // ... for this camera and image size
    int walk_w = 0, walk_h = 0;
    int n_dropped = 0;              // inner nodes the walk leaves out
    int n_rebuilt = 0;              // nodes of the rebuilt tree (0: the tree as uploaded / built)
    int n_vnodes = 0;               // box pre-test nodes in walk_links
    FastTables fast;
    std::vector<float4> links;   // build_links(dnodes), empty when unavailable
    int fast_gen = 0;
    bool spec_ok = false;   // every child box lies inside its parent's (the near-first walk needs it)
    int debug_flags = 0;    // env RT_DEBUG_FLAGS: ablation runs only (bit 0: Perlin -> 0.5; bit 3: compact boxes hit on their planes alone)
    bool uv_always = false;
    bool boxes_canon = false;   // every box has Box.java's axis-aligned face layout (dboxes[18..20])
    bool fd_ok[6] = {true, true, true, true, true, true};   // per binding: records in the fast-division regime
    bool fd_cam = true;
    bool boxes_cond = false;   // every box face's 2-D Cramer system is well conditioned (box pre-test)
    float scene_extent = -1.0f;   // max |coordinate| over records and camera (< 0: not computed)
    bool validated = false;
    uint64_t last_ns = 0;
    int variant = 0;   // kernel structure variant (env RT_KERNEL_VARIANT; A/B only)
    int variant_no_stats = -1;   // the variant active before rt_debug_enable_stats(c, 1), restored by (c, 0)
    // the collapse plan from measured node hits (rt_debug_set_collapse_hits): per node of the walk's
    // tree in its breadth-first link order, the box tests that hit, and the walks begun at the root
    std::vector<int64_t> inj_hits;
    int64_t inj_walks = 0;
    // Work split: aim for chunk_target work units per resident wave (env
    // RT_CHUNK_TARGET; 0 = one chunk per tile), staged_chunk_target when staged
    // (RT_STAGED_CHUNK_TARGET).  With at least stage_tiles tiles
    // per resident wave (env RT_STAGE_TILES) the chunks are ordered (the running
    // mean is handed from wave to wave, rt_kernel.hip wait_chunk); with fewer, a
    // tile's frames would be one long serial chain, so the chunks run in parallel,
    // stage their per-frame colours (at most sample_budget bytes) and the fold (rt_moments.hip)
    // applies the running mean in frame order.  The default stage_tiles stages
    // every chunked launch: with render_stream that measured fastest at N = 1 too
    // (scene 8 -5% against ordered chunks).
    int chunk_target = 16;          // ordered chunks (RT_CHUNK_TARGET)
    int staged_chunk_target = 48;   // staged chunks (RT_STAGED_CHUNK_TARGET)
    int tail_chunks = -1;           // option tail_chunks: staged launches end with this many one-frame chunks
                                    // (-1: tail_chunks_for the tree)
    int stage_tiles = 1 << 20;      // in effect always staged (the measured best with render_stream)
    bool fastdiv = true;   // shared-reciprocal divisions where exact (env RT_FASTDIV=0 disables; A/B)
    bool box_pretest = true;   // the canonical box tests' bounds pre-test (env RT_BOX_PRETEST=0 disables; A/B)
    int sm_batch = 64;   // render_stream's shading batch (env RT_SM_BATCH) ...
    int sm_frac = 0;     // ... or fraction of the lanes with a walk, in 64ths (env RT_SM_FRAC); 0 = by kernel:
                         // 50 for the compact-box kernels (scene 8 1080p -1.1%, 4K -1.6% against 56), 56 else
                         // (scene 6 +1.4% at 52; profiles/r03_sm_frac_knobs.log)
    bool shade_lds = true;       // shading tables in LDS (sphere / box materials, small textures; option):
                                 // scenes 8 / 0 / 6 -0.3 / -1.0 / -1.2% (profiles/r04_shade_lds_ab_s*.log)
    bool tl_small_lds = true;    // two-level walk: small sphere / box tables staged beside the top levels (option)
    bool leaf_prefetch = true;   // leaf records prefetched before the type blocks when all are in LDS (option)
    int walk_frac = 0;   // render_stream: node walks stop at this fraction of lanes ready, in 64ths (env RT_WALK_FRAC);
                         // 0 = by BVH size: 8 up to 64 nodes, 32 up to 1024, 48 above (walk_frac_for)
    bool big_wg = true;    // 1024-thread workgroups with sphere + box records in LDS when they fit (env RT_BIG_WG=0: A/B)
    bool sph_lds = true;   // sphere records' first two float4 in LDS when they fit (env RT_SPH_LDS=0 disables; A/B)
    bool compact_boxes = true;   // boxes' compact records when every box has one (box_test_compact; option 0: A/B)
    bool spine = true;           // walks start past the spine when they hit it for sure (plan_spine)
    int lds_node_cap = 0;        // bytes of BVH nodes staged in LDS, 0 = as many as fit (tests: force the two-level walk)
    bool tl_leaf_lds = true;     // two-level walk: the leaf records in LDS beside the top levels (when they fit)
    int perlin_pk_slot = -1;     // texture slot whose Perlin table has its packed copy (Device::perlin_pk)
    bool sparse_stage = true;    // staged chunks store only the colours that are not exactly zero (option)
    int sphere_pairs = 1;        // the sphere-pair kernels when most leaves hold two spheres (option; 2: always,
                                 // compact-box kernels included)
    int pair_leaves = -1;        // per mille of the link-format leaves that hold two spheres (< 0: not counted)
    bool perlin_pk = true;       // stage the packed Perlin table (option; else the texture as uploaded)
    int n_boxc_ok = 0;           // boxes whose compact record reproduces their faces
    unsigned long long watchdog_ticks = 120ull * 100000000ull;     // render_stream progress bound (100 MHz ticks)
    unsigned long long chunk_wait_ticks = 30ull * 100000000ull;    // ordered-chunk wait bound
    size_t sample_budget = (size_t)32 << 30;   // staged colours per launch, at most (and at most half the free memory)
    int last_launch[RT_LI_N] = {0};
    bool launched = false;
    // Sample moments (rt_set_moments; single-device contexts): every launch is staged and folded by
    // the fold with the moments.  moments_frames = the frames 1 .. n whose moments Device::m2 holds, 0 =
    // invalid (nothing rendered yet, a first_frame gap, the image overwritten or resized).
    bool moments = false;
    int moments_frames = 0;
    // Per-tile frame counts (rt_read_tile_frames): the frames 1 .. n each 8x8 tile of the first device's
    // image holds, 0 = invalid.  While every tile holds the same count tile_frames is empty and
    // moments_frames is that count; once they differ (a launch under a tile mask) tile_frames holds
    // one count per tile and moments_frames their minimum, so "valid" stays moments_frames >= 1.
    // Single-device contexts keep them whether or not the moments are on.
    std::vector<int32_t> tile_frames;
    // rt_set_active_tiles: the mask in effect (mask_set), its tiles' indices in ascending order
    // (Device::tile_list holds the same on the device)
    bool mask_set = false;
    std::vector<int32_t> act_list;
    // rt_denoise: which of Device::dn_px holds the filtered image (-1: none held), and the per-tile
    // counts last copied to Device::dn_counts (copied again only when they change)
    int dn_result = -1;
    std::vector<int32_t> dn_counts;
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

// rt_capi.hip: checks the uploaded records against each other and derives the walk's trees
int validate(rt_ctx* c);
// rt_comm.hip (the RCCL table and its state stay in that unit)
int device_gather(rt_ctx* c);
void comm_destroy(Device& d);   // rt_destroy: frees the device's communicator, if any

}  // namespace rt_impl
