// rt_capi.hip — implementation of include/rt/rt.h (the drop-in C ABI).
//
// Host-side responsibilities that the reference's Java/GL layer had:
// buffer/texture upload (BufferObject.uploadData, Texture.putData), uniforms
// (ShaderProgram.setUniform*), dispatch (RaytraceExecutor.raytrace), readback
// (glGetTexImage) and timing (QueryTimer).  Plus the MI355X-specific parts:
// RGB8->RGBA8 texture expansion, stripe partitioning across devices/processes
// and caller-owned device images.  The scene preparation (the threaded-BVH
// re-layout among it) is rt_prep.cpp, the launch planning rt_plan.cpp, the way from
// the scene to the kernel arguments (everything here that needs no device) rt_args.cpp, RCCL
// rt_comm.hip, the debug hooks rt_debug.hip and rt_debug_host.cpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_ctx.h"
#include "rt_denoise.h"
#include "rt_plan.h"
#include "rt_present.h"
#include "rt_refine.h"
#include "rt_reproject.h"

using namespace rt_impl;

namespace {

// every tile holds frames 1 .. n (0: none valid): the uniform form of the per-tile counts (rt_ctx.h)
void set_all_frames(rt_ctx* c, int n) {
    c->moments_frames = n;
    c->tile_frames.clear();
}

// the device's copies of the scene (bind_scene), its image, counters and stripe in the kernel arguments
void bind_device(const rt_ctx* c, const Device& d, rt_kernel_args& a) {
    bind_scene(d, a);
    a.image = d.image_ptr;
    a.stats = (unsigned long long*)d.stats.ptr;
    a.census = (unsigned*)d.census.ptr;
    a.census_cap = d.census_cap;
    a.node_hits = (unsigned*)d.node_hits.ptr;
    a.census_waves = d.census_waves;
    a.local_rows = d.local_rows;
    a.rank = d.rank;
    a.world = d.world;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

// Failure of the last context-less call (rt_create) on this thread; rt_last_error(NULL).
namespace { thread_local std::string g_create_err; }

int rt_create(int n_devices, const int* device_ids, rt_ctx** out) {
    auto fail = [](int code, const char* msg) { g_create_err = msg; return code; };
    if (!out) return fail(RT_ERR_INVALID_ARG, "rt_create: NULL out");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(RT_ERR_DEVICE, "rt_create: no HIP device");
    // Explicit ids may repeat (several stripe slots on one device); without ids, devices 0..n-1.
    if (n_devices <= 0 || n_devices > 64 || (!device_ids && n_devices > count))
        return fail(RT_ERR_INVALID_ARG, "rt_create: bad device count");
    rt_ctx* c = new rt_ctx();
#ifdef RT_AB_KNOBS
    // A/B build only: the structure variants and knobs from the environment (tools/ab_variants.py).
    // The release library reads no environment: its output depends on its inputs alone.
    if (const char* v = std::getenv("RT_KERNEL_VARIANT")) {
        // 0 (default), 37, 30, 61 and their stats twins 39, 38, 31, 69
        // (rt_kernel.hip rt_launch_render); anything else is the default
        const int want = std::atoi(v);
        c->variant = (want == 30 || want == 31 || want == 37 || want == 38 || want == 39 || want == 61 || want == 69)
                         ? want
                         : 0;
    }
    if (const char* v = std::getenv("RT_CHUNK_TARGET")) c->chunk_target = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("RT_STAGE_TILES")) c->stage_tiles = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("RT_STAGED_CHUNK_TARGET")) c->staged_chunk_target = std::max(1, std::atoi(v));
    if (const char* v = std::getenv("RT_FASTDIV")) c->fastdiv = std::atoi(v) != 0;
    if (const char* v = std::getenv("RT_BOX_PRETEST")) c->box_pretest = std::atoi(v) != 0;
    if (const char* v = std::getenv("RT_SM_BATCH")) c->sm_batch = std::max(1, std::min(64, std::atoi(v)));
    if (const char* v = std::getenv("RT_SM_FRAC")) c->sm_frac = std::max(1, std::min(64, std::atoi(v)));
    if (const char* v = std::getenv("RT_WALK_FRAC")) c->walk_frac = std::max(1, std::min(64, std::atoi(v)));
    if (const char* v = std::getenv("RT_SPH_LDS")) c->sph_lds = std::atoi(v) != 0;
    if (const char* v = std::getenv("RT_BIG_WG")) c->big_wg = std::atoi(v) != 0;
    if (const char* v = std::getenv("RT_COMPACT_BOXES")) c->compact_boxes = std::atoi(v) != 0;
    if (const char* v = std::getenv("RT_LDS_NODE_CAP")) c->lds_node_cap = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("RT_DEBUG_FLAGS")) c->debug_flags = std::atoi(v);
#endif
    c->devs.resize(n_devices);
    for (int i = 0; i < n_devices; i++) {
        Device& d = c->devs[i];
        d.id = device_ids ? device_ids[i] : i;
        if (d.id < 0 || d.id >= count) { delete c; return fail(RT_ERR_INVALID_ARG, "rt_create: device id out of range"); }
        d.rank = i;
        d.world = n_devices;
        if (hipSetDevice(d.id) != hipSuccess || hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreate(&d.ev_start) != hipSuccess || hipEventCreate(&d.ev_stop) != hipSuccess) {
            delete c;
            return fail(RT_ERR_DEVICE, "rt_create: stream/event creation failed");
        }
    }
    g_create_err.clear();
    *out = c;
    return RT_OK;
}

int rt_destroy(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID_ARG;
    for (Device& d : c->devs) {
        (void)hipSetDevice(d.id);
        (void)hipStreamSynchronize(d.stream);
        dev_free(d.nodes); dev_free(d.spheres); dev_free(d.quads); dev_free(d.boxes); dev_free(d.media);
        dev_free(d.lights); dev_free(d.image); dev_free(d.args); dev_free(d.stats); dev_free(d.census); dev_free(d.counter);
        dev_free(d.tile_done); dev_free(d.samples); dev_free(d.wbuf); dev_free(d.dquads); dev_free(d.dboxes);
        dev_free(d.finfo); dev_free(d.f2inner); dev_free(d.f2leaves); dev_free(d.links); dev_free(d.dboxc);
        dev_free(d.gather); dev_free(d.full); dev_free(d.perlin_pk); dev_free(d.sflags);
        dev_free(d.m2); dev_free(d.tile_sums); dev_free(d.node_hits); dev_free(d.tile_list);
        dev_free(d.dn_px[0]); dev_free(d.dn_px[1]); dev_free(d.dn_vb); dev_free(d.dn_counts);
        dev_free(d.ft_nd); dev_free(d.ft_ai); dev_free(d.ft_links); dev_free(d.ft_args);
        dev_free(d.hs_px); dev_free(d.hs_nd); dev_free(d.hs_ai); dev_free(d.rp_out); dev_free(d.rp_counts);
        dev_free(d.hs_s2); dev_free(d.rp_s2); dev_free(d.pr_out); dev_free(d.pr_float); dev_free(d.pr_lut);
        dev_free(d.rf_tiles); dev_free(d.nz_tiles);
        comm_destroy(d);
        if (d.ring) (void)hipHostFree(d.ring);
        for (auto& e : d.ring_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& t : d.tex) dev_free(t);
        if (d.ev_start) (void)hipEventDestroy(d.ev_start);
        if (d.ev_stop) (void)hipEventDestroy(d.ev_stop);
        if (d.own_stream && d.stream) (void)hipStreamDestroy(d.stream);
    }
    delete c;
    return RT_OK;
}

const char* rt_last_error(rt_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int rt_upload_buffer(rt_ctx* c, int binding, const void* bytes, size_t nbytes) {
    if (!c) return RT_ERR_INVALID_ARG;
    BufferPrep p;
    int r = prep_buffer(*c, binding, bytes, nbytes, p, &c->err);
    if (r) return r;
    c->ft_valid = c->ft_links_ok = false;   // the first-hit buffers are another scene's now
    history_drop(c);                        // ... and the history's ids no longer mean the same surfaces
    for (Device& d : c->devs) {
        DevBuf* b = nullptr;
        switch (binding) {
            case RT_BIND_SPHERES: b = &d.spheres; break;
            case RT_BIND_BVH: b = &d.nodes; break;
            case RT_BIND_QUADS: b = &d.quads; break;
            case RT_BIND_MEDIA: b = &d.media; break;
            case RT_BIND_BOXES: b = &d.boxes; break;
            default: b = &d.lights; break;
        }
        r = dev_alloc_copy(c, d, *b, p.src, p.n);
        if (r) return r;
        if (binding == RT_BIND_QUADS || binding == RT_BIND_BOXES) {
            r = dev_alloc_copy(c, d, binding == RT_BIND_QUADS ? d.dquads : d.dboxes, p.faces.data(),
                               p.faces.size() * sizeof(float4));
            if (r) return r;
        }
        if (binding == RT_BIND_BOXES) {
            r = dev_alloc_copy(c, d, d.dboxc, p.boxc.data(), p.boxc.size() * sizeof(float4));
            if (r) return r;
        }
    }
    return RT_OK;
}

int rt_upload_texture(rt_ctx* c, int slot, int format, int w, int h, const void* texels) {
    if (!c) return RT_ERR_INVALID_ARG;
    TexturePrep p;
    int r = prep_texture(slot, format, w, h, texels, p, &c->err);
    if (r) return r;
    c->ft_valid = false;   // the first-hit albedo was another texture's
    history_drop(c);       // ... and so was what the history had accumulated
    for (Device& d : c->devs) {
        r = dev_alloc_copy(c, d, d.tex[slot], p.src, p.bytes);
        if (r) return r;
        if (!p.pk.empty()) {
            r = dev_alloc_copy(c, d, d.perlin_pk, p.pk.data(), p.pk.size() * sizeof(float4));
            if (r) return r;
        }
    }
    set_texture(*c, slot, format, w, h, !p.pk.empty());
    return RT_OK;
}

int rt_set_camera(rt_ctx* c, const float ubo[28]) {
    if (!c || !ubo) return set_err(c, RT_ERR_INVALID_ARG, "NULL camera");
    set_camera(*c, ubo);
    c->ft_valid = c->ft_links_ok = false;   // the first-hit buffers were another camera's (and under RT_BVH_SAH another tree's)
    return RT_OK;
}

int rt_set_params(rt_ctx* c, int max_depth, const float background[3], float sqrt_spp, float recip_sqrt_spp) {
    if (!c || !background) return set_err(c, RT_ERR_INVALID_ARG, "NULL background");
    if (max_depth < 0) return set_err(c, RT_ERR_INVALID_ARG, "max_depth must be >= 0");
    c->max_depth = max_depth;
    std::memcpy(c->background, background, 12);
    c->sqrt_spp = sqrt_spp;
    c->recip_sqrt_spp = recip_sqrt_spp;
    return RT_OK;
}

int rt_set_partition(rt_ctx* c, int rank, int world, int stripe_rows) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (world < 1 || rank < 0 || rank >= world || stripe_rows < 1) return set_err(c, RT_ERR_INVALID_ARG, "bad partition");
    if (world > 1 && c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "process partition needs a 1-device context");
    c->proc_rank = rank;
    c->proc_world = world;
    c->stripe_rows = stripe_rows;
    if (c->devs.size() == 1) {
        c->devs[0].rank = rank;
        c->devs[0].world = world;
    }
    if (c->width > 0) return rt_resize(c, c->width, c->height);
    return RT_OK;
}

int rt_resize(rt_ctx* c, int w, int h) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (w <= 0 || h <= 0 || w > RT_MAX_IMAGE_DIM || h > RT_MAX_IMAGE_DIM || (size_t)w * h > ((size_t)1 << 30))
        return set_err(c, RT_ERR_INVALID_ARG, "bad image size");
    c->width = w;
    c->height = h;
    for (Device& d : c->devs) {
        int r = alloc_image(c, d);
        if (r) return r;
    }
    c->staged_frames = 0;
    denoise_free(c);        // (alloc_image left every stream idle) the filtered image was the old size's
    features_free(c);       // ... and so were the first-hit buffers
    reproject_free(c);      // ... the history and the reprojected result
    present_free(c);        // ... and the presented frame (a bound frame buffer was the old size's too)
    refine_free(c);         // ... and the reach and noise records
    set_all_frames(c, 0);   // another image: no tile holds a frame, and a tile mask no longer fits it
    c->mask_set = false;
    c->act_list.clear();
    if (c->moments) return alloc_moments(c, c->devs[0]);
    return RT_OK;
}

int rt_bind_device_image(rt_ctx* c, void* ptr, size_t nbytes) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "device image binding needs a 1-device context");
    Device& d = c->devs[0];
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "rt_resize first");
    set_all_frames(c, 0);   // another image: its moments are not the ones held
    if (!ptr) {
        d.image_ptr = (float*)d.image.ptr;
        d.image_bound = false;
        return RT_OK;
    }
    if (nbytes < (size_t)d.local_rows * c->width * 16) return set_err(c, RT_ERR_INVALID_ARG, "device image too small");
    d.image_ptr = (float*)ptr;
    d.image_bound = true;
    return RT_OK;
}

int rt_set_stream(rt_ctx* c, void* stream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "stream binding needs a 1-device context");
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    if (d.own_stream && d.stream) HIPCHK(c, hipStreamSynchronize(d.stream));
    if (!stream) {
        if (!d.own_stream) {
            HIPCHK(c, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
            d.own_stream = true;
        }
        return RT_OK;
    }
    if (d.own_stream && d.stream) HIPCHK(c, hipStreamDestroy(d.stream));
    d.stream = (hipStream_t)stream;
    d.own_stream = false;
    return RT_OK;
}

namespace {

// One device's part of rt_render: its buffers, the unit split, and the launches of the frame range.
// a: the scene's arguments (scene_args); mom: the launches fold the moments too.
int render_device(rt_ctx* c, Device& d, rt_kernel_args& a, bool mom, int first_frame, int n_frames,
                  const float* rand_factors) {
    int r;
    HIPCHK(c, hipSetDevice(d.id));
    const bool first_dev = &d == &c->devs[0];
    if (c->mask_set && c->act_list.empty()) {
        // no tile to sample: nothing is launched or read; the events keep rt_sync / rt_last_render_ns working
        HIPCHK(c, hipEventRecord(d.ev_start, d.stream));
        HIPCHK(c, hipEventRecord(d.ev_stop, d.stream));
        d.timed = true;
        c->last_launch[RT_LI_TILES_ACTIVE] = 0;   // (the other fields keep the previous launch's)
        c->launched = c->launched || n_frames > 0;
        return RT_OK;
    }
    bind_device(c, d, a);
    if (!d.args.ptr) {
        if ((r = ensure(c, d, d.counter, 256))) return r;
        HIPCHK(c, hipMemsetAsync(d.counter.ptr, 0, 256, d.stream));
        if ((r = ensure(c, d, d.args, sizeof(rt_kernel_args)))) return r;
        HIPCHK(c, hipHostMalloc((void**)&d.ring, sizeof(rt_kernel_args) * Device::kRing, hipHostMallocDefault));
        for (auto& e : d.ring_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    a.tile_counter = (int*)d.counter.ptr;
    if (d.fast_gen != c->fast_gen) {
        const FastTables& F = c->fast;
        int rf = dev_alloc_copy(c, d, d.finfo, F.info.data(), F.info.size() * sizeof(uint32_t));
        if (!rf) rf = dev_alloc_copy(c, d, d.f2inner, F.inner2.data(), F.inner2.size() * sizeof(float4));
        if (!rf) rf = dev_alloc_copy(c, d, d.f2leaves, F.leaves2.data(), F.leaves2.size() * sizeof(uint2));
        if (!rf) rf = dev_alloc_copy(c, d, d.links, c->walk_links.data(), c->walk_links.size() * sizeof(float4));
        if (rf) return rf;
        d.fast_gen = c->fast_gen;
    }
    a.finfo = (const uint32_t*)d.finfo.ptr;
    a.f2inner = (const float4*)d.f2inner.ptr;
    a.f2leaves = (const uint2*)d.f2leaves.ptr;
    a.lnodes = (const float4*)d.links.ptr;
    // frames per launch and the unit split (plan_device); a staged launch's colours take at most
    // half the device's free memory (what this context already holds counts as free)
    const long long waves = rt_resident_waves();
    size_t free_b = 0, total_b = 0;
    const size_t avail = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b + d.samples.bytes : SIZE_MAX;
    const Split split = plan_device(*c, d.local_rows, waves, avail, mom, n_frames, a);
    a.tile_list = c->mask_set ? (const int*)d.tile_list.ptr : nullptr;
    a.fault = (unsigned*)d.counter.ptr + 1;
    HIPCHK(c, hipEventRecord(d.ev_start, d.stream));
    for (int f0 = 0; f0 < n_frames; f0 += split.per_launch) {
        const LaunchPlan p = plan_launch(*c, split, mom, waves, first_frame, n_frames, f0, a);
        if (split.staged && (r = ensure(c, d, d.samples, a.n_pixels * sizeof(float4) * p.launch_frames))) return r;
        if (!split.staged && split.chunks_wanted > 1 &&
            (r = ensure(c, d, d.tile_done, sizeof(unsigned) * (size_t)tile_count(c->width, d.local_rows))))
            return r;
        a.tile_done = (unsigned*)d.tile_done.ptr;
        a.samples = p.stage ? (float4*)d.samples.ptr : nullptr;
        a.sflags = nullptr;
        if (p.sparse) {
            if ((r = ensure(c, d, d.sflags, a.n_pixels * p.launch_frames))) return r;
            a.sflags = (uint8_t*)d.sflags.ptr;
        }
        a.wbuf = nullptr;
        if (p.wave_slots) {
            if ((r = ensure(c, d, d.wbuf, (size_t)waves * 2 * 64 * (size_t)a.chunk_frames * sizeof(float4)))) return r;
            a.wbuf = (float4*)d.wbuf.ptr;
        }
        std::memcpy(a.rand_factors, rand_factors + f0, sizeof(float) * a.n_frames);
        int slot = d.ring_pos++ % Device::kRing;
        HIPCHK(c, hipEventSynchronize(d.ring_ev[slot]));   // the copy that last used this slot is done
        d.ring[slot] = a;
        if (rt_launch_render(d.ring[slot], (rt_kernel_args*)d.args.ptr, d.stream, first_dev ? c->last_launch : nullptr,
                             mom ? d.m2.ptr : nullptr))
            return set_err(c, RT_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
        HIPCHK(c, hipEventRecord(d.ring_ev[slot], d.stream));
        if (first_dev) {
            c->staged_frames = a.samples ? a.n_frames : 0;
            c->staged_sparse = a.samples && a.sflags;
            launch_report(*c, a, c->last_launch, c->first_leaf_last);
        }
    }
    HIPCHK(c, hipEventRecord(d.ev_stop, d.stream));
    d.timed = true;
    c->launched = c->launched || n_frames > 0;
    return RT_OK;
}

}  // namespace

int rt_render(rt_ctx* c, int first_frame, int n_frames, const float* rand_factors) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (first_frame < 1 || n_frames < 0 || (n_frames > 0 && !rand_factors))
        return set_err(c, RT_ERR_INVALID_ARG, "first_frame >= 1, n_frames >= 0, rand_factors required");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "rt_resize before rt_render");
    if (!c->have_cam) return set_err(c, RT_ERR_STATE, "rt_set_camera before rt_render");
    if (!c->uploaded[RT_BIND_BVH]) return set_err(c, RT_ERR_STATE, "no BVH uploaded");
    // u_rand_factor is (float)Math.random() in the reference (RaytraceExecutor.java:124-127).
    // rand() adds 0.001 to it per call (random.glsl:2-7): a NaN / inf, or a value so large
    // that the addition no longer changes it, would freeze rand() and keep a rejection
    // loop (random.glsl:19-24, 40-45) spinning on the device forever
    for (int i = 0; i < n_frames; i++)
        if (!(std::fabs(rand_factors[i]) <= RT_MAX_RAND_FACTOR))
            return set_err(c, RT_ERR_INVALID_ARG, "rand_factors must be finite with |value| <= 1024");
    int r = validate(c);
    if (r) return r;
    rt_kernel_args a;
    if ((r = scene_args(*c, a, &c->err))) return r;
    // Sample moments: every launch staged (one frame or one chunk too) and folded by
    // fold_moments_kernel.  The moments follow frames 1 .. moments_frames: a render from frame 1
    // restarts them (the fold zeroes them at frame 1), one from moments_frames + 1 extends them,
    // any other leaves them invalid.
    const int rows0 = c->devs[0].local_rows;
    const bool mom = c->moments && n_frames > 0 && rows0 > 0;   // (a rank may own no row)
    if (mom && !c->devs[0].m2.ptr) return set_err(c, RT_ERR_STATE, "sample moments: no buffer (rt_resize)");
    // A tile mask (rt_set_active_tiles): the units run over the active tiles alone.
    if (c->mask_set && !pooled_variant(c->variant))
        return set_err(c, RT_ERR_STATE, "a tile mask runs on the default kernel structure only");
    // The per-tile frame counts of the tiles this call samples (step_frame_counts); a single-device
    // context keeps them with the moments off too (the image's frames).
    const bool track = (mom || c->devs.size() == 1) && n_frames > 0 && rows0 > 0;
    FrameCounts after;
    if (track) {
        after = step_frame_counts(c->moments_frames, c->tile_frames, tile_count(c->width, rows0),
                                  c->mask_set ? &c->act_list : nullptr, first_frame, n_frames);
        if (!c->mask_set || !c->act_list.empty()) set_all_frames(c, 0);   // until every launch is queued
    }
    for (Device& d : c->devs)
        if ((r = render_device(c, d, a, mom, first_frame, n_frames, rand_factors))) return r;
    if (track) {
        c->moments_frames = after.all;
        c->tile_frames.swap(after.tiles);
    }
    return RT_OK;
}

int rt_sync(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID_ARG;
    for (Device& d : c->devs) {
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        if (d.counter.ptr) {   // fault word: an ordered-chunk wait timed out (never expected)
            unsigned fault = 0;
            HIPCHK(c, hipMemcpy(&fault, (unsigned*)d.counter.ptr + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (fault) {
                HIPCHK(c, hipMemset((unsigned*)d.counter.ptr + 1, 0, sizeof(unsigned)));
                return set_err(c, RT_ERR_DEVICE, fault == 2 ? "render kernel: a wave stored no sample within its progress bound (watchdog)"
                                                            : "render kernel: ordered-chunk wait timed out");
            }
        }
    }
    return RT_OK;
}

int rt_last_render_ns(rt_ctx* c, uint64_t* ns) {
    if (!c || !ns) return RT_ERR_INVALID_ARG;
    double mx = 0;
    for (Device& d : c->devs) {
        if (!d.timed) continue;
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipEventSynchronize(d.ev_stop));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, d.ev_start, d.ev_stop));
        mx = std::max(mx, (double)ms);
    }
    *ns = (uint64_t)(mx * 1e6);
    c->last_ns = *ns;
    return RT_OK;
}

int rt_render_done(rt_ctx* c, uint64_t* ns) {
    if (!c || !ns) return RT_ERR_INVALID_ARG;
    double mx = 0;
    for (Device& d : c->devs) {
        if (!d.timed) continue;
        HIPCHK(c, hipSetDevice(d.id));
        const hipError_t q = hipEventQuery(d.ev_stop);
        if (q == hipErrorNotReady) return 0;
        if (q != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, d.ev_start, d.ev_stop));
        mx = std::max(mx, (double)ms);
    }
    *ns = (uint64_t)(mx * 1e6);
    return 1;
}

int rt_read_image(rt_ctx* c, float* rgba) {
    if (!c || !rgba) return RT_ERR_INVALID_ARG;
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "no image");
    int r = rt_sync(c);
    if (r) return r;
    if (c->devs.size() == 1) {
        Device& d = c->devs[0];
        HIPCHK(c, hipSetDevice(d.id));
        return d2h(c, d, rgba, d.image_ptr, (size_t)d.local_rows * c->width * 16);
    }
    // multi-device context: the stripe blocks gathered on device 0 (RCCL when the devices
    // are distinct and RCCL loads, else peer copies), de-interleaved there, one copy out
    if (device_gather(c) == RT_OK) {
        Device& d0 = c->devs[0];
        HIPCHK(c, hipSetDevice(d0.id));
        return d2h(c, d0, rgba, d0.full.ptr, (size_t)c->height * c->width * 16);
    }
    // last resort: every block to the host, de-interleaved there
    int ndev = (int)c->devs.size();
    int padded = padded_rows_of(c->height, ndev, c->stripe_rows);
    std::vector<float> g((size_t)ndev * padded * c->width * 4, 0.0f);
    for (int k = 0; k < ndev; k++) {
        Device& d = c->devs[k];
        HIPCHK(c, hipSetDevice(d.id));
        int r2 = d2h(c, d, g.data() + (size_t)k * padded * c->width * 4, d.image_ptr,
                     (size_t)d.local_rows * c->width * 16);
        if (r2) return r2;
    }
    c->gather_path = RT_GATHER_HOST;
    return rt_deinterleave_rows(g.data(), c->width, c->height, ndev, c->stripe_rows, rgba);
}

int rt_write_image(rt_ctx* c, const float* rgba) {
    if (!c || !rgba) return RT_ERR_INVALID_ARG;
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "no image");
    int r = rt_sync(c);
    if (r) return r;
    set_all_frames(c, 0);   // rt_write_moments restores them from the same checkpoint
    for (Device& d : c->devs) {
        HIPCHK(c, hipSetDevice(d.id));
        std::vector<float> local((size_t)d.local_rows * c->width * 4);
        // pick this device's rows from the (process-local) image
        if (c->devs.size() == 1) {
            int r2 = h2d(c, d, d.image_ptr, rgba, local.size() * 4);
            if (r2) return r2;
            continue;
        }
        int n_stripes = (c->height + c->stripe_rows - 1) / c->stripe_rows;
        size_t lr = 0;
        for (int s = d.rank; s < n_stripes; s += d.world)
            for (int y = s * c->stripe_rows; y < std::min(c->height, (s + 1) * c->stripe_rows); y++, lr++)
                std::memcpy(&local[lr * c->width * 4], rgba + (size_t)y * c->width * 4, (size_t)c->width * 16);
        int r2 = h2d(c, d, d.image_ptr, local.data(), local.size() * 4);
        if (r2) return r2;
    }
    return RT_OK;
}

// ---- sample moments and the noise-target loop (rt.h; kernels in rt_moments.hip) ----

int rt_set_moments(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "sample moments need a 1-device context");
    Device& d = c->devs[0];
    if (!on) {
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        dev_free(d.m2);
        dev_free(d.tile_sums);
        denoise_free(c);
        c->moments = false;
        set_all_frames(c, 0);
        return RT_OK;
    }
    if (c->moments) return RT_OK;
    c->moments = true;
    set_all_frames(c, 0);
    return c->width > 0 ? alloc_moments(c, d) : RT_OK;
}

namespace {
int moments_ready(rt_ctx* c, bool need_valid) {
    if (!c->moments) return set_err(c, RT_ERR_STATE, "rt_set_moments(ctx, 1) first");
    if (c->width <= 0 || !c->devs[0].m2.ptr) return set_err(c, RT_ERR_STATE, "no image");
    if (need_valid && c->moments_frames < 1)
        return set_err(c, RT_ERR_STATE, "the moments are invalid: render from frame 1 (or rt_write_moments)");
    return RT_OK;
}
}  // namespace

int rt_read_moments(rt_ctx* c, float* m2_rgba) {
    if (!c || !m2_rgba) return RT_ERR_INVALID_ARG;
    int r = moments_ready(c, true);
    if (!r) r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, m2_rgba, d.m2.ptr, (size_t)d.local_rows * c->width * 16);
}

int rt_write_moments(rt_ctx* c, const float* m2_rgba, int n_frames) {
    if (!c || !m2_rgba || n_frames < 1) return RT_ERR_INVALID_ARG;
    int r = moments_ready(c, false);
    if (!r) r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    set_all_frames(c, 0);
    r = h2d(c, d, d.m2.ptr, m2_rgba, (size_t)d.local_rows * c->width * 16);
    if (r) return r;
    set_all_frames(c, n_frames);
    return RT_OK;
}

int rt_read_tile_sums(rt_ctx* c, rt_tile_sum* out, int cap, int* n_tiles) {
    if (!c || !n_tiles) return RT_ERR_INVALID_ARG;
    int r = moments_ready(c, false);
    if (r) return r;
    Device& d = c->devs[0];
    const int n = tile_count(c->width, d.local_rows);
    *n_tiles = n;
    if (!out) return RT_OK;
    if (cap < n) return set_err(c, RT_ERR_LIMIT, "rt_read_tile_sums: out is too small");
    r = moments_ready(c, true);
    if (!r) r = rt_sync(c);
    if (r || n == 0) return r;
    HIPCHK(c, hipSetDevice(d.id));
    r = ensure(c, d, d.tile_sums, (size_t)n * sizeof(rt_tile_sum));
    if (r) return r;
    if (rt_launch_tile_sums(d.image_ptr, d.m2.ptr, c->width, d.local_rows, d.tile_sums.ptr, d.stream))
        return set_err(c, RT_ERR_DEVICE, std::string("tile sums launch failed: ") + hipGetErrorString(hipGetLastError()));
    return d2h(c, d, out, d.tile_sums.ptr, (size_t)n * sizeof(rt_tile_sum));
}

int rt_noise(rt_ctx* c, rt_noise_stats* out) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    int r = moments_ready(c, true);
    if (r) return r;
    if (c->moments_frames < 2) return set_err(c, RT_ERR_STATE, "rt_noise needs at least two frames");
    int n = 0;
    r = rt_read_tile_sums(c, nullptr, 0, &n);
    if (r) return r;
    std::vector<rt_tile_sum> tiles((size_t)n);
    r = rt_read_tile_sums(c, tiles.data(), n, &n);
    if (r) return r;
    if (!c->tile_frames.empty())   // the tiles hold different counts (a tile mask): each with its own
        return rt_noise_from_tile_sums_frames(tiles.data(), c->tile_frames.data(), n, out);
    return rt_noise_from_tile_sums(tiles.data(), n, c->moments_frames, out);
}

// ---- tile masks, per-tile frame counts and the adaptive loop (rt.h) ----

namespace {
int tiles_ready(rt_ctx* c, const char* what) {
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, std::string(what) + " needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, std::string(what) + ": not under rt_set_partition");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "no image");
    return RT_OK;
}
int tile_count(const rt_ctx* c) { return rt_impl::tile_count(c->width, c->devs[0].local_rows); }
}  // namespace

int rt_set_active_tiles(rt_ctx* c, const uint8_t* active, int n_tiles) {
    if (!c) return RT_ERR_INVALID_ARG;
    int r = tiles_ready(c, "rt_set_active_tiles");
    if (r) return r;
    if (!active) {
        c->mask_set = false;
        c->act_list.clear();
        return RT_OK;
    }
    const int nt = tile_count(c);
    if (n_tiles != nt) return set_err(c, RT_ERR_INVALID_ARG, "rt_set_active_tiles: n_tiles does not match the image");
    std::vector<int32_t> list;
    for (int t = 0; t < nt; t++)
        if (active[t]) list.push_back(t);
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    if (!list.empty()) {
        // ordered on the render stream and complete on return: a queued launch keeps the list it was given
        HIPCHK(c, hipStreamSynchronize(d.stream));
        if ((r = ensure(c, d, d.tile_list, (size_t)nt * sizeof(int32_t)))) return r;
        if ((r = h2d(c, d, d.tile_list.ptr, list.data(), list.size() * sizeof(int32_t)))) return r;
    }
    c->act_list.swap(list);
    c->mask_set = true;
    return RT_OK;
}

int rt_read_tile_frames(rt_ctx* c, int32_t* frames, int cap, int* n_tiles) {
    if (!c || !n_tiles) return RT_ERR_INVALID_ARG;
    int r = tiles_ready(c, "rt_read_tile_frames");
    if (r) return r;
    const int nt = tile_count(c);
    *n_tiles = nt;
    if (!frames) return RT_OK;
    if (cap < nt) return set_err(c, RT_ERR_LIMIT, "rt_read_tile_frames: frames is too small");
    for (int t = 0; t < nt; t++) frames[t] = c->tile_frames.empty() ? c->moments_frames : c->tile_frames[(size_t)t];
    return RT_OK;
}

int rt_write_tile_frames(rt_ctx* c, const int32_t* frames, int n_tiles) {
    if (!c || !frames) return RT_ERR_INVALID_ARG;
    int r = tiles_ready(c, "rt_write_tile_frames");
    if (r) return r;
    const int nt = tile_count(c);
    if (n_tiles != nt) return set_err(c, RT_ERR_INVALID_ARG, "rt_write_tile_frames: n_tiles does not match the image");
    for (int t = 0; t < nt; t++)
        if (frames[t] < 0) return set_err(c, RT_ERR_INVALID_ARG, "rt_write_tile_frames: a count is negative");
    if (nt == 0) return RT_OK;
    const int lo = *std::min_element(frames, frames + nt), hi = *std::max_element(frames, frames + nt);
    set_all_frames(c, lo);
    if (lo != hi) c->tile_frames.assign(frames, frames + nt);
    return RT_OK;
}

int rt_render_adaptive(rt_ctx* c, int first_frame, int max_frames, int batch_frames, int min_frames, uint64_t seed,
                       float target_noise, int* frames_done, rt_noise_stats* last) {
    if (!c || !frames_done || !last) return RT_ERR_INVALID_ARG;
    *frames_done = 0;
    std::memset(last, 0, sizeof(*last));
    if (first_frame < 1 || max_frames < 1 || batch_frames < 1 || min_frames < 2 || first_frame > INT_MAX - max_frames)
        return set_err(c, RT_ERR_INVALID_ARG, "first_frame >= 1, max_frames >= 1, batch_frames >= 1, min_frames >= 2");
    int r = tiles_ready(c, "rt_render_adaptive");
    if (r) return r;
    if (!c->moments) return set_err(c, RT_ERR_STATE, "rt_set_moments(ctx, 1) first");
    if (c->mask_set) return set_err(c, RT_ERR_STATE, "rt_render_adaptive: a tile mask is set (rt_set_active_tiles(ctx, NULL, 0))");
    const int nt = tile_count(c);
    // the tiles still sampled: all of them from frame 1; on a resume the ones at the largest count
    std::vector<uint8_t> active((size_t)nt, 1), next((size_t)nt, 0);
    int n_active = nt;
    if (first_frame != 1) {
        int hi = c->moments_frames;
        for (int32_t v : c->tile_frames) hi = std::max(hi, (int)v);
        if (c->moments_frames < 1 || first_frame != hi + 1)
            return set_err(c, RT_ERR_STATE, "rt_render_adaptive: first_frame is 1, or the largest tile count + 1 of valid counts");
        if (!c->tile_frames.empty()) {
            n_active = 0;
            for (int t = 0; t < nt; t++) n_active += active[(size_t)t] = c->tile_frames[(size_t)t] == hi;
        }
    }
    std::vector<float> rf((size_t)std::min(batch_frames, max_frames));
    std::vector<rt_tile_sum> tiles((size_t)nt);
    int done = 0, converged = 0;
    while (done < max_frames) {
        const int n = std::min(batch_frames, max_frames - done);
        for (int i = 0; i < n; i++) rf[i] = rt_frame_rand_factor(seed, (uint64_t)(first_frame + done + i - 1));
        // (every tile active: the plain launch, the same bits)
        r = n_active == nt ? rt_set_active_tiles(c, nullptr, 0) : rt_set_active_tiles(c, active.data(), nt);
        if (!r) r = rt_render(c, first_frame + done, n, rf.data());
        if (!r) r = rt_sync(c);   // not pipelined: the selection depends on the inputs alone
        if (r) break;
        done += n;
        *frames_done = done;
        const int F = first_frame + done - 1;   // the frames every active tile holds
        if (F < 2) continue;   // one frame: no variance yet
        int m = 0;
        r = rt_read_tile_sums(c, tiles.data(), nt, &m);
        if (!r) r = rt_adaptive_select(tiles.data(), active.data(), nt, F, min_frames, target_noise, next.data(), &n_active);
        if (r) break;
        active.swap(next);
        if (n_active == 0) {
            converged = 1;
            break;
        }
    }
    const int r2 = rt_set_active_tiles(c, nullptr, 0);   // no mask is left set
    if (r) return r;
    if (r2) return r2;
    if (c->moments_frames < 2) {
        last->frames = c->moments_frames;
        last->noise = (double)INFINITY;
    } else if ((r = rt_noise(c, last))) {
        return r;
    }
    last->converged = converged;
    return RT_OK;
}

int rt_render_until(rt_ctx* c, int first_frame, int max_frames, int batch_frames, uint64_t seed, float target_noise,
                    int* frames_done, rt_noise_stats* last) {
    if (!c || !frames_done || !last) return RT_ERR_INVALID_ARG;
    *frames_done = 0;
    std::memset(last, 0, sizeof(*last));
    if (first_frame < 1 || max_frames < 1 || batch_frames < 1 || first_frame > INT_MAX - max_frames)
        return set_err(c, RT_ERR_INVALID_ARG, "first_frame >= 1, max_frames >= 1, batch_frames >= 1");
    if (!c->moments) return set_err(c, RT_ERR_STATE, "rt_set_moments(ctx, 1) first");
    std::vector<float> rf((size_t)std::min(batch_frames, max_frames));
    int done = 0;
    while (done < max_frames) {
        const int n = std::min(batch_frames, max_frames - done);
        for (int i = 0; i < n; i++) rf[i] = rt_frame_rand_factor(seed, (uint64_t)(first_frame + done + i - 1));
        int r = rt_render(c, first_frame + done, n, rf.data());
        if (r) return r;
        done += n;
        *frames_done = done;
        if (first_frame + done - 1 < 2) {   // one frame: no variance yet
            r = rt_sync(c);
            if (r) return r;
            last->frames = 1;
            last->noise = (double)INFINITY;
            continue;
        }
        r = rt_noise(c, last);   // waits for the batch: not pipelined, so the stop depends on the inputs alone
        if (r) return r;
        if (last->noise <= (double)target_noise) {
            last->converged = 1;
            break;
        }
    }
    return RT_OK;
}

int rt_set_bvh_mode(rt_ctx* c, int mode) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (mode != RT_BVH_REFERENCE && mode != RT_BVH_SAH) return set_err(c, RT_ERR_INVALID_ARG, "bad BVH mode");
    if (mode != c->bvh_mode) {
        c->bvh_mode = mode;
        c->ft_valid = c->ft_links_ok = false;   // the first-hit pass walked the other tree
        c->validated = false;   // validate() rebuilds the links (and a new fast_gen re-uploads them)
    }
    return RT_OK;
}

}  // extern "C"
