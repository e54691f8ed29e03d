// rt_debug.hip — rt_debug.h's hooks that work on a context or a device: the stats, census and
// node-hit counters, the options, the last launch, the walk's BVH, the staged samples and the
// built-in evaluation.  The options and the stats gate depend on RT_AB_KNOBS: built per library.
// (The hooks that need neither are in rt_debug_host.cpp.)
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "rt_ctx.h"

using namespace rt_impl;

extern "C" {

// ---- debug / test hooks (rt_debug.h)
int rt_debug_eval_builtin(int device, int fn, const float* x, const float* y, float* out, int n) {
    if (!x || !out || n < 0) return RT_ERR_INVALID_ARG;
    if (n == 0) return RT_OK;
    if (hipSetDevice(device) != hipSuccess) return RT_ERR_DEVICE;
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    size_t b = (size_t)n * 4;
    int rc = RT_OK;
    if (hipMalloc(&dx, b) != hipSuccess || hipMalloc(&dout, b) != hipSuccess || (y && hipMalloc(&dy, b) != hipSuccess))
        rc = RT_ERR_DEVICE;
    if (!rc && hipMemcpy(dx, x, b, hipMemcpyHostToDevice) != hipSuccess) rc = RT_ERR_DEVICE;
    if (!rc && y && hipMemcpy(dy, y, b, hipMemcpyHostToDevice) != hipSuccess) rc = RT_ERR_DEVICE;
    if (!rc && rt_launch_eval_builtin(fn, dx, dy, dout, n, nullptr)) rc = RT_ERR_DEVICE;
    if (!rc && hipMemcpy(out, dout, b, hipMemcpyDeviceToHost) != hipSuccess) rc = RT_ERR_DEVICE;
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    if (dout) (void)hipFree(dout);
    return rc;
}

int rt_debug_read_samples(rt_ctx* c, float* out, size_t cap_floats, int* n_frames) {
    if (!c || !n_frames) return RT_ERR_INVALID_ARG;
    if (!c->launched || c->staged_frames <= 0) return set_err(c, RT_ERR_STATE, "the last launch was not staged");
    Device& d = c->devs[0];
    const size_t n_pixels = (size_t)d.local_rows * c->width;
    const int nf = c->staged_frames;
    *n_frames = nf;
    if (!out) return RT_OK;
    if (cap_floats < (size_t)nf * n_pixels * 4) return set_err(c, RT_ERR_LIMIT, "rt_debug_read_samples: out is too small");
    int r = rt_sync(c);
    if (r) return r;
    HIPCHK(c, hipSetDevice(d.id));
    if (d.samples.bytes < (size_t)nf * n_pixels * 16 || (c->staged_sparse && d.sflags.bytes < (size_t)nf * n_pixels))
        return set_err(c, RT_ERR_STATE, "the staged colours are gone");
    r = d2h(c, d, out, d.samples.ptr, (size_t)nf * n_pixels * 16);
    if (r || !c->staged_sparse) return r;
    std::vector<uint8_t> fl((size_t)nf * n_pixels);   // a clear flag is the zero colour, never stored
    r = d2h(c, d, fl.data(), d.sflags.ptr, fl.size());
    if (r) return r;
    for (size_t i = 0; i < fl.size(); i++)
        if (!fl[i]) std::memset(out + i * 4, 0, 16);
    return RT_OK;
}

// The stats twin (region timers + lane counters) of a launch variant: 61 -> 69, 30 -> 31, 37 -> 38, 0 -> 39.
static int stats_twin(int v) {
    if (v == 61 || v == 69) return 69;
    if (v == 30 || v == 31) return 31;
    if (v == 37 || v == 38) return 38;
    return 39;
}

// Leaf census records per resident wave (rt_debug_enable_stats(ctx, 2); tools/leaf_census.py)
#define RT_CENSUS_CAP 2048

int rt_debug_enable_stats(rt_ctx* c, int on) {
    if (!c || on < 0 || on > 2) return RT_ERR_INVALID_ARG;
#ifndef RT_AB_KNOBS
    if (on) return set_err(c, RT_ERR_STATE, "the stats kernels are in the A/B build (librtamd_ab.so)");
#endif
    for (Device& d : c->devs) {
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        if (on && !d.stats.ptr) {
            HIPCHK(c, hipMalloc(&d.stats.ptr, RT_STATS_N * sizeof(unsigned long long)));
            d.stats.bytes = RT_STATS_N * sizeof(unsigned long long);
        }
        if (d.stats.ptr) HIPCHK(c, hipMemsetAsync(d.stats.ptr, 0, d.stats.bytes, d.stream));
        if (on == 2 && !d.census.ptr) {
            const int waves = rt_resident_waves();
            const size_t bytes = ((size_t)waves + (size_t)waves * RT_CENSUS_CAP * RT_CENSUS_WORDS) * sizeof(unsigned);
            HIPCHK(c, hipMalloc(&d.census.ptr, bytes));
            d.census.bytes = bytes;
            d.census_cap = RT_CENSUS_CAP;
            d.census_waves = waves;
        }
        if (on != 2 && d.census.ptr) {
            dev_free(d.census);
            d.census_cap = d.census_waves = 0;
        }
        if (d.census.ptr) HIPCHK(c, hipMemsetAsync(d.census.ptr, 0, d.census.bytes, d.stream));
        HIPCHK(c, hipStreamSynchronize(d.stream));
    }
    if (on) {
        if (c->variant_no_stats < 0) c->variant_no_stats = c->variant;
        c->variant = stats_twin(c->variant_no_stats);
    } else if (c->variant_no_stats >= 0) {
        c->variant = c->variant_no_stats;
        c->variant_no_stats = -1;
    }
    return RT_OK;
}

int rt_debug_read_census(rt_ctx* c, unsigned* out, size_t words, size_t* needed, int* waves, int* cap) {
    if (!c || c->devs.empty()) return RT_ERR_INVALID_ARG;
    Device& d = c->devs[0];
    const size_t n = d.census.bytes / sizeof(unsigned);
    if (needed) *needed = n;
    if (waves) *waves = d.census_waves;
    if (cap) *cap = d.census_cap;
    if (!out) return RT_OK;
    if (words < n) return set_err(c, RT_ERR_LIMIT, "census buffer too small");
    if (!n) return RT_OK;
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, out, d.census.ptr, d.census.bytes);
}

// The stats twin's node-hit count (tools/collapse_hits_ab.py): on = 1 allocates and zeroes one word
// per possible link node plus the walk count; the stats twin's launches then add to it.
int rt_debug_count_node_hits(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID_ARG;
    for (Device& d : c->devs) {
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        if (!on) {
            dev_free(d.node_hits);
            continue;
        }
        const size_t bytes = ((size_t)2 * RT_LINK_MAX_NODES + 1) * sizeof(unsigned);
        if (!d.node_hits.ptr) {
            HIPCHK(c, hipMalloc(&d.node_hits.ptr, bytes));
            d.node_hits.bytes = bytes;
        }
        HIPCHK(c, hipMemset(d.node_hits.ptr, 0, d.node_hits.bytes));
    }
    return RT_OK;
}

// Per link node (the last launch's layout, n_walk_nodes of them) its hits, summed over the devices,
// then the walks begun at the root: n_out = n_walk_nodes + 1 words.
int rt_debug_read_node_hits(rt_ctx* c, unsigned* out, size_t words, size_t* n_out) {
    if (!c || c->devs.empty()) return RT_ERR_INVALID_ARG;
    const size_t n = (size_t)c->n_walk_nodes + 1;
    if (n_out) *n_out = n;
    if (!out) return RT_OK;
    if (words < n) return set_err(c, RT_ERR_LIMIT, "node-hit buffer too small");
    std::memset(out, 0, n * sizeof(unsigned));
    std::vector<unsigned> tmp(n);
    for (Device& d : c->devs) {
        if (!d.node_hits.ptr) return set_err(c, RT_ERR_STATE, "rt_debug_count_node_hits(ctx, 1) first");
        HIPCHK(c, hipSetDevice(d.id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        HIPCHK(c, hipMemcpy(tmp.data(), d.node_hits.ptr, (n - 1) * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&tmp[n - 1], (unsigned*)d.node_hits.ptr + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) out[i] += tmp[i];
    }
    return RT_OK;
}

// The collapse planned from measured hits (rt_debug_read_node_hits of an uncollapsed walk over the same
// tree, spine off) instead of the camera grid; n = 0 goes back to the grid.  Exact either way.
int rt_debug_set_collapse_hits(rt_ctx* c, const unsigned* hits, size_t n, unsigned long long walks) {
    if (!c || (n && !hits)) return RT_ERR_INVALID_ARG;
    c->inj_hits.assign(hits, hits + n);
    c->inj_walks = (int64_t)walks;
    c->walk_stale = true;
    return RT_OK;
}

int rt_debug_read_stats(rt_ctx* c, unsigned long long* out, int n) {
    if (!c || !out || n <= 0 || n > RT_STATS_N) return RT_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(unsigned long long) * n);
    for (Device& d : c->devs) {
        if (!d.stats.ptr) continue;
        HIPCHK(c, hipSetDevice(d.id));
        std::vector<unsigned long long> tmp(n);
        int r = d2h(c, d, tmp.data(), d.stats.ptr, sizeof(unsigned long long) * n);
        if (r) return r;
        for (int i = 0; i < n; i++) out[i] += tmp[i];
    }
    return RT_OK;
}

int rt_debug_ab_build(void) {
#ifdef RT_AB_KNOBS
    return 1;
#else
    return 0;
#endif
}

int rt_debug_set_option(rt_ctx* c, int option, int v) {
    if (!c) return RT_ERR_INVALID_ARG;
    auto bad = [&]() { return set_err(c, RT_ERR_INVALID_ARG, "option value out of range"); };
    switch (option) {
        case RT_OPTION_BOX_PRETEST: c->box_pretest = v != 0; break;
        case RT_OPTION_FASTDIV: c->fastdiv = v != 0; break;
        case RT_OPTION_SPH_LDS: c->sph_lds = v != 0; break;
        case RT_OPTION_BIG_WG: c->big_wg = v != 0; break;
        case RT_OPTION_COMPACT_BOXES: c->compact_boxes = v != 0; break;
        case RT_OPTION_SPINE: c->spine = v != 0; break;
        case RT_OPTION_TL_LEAF_LDS: c->tl_leaf_lds = v != 0; break;
        case RT_OPTION_PERLIN_PACKED: c->perlin_pk = v != 0; break;
        case RT_OPTION_SPARSE_STAGE: c->sparse_stage = v != 0; break;
        case RT_OPTION_SPHERE_PAIRS: if (v < 0 || v > 2) return bad(); c->sphere_pairs = v; break;
        case RT_OPTION_LEAF_PREFETCH: c->leaf_prefetch = v != 0; break;
        case RT_OPTION_TL_SMALL_LDS: c->tl_small_lds = v != 0; break;
        case RT_OPTION_SHADE_LDS: c->shade_lds = v != 0; break;
        case RT_OPTION_BOX_VNODES: c->box_vnodes = v != 0; break;
        case RT_OPTION_BOX_INTERIOR: c->box_interior = v != 0; break;
        case RT_OPTION_ZERO_DIR_END: c->zero_dir_end = v != 0; break;
        case RT_OPTION_FIRST_LEAF: c->first_leaf = v != 0; break;
        case RT_OPTION_COLLAPSE: c->collapse = v != 0; break;
        case RT_OPTION_REBUILD: if (v < 0 || v > 2) return bad(); c->rebuild = v; break;
        case RT_OPTION_CHUNK_TARGET: if (v < 0) return bad(); c->chunk_target = v; break;
        case RT_OPTION_STAGED_CHUNK_TARGET: if (v < 1) return bad(); c->staged_chunk_target = v; break;
        case RT_OPTION_STAGE_TILES: if (v < 0) return bad(); c->stage_tiles = v; break;
        case RT_OPTION_SM_BATCH: if (v < 1 || v > 64) return bad(); c->sm_batch = v; break;
        case RT_OPTION_SM_FRAC: if (v < 0 || v > 64) return bad(); c->sm_frac = v; break;
        case RT_OPTION_WALK_FRAC: if (v < 0 || v > 64) return bad(); c->walk_frac = v; break;
        case RT_OPTION_WATCHDOG_MS: if (v < 0) return bad(); c->watchdog_ticks = (unsigned long long)v * 100000ull; break;
        case RT_OPTION_CHUNK_WAIT_MS: if (v < 0) return bad(); c->chunk_wait_ticks = (unsigned long long)v * 100000ull; break;
        case RT_OPTION_LDS_NODE_CAP: if (v < 0) return bad(); c->lds_node_cap = v; break;
        case RT_OPTION_TAIL_CHUNKS: if (v < -1 || v > RT_MAX_FRAMES_PER_LAUNCH) return bad(); c->tail_chunks = v; break;
#ifdef RT_AB_KNOBS
        case RT_OPTION_KERNEL_VARIANT:
            if (!(v == 0 || v == 30 || v == 31 || v == 37 || v == 38 || v == 39 || v == 61 || v == 69)) return bad();
            c->variant = v;
            break;
        case RT_OPTION_DEBUG_FLAGS: c->debug_flags = v; break;
#endif
        default: return set_err(c, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
    }
    return RT_OK;
}

int rt_debug_get_option(rt_ctx* c, int option, int* v) {
    if (!c || !v) return RT_ERR_INVALID_ARG;
    switch (option) {
        case RT_OPTION_BOX_PRETEST: *v = c->box_pretest; break;
        case RT_OPTION_FASTDIV: *v = c->fastdiv; break;
        case RT_OPTION_SPH_LDS: *v = c->sph_lds; break;
        case RT_OPTION_BIG_WG: *v = c->big_wg; break;
        case RT_OPTION_COMPACT_BOXES: *v = c->compact_boxes; break;
        case RT_OPTION_SPINE: *v = c->spine; break;
        case RT_OPTION_TL_LEAF_LDS: *v = c->tl_leaf_lds; break;
        case RT_OPTION_PERLIN_PACKED: *v = c->perlin_pk; break;
        case RT_OPTION_SPARSE_STAGE: *v = c->sparse_stage; break;
        case RT_OPTION_SPHERE_PAIRS: *v = c->sphere_pairs; break;
        case RT_OPTION_LEAF_PREFETCH: *v = c->leaf_prefetch; break;
        case RT_OPTION_TL_SMALL_LDS: *v = c->tl_small_lds; break;
        case RT_OPTION_SHADE_LDS: *v = c->shade_lds; break;
        case RT_OPTION_BOX_VNODES: *v = c->box_vnodes; break;
        case RT_OPTION_BOX_INTERIOR: *v = c->box_interior; break;
        case RT_OPTION_ZERO_DIR_END: *v = c->zero_dir_end; break;
        case RT_OPTION_FIRST_LEAF: *v = c->first_leaf; break;
        case RT_OPTION_COLLAPSE: *v = c->collapse; break;
        case RT_OPTION_REBUILD: *v = c->rebuild; break;
        case RT_OPTION_CHUNK_TARGET: *v = c->chunk_target; break;
        case RT_OPTION_STAGED_CHUNK_TARGET: *v = c->staged_chunk_target; break;
        case RT_OPTION_STAGE_TILES: *v = c->stage_tiles; break;
        case RT_OPTION_SM_BATCH: *v = c->sm_batch; break;
        case RT_OPTION_SM_FRAC: *v = c->sm_frac; break;
        case RT_OPTION_WALK_FRAC: *v = c->walk_frac; break;
        case RT_OPTION_WATCHDOG_MS: *v = (int)std::min<unsigned long long>(INT_MAX, c->watchdog_ticks / 100000ull); break;
        case RT_OPTION_CHUNK_WAIT_MS: *v = (int)std::min<unsigned long long>(INT_MAX, c->chunk_wait_ticks / 100000ull); break;
        case RT_OPTION_LDS_NODE_CAP: *v = c->lds_node_cap; break;
        case RT_OPTION_TAIL_CHUNKS: *v = c->tail_chunks; break;
#ifdef RT_AB_KNOBS
        case RT_OPTION_KERNEL_VARIANT: *v = c->variant; break;
        case RT_OPTION_DEBUG_FLAGS: *v = c->debug_flags; break;
#endif
        default: return set_err(c, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
    }
    return RT_OK;
}

int rt_debug_walk_bvh(rt_ctx* c, void* out, size_t out_cap, size_t* nbytes) {
    if (!c || !nbytes) return RT_ERR_INVALID_ARG;
    if (!c->uploaded[RT_BIND_BVH]) return set_err(c, RT_ERR_STATE, "no BVH uploaded");
    int r = validate(c);
    if (r) return r;
    const std::vector<uint8_t>& B = c->bvh_mode == RT_BVH_SAH ? c->sah_bvh : c->host_buf[RT_BIND_BVH];
    *nbytes = B.size();
    if (!out) return RT_OK;
    if (out_cap < B.size()) return set_err(c, RT_ERR_LIMIT, "buffer too small");
    if (!B.empty()) std::memcpy(out, B.data(), B.size());
    return RT_OK;
}

int rt_debug_last_launch(rt_ctx* c, int* out, int n) {
    if (!c || !out || n < 0 || n > RT_LI_N) return RT_ERR_INVALID_ARG;
    if (!c->launched) return set_err(c, RT_ERR_STATE, "no render launched yet");
    std::memcpy(out, c->last_launch, sizeof(int) * (size_t)n);
    return RT_OK;
}

int rt_debug_first_leaf(rt_ctx* c, int out[4]) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    if (!c->launched) return set_err(c, RT_ERR_STATE, "no render launched yet");
    std::memcpy(out, c->first_leaf_last, sizeof(c->first_leaf_last));
    return RT_OK;
}

int rt_debug_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
