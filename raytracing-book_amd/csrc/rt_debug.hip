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

#ifdef RT_AB_KNOBS
static const bool kAbOptions = true;
#else
static const bool kAbOptions = false;
#endif

int rt_debug_set_option(rt_ctx* c, int option, int v) {
    if (!c) return RT_ERR_INVALID_ARG;
    return set_option(*c, option, v, kAbOptions, &c->err);
}

int rt_debug_get_option(rt_ctx* c, int option, int* v) {
    if (!c || !v) return RT_ERR_INVALID_ARG;
    return get_option(*c, option, v, kAbOptions, &c->err);
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
