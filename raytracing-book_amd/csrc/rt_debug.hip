// rt_debug.hip — rt_debug.h's hooks that work on a context or a device: the stats, census and
// node-hit counters, the options, the last launch, the walk's BVH, the staged samples and the
// built-in evaluation.  The options and the stats gate depend on RT_AB_KNOBS: built per library.
// (The hooks that need neither are in rt_debug_host.cpp.)
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "rt/rt_glsl.h"
#include "rt_ctx.h"

using namespace rt_impl;

namespace {

// A device buffer of one evaluation call, freed when the call returns.  Each step says whether it
// succeeded; the callers chain them and report one RT_ERR_DEVICE.
struct Scratch {
    void* p = nullptr;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes) == hipSuccess; }
    bool alloc_zero(size_t bytes) { return alloc(bytes) && hipMemset(p, 0, bytes) == hipSuccess; }
    bool upload(const void* src, size_t bytes) { return upload_rows(src, bytes, 1, 1); }
    // rows 0..n-1 of `row` bytes, padded to npad rows (whole waves) with copies of the last row
    bool upload_rows(const void* src, size_t row, int n, int npad) {
        if (!alloc(row * (size_t)npad) || hipMemcpy(p, src, row * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
            return false;
        for (int i = n; i < npad; i++)
            if (hipMemcpy((char*)p + row * (size_t)i, (const char*)src + row * (size_t)(n - 1), row,
                          hipMemcpyHostToDevice) != hipSuccess)
                return false;
        return true;
    }
    bool download(void* dst, size_t bytes) const { return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

}  // namespace

extern "C" {

// ---- debug / test hooks (rt_debug.h)
int rt_debug_eval_builtin(int device, int fn, const float* x, const float* y, float* out, int n) {
    if (!x || !out || n < 0) return RT_ERR_INVALID_ARG;
    if (n == 0) return RT_OK;
    if (hipSetDevice(device) != hipSuccess) return RT_ERR_DEVICE;
    const size_t b = (size_t)n * 4;
    Scratch dx, dy, dout;
    const bool ok = dx.upload(x, b) && (!y || dy.upload(y, b)) && dout.alloc(b) &&
                    !rt_launch_eval_builtin(fn, (const float*)dx.p, (const float*)dy.p, (float*)dout.p, n, nullptr) &&
                    dout.download(out, b);
    return ok ? RT_OK : RT_ERR_DEVICE;
}

// The host half prepares the device records with the uploads' own functions (rt_prep.h, rt_args.h) and
// reports their flags; the device half is rt_ops_eval.hip.
int rt_debug_eval_op(int device, int op, int form, const void* recs, size_t rec_bytes, const float* rows, int n,
                     int tex_format, int tex_w, int tex_h, const void* tex, unsigned int* out, int flags[4]) {
    if (op < 0 || op >= RT_OP_N || form < 0 || !rows || n < 0 || (device >= 0 && !out)) return RT_ERR_INVALID_ARG;
    static const size_t kRec[RT_OP_N] = {sizeof(rt_sphere), sizeof(rt_sphere), sizeof(rt_quad), 6 * sizeof(rt_quad),
                                         6 * sizeof(float), 0, 0, 0};
    static const int kForms[RT_OP_N] = {4, 2, 2, 5, 3, 2, 1, 1};
    if (form >= kForms[op] || rec_bytes != kRec[op] * (size_t)n || (rec_bytes && !recs)) return RT_ERR_INVALID_ARG;
    int fl[4] = {1, 0, 0, 0};
    const int npad = (n + 63) / 64 * 64;
    // the device records, padded to whole waves with copies of the last row's
    std::vector<float4> drec;
    const void* rec_src = nullptr;
    size_t rec_row = 0;   // bytes per row of what is copied to the device
    TexturePrep tp;
    if (op == RT_OP_SPHERE || op == RT_OP_MEDIUM_SPHERE) {
        fl[0] = spheres_fd((const rt_sphere*)recs, (size_t)n);
        rec_src = recs;
        rec_row = sizeof(rt_sphere);
    } else if (op == RT_OP_QUAD) {
        fl[0] = prep_quads((const rt_quad*)recs, (size_t)n, drec);
        rec_src = drec.data();
        rec_row = RT_DFACE_F4 * sizeof(float4);
    } else if (op == RT_OP_BOX) {
        const BoxPrep B = prep_boxes((const rt_quad*)recs, (size_t)n);
        fl[0] = B.fd;
        fl[1] = B.n_compact;
        if (form >= 2 && B.n_compact != n) return RT_ERR_INVALID_ARG;
        drec.resize((size_t)n * (RT_DBOX_F4 + RT_BOXC_F4));
        for (int i = 0; i < n; i++) {
            float4* o = &drec[(size_t)i * (RT_DBOX_F4 + RT_BOXC_F4)];
            std::copy(&B.faces[(size_t)i * RT_DBOX_F4], &B.faces[(size_t)i * RT_DBOX_F4] + RT_DBOX_F4, o);
            std::copy(&B.boxc[(size_t)i * RT_BOXC_F4], &B.boxc[(size_t)i * RT_BOXC_F4] + RT_BOXC_F4, o + RT_DBOX_F4);
        }
        rec_src = drec.data();
        rec_row = (RT_DBOX_F4 + RT_BOXC_F4) * sizeof(float4);
    } else if (op == RT_OP_NODE) {
        rec_src = recs;
        rec_row = 6 * sizeof(float);
    }
    if (op == RT_OP_PERLIN || op == RT_OP_TEXTURE) {
        std::string err;
        if (op == RT_OP_PERLIN && (tex_format != RT_TEX_R32F || tex_w != 6 || tex_h != 256)) return RT_ERR_INVALID_ARG;
        const int r = prep_texture(0, tex_format, tex_w, tex_h, tex, tp, &err);
        if (r) return r;
        fl[1] = op == RT_OP_PERLIN && !tp.pk.empty();
        if (op == RT_OP_PERLIN && form == 1 && tp.pk.empty()) return RT_ERR_INVALID_ARG;
    }
    for (int w = 0; w < npad / 64; w++) {
        int bad = 0;
        for (int i = w * 64; i < w * 64 + 64; i++) {
            const float* r = rows + (size_t)std::min(i, n - 1) * RT_OPS_ROW_F;
            const float a = g_dot(mk3(r[3], r[4], r[5]), mk3(r[3], r[4], r[5]));
            if (!(a >= 0x1p-60f)) bad += i < n;
        }
        fl[2] += bad > 0;
        fl[3] += bad;
    }
    if (flags) std::memcpy(flags, fl, sizeof(fl));
    if (device < 0 || n == 0) return RT_OK;

    if (hipSetDevice(device) != hipSuccess) return RT_ERR_DEVICE;
    Scratch d_rec, d_rows, d_out, d_tex, d_args;
    bool ok = d_rows.upload_rows(rows, RT_OPS_ROW_F * sizeof(float), n, npad) &&
              (!rec_row || d_rec.upload_rows(rec_src, rec_row, n, npad)) &&
              d_out.alloc_zero((size_t)npad * RT_OPS_OUT_W * 4);
    // the argument block the texture functions read: slot 0's texture in global memory, no LDS tables
    rt_kernel_args a;
    std::memset(&a, 0, sizeof(a));
    a.perlin_slot = -1;
    clear_lds_tables(a, LDS_LEAF);   // (tex_lds_off[] stays 0: read only where tex_lds >= 0)
    if (op == RT_OP_PERLIN || op == RT_OP_TEXTURE) {
        const bool pk = op == RT_OP_PERLIN && form == 1;
        ok = ok && (pk ? d_tex.upload(tp.pk.data(), tp.pk.size() * sizeof(float4)) : d_tex.upload(tp.src, tp.bytes));
        a.tex[0].data = d_tex.p;
        a.tex[0].w = tex_w;
        a.tex[0].h = tex_h;
        a.tex[0].is_float = tex_format == RT_TEX_R32F;
    }
    ok = ok && d_args.upload(&a, sizeof(a)) &&
         !rt_launch_eval_op((const rt_kernel_args*)d_args.p, op, form, op == RT_OP_PERLIN ? d_tex.p : d_rec.p,
                            (const float*)d_rows.p, d_out.p, npad, nullptr) &&
         d_out.download(out, (size_t)n * RT_OPS_OUT_W * 4);
    return ok ? RT_OK : RT_ERR_DEVICE;
}

// The host half checks the rows (the rejection loops never end on NaN draws; a shade row must name
// records the scene holds), assembles the scene's argument block as rt_render does (scene_args) with
// every LDS offset at -1, and binds the first device's copies; the device half is rt_shade_eval.hip.
int rt_debug_eval_shade_op(rt_ctx* c, int device, int op, int form, const float* rows, int n, unsigned int* out) {
    if (op < 0 || op >= RT_SOP_N || form < 0 || form > (op == RT_SOP_SHADE || op == RT_SOP_TRACE ? 1 : 0) || !rows || n < 0)
        return RT_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        const float* r = rows + (size_t)i * RT_SOP_ROW_F;
        if (!(r[9] >= 0.0f && r[9] < 16384.0f) || !(r[10] >= 0.0f && r[10] < 16384.0f) ||
            !(r[11] >= 0.0f && r[11] < 4096.0f))
            return RT_ERR_INVALID_ARG;
    }
    if (device < 0) return RT_OK;
    if (!c || !out) return RT_ERR_INVALID_ARG;
    if (c->devs.empty()) return set_err(c, RT_ERR_STATE, "rt_debug_eval_shade_op: the context has no device");
    if (!c->have_cam) return set_err(c, RT_ERR_STATE, "rt_set_camera before rt_debug_eval_shade_op");
    if (!c->uploaded[RT_BIND_BVH]) return set_err(c, RT_ERR_STATE, "no BVH uploaded");
    int r = validate(c);
    if (r) return r;
    if (op == RT_SOP_SHADE) {
        const size_t count[4] = {c->n_records(RT_BIND_SPHERES), c->n_records(RT_BIND_QUADS),
                                 c->n_records(RT_BIND_MEDIA), c->n_records(RT_BIND_BOXES)};
        for (int i = 0; i < n; i++) {
            int32_t tif, uvk;
            std::memcpy(&tif, rows + (size_t)i * RT_SOP_ROW_F + 7, 4);
            std::memcpy(&uvk, rows + (size_t)i * RT_SOP_ROW_F + 15, 4);
            const int type = tif & 0xF, face = (tif >> 4) & 0x7;
            const size_t idx = (uint32_t)tif >> 16;
            const int which = type == RT_MODEL_SPHERE ? 0 : type == RT_MODEL_QUAD ? 1
                            : type == RT_MODEL_CONSTANT_MEDIUM ? 2 : type == RT_MODEL_BOX ? 3 : -1;
            if (which < 0 || idx >= count[which] || face > (type == RT_MODEL_BOX ? 5 : 0))
                return set_err(c, RT_ERR_INVALID_ARG, "rt_debug_eval_shade_op: a row's tif names no record of the scene");
            if ((uvk >> 16) == 1 && (size_t)(uvk & 0xFFFF) >= count[0])
                return set_err(c, RT_ERR_INVALID_ARG, "rt_debug_eval_shade_op: a row's UvSrc names no sphere of the scene");
        }
    }
    if (n == 0) return RT_OK;
    rt_kernel_args a;
    if ((r = scene_args(*c, a, &c->err))) return r;
    clear_lds_tables(a, LDS_ALL);
    if (op == RT_SOP_TRACE) {
        // the plain walk's links (validate() built them) and its leaf tests: form 0 the generic ones under
        // the context's box pre-test margin, form 1 the shared-reciprocal ones, only where the launch plan
        // itself would take them
        if (c->n_link_nodes > 0 && c->links.empty())
            return set_err(c, RT_ERR_LIMIT, "rt_debug_eval_shade_op: the BVH has no link form (more than 65535 nodes)");
        if (form == 1 && !a.fastdiv)
            return set_err(c, RT_ERR_INVALID_ARG, "rt_debug_eval_shade_op: the scene is not in the shared-reciprocal regime");
    }
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    bind_scene(d, a);
    const int npad = (n + 63) / 64 * 64;
    Scratch d_rows, d_out, d_args;
    if (op == RT_SOP_TRACE) {
        Scratch d_links;
        const bool ok = d_rows.upload_rows(rows, RT_SOP_ROW_F * sizeof(float), n, npad) &&
                        d_out.alloc_zero((size_t)npad * RT_SOP_OUT_W * 4) && d_args.upload(&a, sizeof(a)) &&
                        (c->links.empty() || d_links.upload(c->links.data(), c->links.size() * sizeof(float4))) &&
                        !rt_launch_eval_trace_op((const rt_kernel_args*)d_args.p, form, d_links.p, c->n_link_nodes,
                                                 (const float*)d_rows.p, d_out.p, npad, nullptr) &&
                        d_out.download(out, (size_t)n * RT_SOP_OUT_W * 4);
        return ok ? RT_OK : set_err(c, RT_ERR_DEVICE, "rt_debug_eval_shade_op: a HIP call failed");
    }
    const bool ok = d_rows.upload_rows(rows, RT_SOP_ROW_F * sizeof(float), n, npad) &&
                    d_out.alloc_zero((size_t)npad * RT_SOP_OUT_W * 4) && d_args.upload(&a, sizeof(a)) &&
                    !rt_launch_eval_shade_op((const rt_kernel_args*)d_args.p, op, form, (const float*)d_rows.p, d_out.p,
                                             npad, nullptr) &&
                    d_out.download(out, (size_t)n * RT_SOP_OUT_W * 4);
    return ok ? RT_OK : set_err(c, RT_ERR_DEVICE, "rt_debug_eval_shade_op: a HIP call failed");
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
