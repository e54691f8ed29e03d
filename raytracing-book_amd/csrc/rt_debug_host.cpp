// rt_debug_host.cpp — the C ABI's entries that need no context and no device: the stripe
// arithmetic and frame factors of rt.h, and rt_debug.h's views of the host-only scene
// preparation (rt_prep.h), launch planning (rt_plan.h) and argument assembly (rt_args.h).  Plain C++, built once and linked into both libraries; with
// rt_prep.cpp it links into a stand-alone program (tools/fuzz).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt/rt.h"
#include "rt/rt_debug.h"
#include "rt/rt_types.h"
#include "rt_args.h"
#include "rt_plan.h"
#include "rt_prep.h"
#include "bvh_sah.h"

using namespace rt_impl;

extern "C" {

int rt_local_rows(int height, int rank, int world, int stripe_rows) { return local_rows_of(height, rank, world, stripe_rows); }
int rt_padded_local_rows(int height, int world, int stripe_rows) {
    if (height <= 0 || world <= 0 || stripe_rows <= 0) return 0;
    return padded_rows_of(height, world, stripe_rows);
}

int rt_noise_from_tile_sums(const rt_tile_sum* tiles, int n_tiles, int frames, rt_noise_stats* out) {
    if (!out || n_tiles < 0 || (n_tiles > 0 && !tiles) || frames < 2) return RT_ERR_INVALID_ARG;
    rt_noise_stats s;
    std::memset(&s, 0, sizeof(s));
    for (int i = 0; i < n_tiles; i++) {   // in tile order, in double: the figure depends on the tiles alone
        s.sum_m2y += (double)tiles[i].m2y;
        s.sum_y += (double)tiles[i].y;
        s.pixels += tiles[i].pixels;
        s.bad += tiles[i].bad;
    }
    s.frames = frames;
    const double p = (double)(s.pixels - s.bad);
    const double num = std::sqrt(std::max(0.0, s.sum_m2y / ((double)frames * ((double)frames - 1.0))) * p);
    if (s.sum_y == 0.0) s.noise = num == 0.0 ? 0.0 : (double)INFINITY;
    else s.noise = num / s.sum_y;
    *out = s;
    return RT_OK;
}

int rt_noise_from_tile_sums_frames(const rt_tile_sum* tiles, const int32_t* frames, int n_tiles, rt_noise_stats* out) {
    if (!out || n_tiles < 0 || (n_tiles > 0 && (!tiles || !frames))) return RT_ERR_INVALID_ARG;
    for (int i = 0; i < n_tiles; i++)
        if (frames[i] < 2) return RT_ERR_INVALID_ARG;
    rt_noise_stats s;
    std::memset(&s, 0, sizeof(s));
    double var = 0.0;   // sum over tiles of m2y_t / (n_t (n_t - 1)), in tile order
    for (int i = 0; i < n_tiles; i++) {
        const double n = (double)frames[i];
        var += (double)tiles[i].m2y / (n * (n - 1.0));
        s.sum_m2y += (double)tiles[i].m2y;
        s.sum_y += (double)tiles[i].y;
        s.pixels += tiles[i].pixels;
        s.bad += tiles[i].bad;
        s.frames = std::max(s.frames, (int)frames[i]);
    }
    const double p = (double)(s.pixels - s.bad);
    const double num = std::sqrt(std::max(0.0, var) * p);
    if (s.sum_y == 0.0) s.noise = num == 0.0 ? 0.0 : (double)INFINITY;
    else s.noise = num / s.sum_y;
    *out = s;
    return RT_OK;
}

int rt_adaptive_select(const rt_tile_sum* tiles, const uint8_t* active_in, int n_tiles, int frames, int min_frames,
                       float target, uint8_t* active_out, int* n_active) {
    if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !active_out)) || frames < 1 || min_frames < 2)
        return RT_ERR_INVALID_ARG;
    double sy = 0.0, sp = 0.0;   // over all tiles, stopped ones included, in tile order
    for (int i = 0; i < n_tiles; i++) {
        sy += (double)tiles[i].y;
        sp += (double)(tiles[i].pixels - tiles[i].bad);
    }
    const double ybar = sp > 0.0 ? sy / sp : 0.0;
    const double lim = (double)target * ybar;
    const double F = (double)frames;
    int n = 0;
    for (int i = 0; i < n_tiles; i++) {
        bool keep = !active_in || active_in[i] != 0;
        if (keep && frames >= min_frames) {
            const double pt = (double)(tiles[i].pixels - tiles[i].bad);
            if (pt == 0.0) {
                keep = false;
            } else {
                const double v = (double)tiles[i].m2y / (F * (F - 1.0)) / pt;
                keep = !(v <= lim * lim);
            }
        }
        active_out[i] = keep ? 1 : 0;
        n += keep;
    }
    if (n_active) *n_active = n;
    return RT_OK;
}

int rt_deinterleave_rows(const float* gathered, int width, int height, int world, int stripe_rows, float* out) {
    if (!gathered || !out || width <= 0 || height <= 0 || world < 1 || stripe_rows < 1) return RT_ERR_INVALID_ARG;
    int padded = padded_rows_of(height, world, stripe_rows);
    int n_stripes = (height + stripe_rows - 1) / stripe_rows;
    for (int k = 0; k < world; k++) {
        size_t lr = 0;
        for (int s = k; s < n_stripes; s += world)
            for (int y = s * stripe_rows; y < std::min(height, (s + 1) * stripe_rows); y++, lr++)
                std::memcpy(out + (size_t)y * width * 4, gathered + ((size_t)k * padded + lr) * width * 4,
                            (size_t)width * 16);
    }
    return RT_OK;
}

float rt_frame_rand_factor(uint64_t seed, uint64_t frame_index) {
    uint64_t z = seed + (frame_index + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) / 16777216.0f;
}

int rt_debug_threaded_bvh(const void* nodes, size_t nbytes, void* out, size_t out_cap, int* n_out) {
    if (!nodes || !n_out || nbytes % sizeof(rt_bvh_node)) return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)nodes, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    *n_out = (int)dn.size();
    if (out) {
        if (out_cap < dn.size() * sizeof(rt_dnode)) return RT_ERR_INVALID_ARG;
        if (!dn.empty()) std::memcpy(out, dn.data(), dn.size() * sizeof(rt_dnode));
    }
    return RT_OK;
}

int rt_debug_deinterleave(const float* gathered, int width, int height, int world, int stripe_rows, float* out) {
    if (!gathered || !out || width <= 0 || height <= 0 || world < 1 || stripe_rows < 1) return RT_ERR_INVALID_ARG;
    const int padded = padded_rows_of(height, world, stripe_rows);
    for (int y = 0; y < height; y++) {   // deinterleave_kernel's indexing, one row at a time
        int k, lr;
        rt_gathered_row(y, world, stripe_rows, &k, &lr);
        std::memcpy(out + (size_t)y * width * 4, gathered + ((size_t)k * padded + lr) * width * 4, (size_t)width * 16);
    }
    return RT_OK;
}

int rt_debug_box_records(const void* boxes, size_t nbytes, void* out, size_t out_cap, int* n_compact) {
    if (!boxes || !n_compact || nbytes % sizeof(rt_box)) return RT_ERR_INVALID_ARG;
    const size_t nb = nbytes / sizeof(rt_box);
    if (out && out_cap < nb * RT_BOXC_F4 * sizeof(float4)) return RT_ERR_INVALID_ARG;
    // the upload's own path (rt_upload_buffer(RT_BIND_BOXES) calls prep_boxes too)
    const BoxPrep P = prep_boxes((const rt_quad*)boxes, nb);
    const std::vector<float4>& recs = P.boxc;
    *n_compact = P.n_compact;
    if (out && !recs.empty()) std::memcpy(out, recs.data(), recs.size() * sizeof(float4));
    return RT_OK;
}

int rt_debug_link_nodes_vbox(const void* bvh, size_t nbytes, const float* vbox, int n_box, void* out,
                             size_t out_cap, int* n_f4, int* n_nodes) {
    if (!bvh || !n_f4 || !n_nodes || nbytes % sizeof(rt_bvh_node) || n_box < 0 || (n_box && !vbox))
        return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)bvh, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    const std::vector<float> vb(vbox, vbox + 6 * (size_t)n_box);
    const std::vector<float4> L = build_links(dn, &vb, n_nodes);
    *n_f4 = (int)L.size();
    if (out) {
        if (out_cap < L.size() * sizeof(float4)) return RT_ERR_INVALID_ARG;
        if (!L.empty()) std::memcpy(out, L.data(), L.size() * sizeof(float4));
    }
    return RT_OK;
}

int rt_debug_collapse_links(const void* bvh, size_t nbytes, const float cam[28], int width, int height, int rebuild,
                            void* out, size_t out_cap, int* n_f4, uint8_t* drop, size_t drop_cap, int* n_dropped) {
    if (!bvh || !cam || !n_f4 || !n_dropped || nbytes % sizeof(rt_bvh_node)) return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)bvh, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    if (rebuild) {
        std::vector<rt_dnode> rb = rebuild_inner(dn, rebuild);
        if (!rb.empty()) dn.swap(rb);
    }
    rt_camera_ubo cu;
    std::memcpy(&cu, cam, sizeof(cu));
    const std::vector<uint8_t> d = plan_collapse(dn, cu, width, height);
    int nd = 0;
    for (uint8_t x : d) nd += x;
    *n_dropped = nd;
    int nn = 0;
    const std::vector<float4> L = build_links(dn, nullptr, &nn, &d);
    *n_f4 = (int)L.size();
    if (out) {
        if (out_cap < L.size() * sizeof(float4)) return RT_ERR_INVALID_ARG;
        if (!L.empty()) std::memcpy(out, L.data(), L.size() * sizeof(float4));
    }
    if (drop) {
        if (drop_cap < d.size()) return RT_ERR_INVALID_ARG;
        if (!d.empty()) std::memcpy(drop, d.data(), d.size());
    }
    return RT_OK;
}

int rt_debug_link_nodes(const void* bvh, size_t nbytes, void* out, size_t out_cap, int* n_f4) {
    if (!bvh || !n_f4 || nbytes % sizeof(rt_bvh_node)) return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)bvh, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    const std::vector<float4> L = build_links(dn);
    *n_f4 = (int)L.size();
    if (out) {
        if (out_cap < L.size() * sizeof(float4)) return RT_ERR_INVALID_ARG;
        if (!L.empty()) std::memcpy(out, L.data(), L.size() * sizeof(float4));
    }
    return RT_OK;
}

int rt_debug_plan_kernel(const int* in, int n_in, int ab, int* out, int n_out, int* info, int* table, int table_cap,
                         int* n_table) {
    if (!in || !out || !info || n_in != RT_PK_N || n_out != RT_PKO_N || table_cap < 0) return RT_ERR_INVALID_ARG;
    if (n_table) *n_table = N_RENDER_KERNELS;
    if (table) {
        if (table_cap < N_RENDER_KERNELS) return RT_ERR_LIMIT;
        for (int i = 0; i < N_RENDER_KERNELS; i++) {
            table[2 * i] = RENDER_KERNELS[i].block;
            table[2 * i + 1] = RENDER_KERNELS[i].opt;
        }
    }
    static float4 there[1];   // plan_kernel asks only whether a buffer is there
    rt_kernel_args a = {};
    a.variant = in[RT_PK_VARIANT];
    a.block = in[RT_PK_BLOCK];
    a.n_active = in[RT_PK_N_ACTIVE];
    a.samples = in[RT_PK_SAMPLES] ? there : nullptr;
    a.sflags = in[RT_PK_SFLAGS] ? (uint8_t*)there : nullptr;
    a.wbuf = in[RT_PK_WBUF] ? there : nullptr;
    a.tile_list = in[RT_PK_TILE_LIST] ? (const int*)there : nullptr;
    a.n_nodes = in[RT_PK_N_NODES];
    a.n_lnode_f4 = in[RT_PK_N_LNODE_F4];
    a.lds_node_f4 = in[RT_PK_LDS_NODE_F4];
    a.lds_end_f4 = in[RT_PK_LDS_END_F4];
    a.n_f2inner = in[RT_PK_N_F2INNER];
    a.n_f2leaves = in[RT_PK_N_F2LEAVES];
    a.fastdiv = in[RT_PK_FASTDIV];
    a.box_all_cmp = in[RT_PK_BOX_ALL_CMP];
    a.box_interior = in[RT_PK_BOX_INTERIOR];
    a.sph_pairs = in[RT_PK_SPH_PAIRS];
    a.leaf_pf = in[RT_PK_LEAF_PF];
    a.media_sph = in[RT_PK_MEDIA_SPH];
    a.n_media = in[RT_PK_N_MEDIA];
    a.n_sph_lds = in[RT_PK_N_SPH_LDS];
    a.n_box_lds = in[RT_PK_N_BOX_LDS];
    a.perlin_lds = in[RT_PK_PERLIN_LDS];
    a.media_lds = in[RT_PK_MEDIA_LDS];
    a.sph_lds = in[RT_PK_SPH_LDS];
    a.box_cmp_lds = in[RT_PK_BOX_CMP_LDS];
    a.sph_mat_lds = in[RT_PK_SPH_MAT_LDS];
    a.box_mat_lds = in[RT_PK_BOX_MAT_LDS];
    a.tex_lds = in[RT_PK_TEX_LDS];
    a.box_margin = in[RT_PK_PRETEST] ? 1.0f : 0.0f;
    a.n_chunks = in[RT_PK_N_CHUNKS];
    a.spine_len = in[RT_PK_SPINE_LEN];
    a.walk_frac = in[RT_PK_WALK_FRAC];
    const KernelPlan k = plan_kernel(a, ab != 0);
    std::memset(out, 0, sizeof(int) * RT_PKO_N);
    std::memset(info, 0, sizeof(int) * RT_LI_N);
    out[RT_PKO_OK] = k.ok;
    out[RT_PKO_PERLIN_LDS] = a.perlin_lds;
    out[RT_PKO_MEDIA_LDS] = a.media_lds;
    out[RT_PKO_SPH_LDS] = a.sph_lds;
    out[RT_PKO_BOX_CMP_LDS] = a.box_cmp_lds;
    out[RT_PKO_SPH_MAT_LDS] = a.sph_mat_lds;
    out[RT_PKO_BOX_MAT_LDS] = a.box_mat_lds;
    out[RT_PKO_TEX_LDS] = a.tex_lds;
    out[RT_PKO_ACC_LDS] = a.acc_lds;
    out[RT_PKO_LEAF_PF] = a.leaf_pf;
    if (!k.ok) return RT_OK;
    out[RT_PKO_SHAPE] = k.shape;
    out[RT_PKO_STATS] = k.stats;
    out[RT_PKO_POOL] = k.pool;
    out[RT_PKO_BLOCK] = k.block;
    out[RT_PKO_OPT] = k.opt;
    out[RT_PKO_LDS_BYTES] = (int)k.lds;
    std::memcpy(info, k.info, sizeof(int) * RT_LI_N);
    return RT_OK;
}

// rt_debug_plan_kernel's RT_PK_* view of a launch's arguments (the inverse of its reading above)
static void pk_from_args(const rt_kernel_args& a, int* pk) {
    pk[RT_PK_VARIANT] = a.variant;
    pk[RT_PK_BLOCK] = a.block;
    pk[RT_PK_N_ACTIVE] = a.n_active;
    pk[RT_PK_SAMPLES] = a.samples != nullptr;
    pk[RT_PK_SFLAGS] = a.sflags != nullptr;
    pk[RT_PK_WBUF] = a.wbuf != nullptr;
    pk[RT_PK_TILE_LIST] = a.tile_list != nullptr;
    pk[RT_PK_N_NODES] = a.n_nodes;
    pk[RT_PK_N_LNODE_F4] = a.n_lnode_f4;
    pk[RT_PK_LDS_NODE_F4] = a.lds_node_f4;
    pk[RT_PK_LDS_END_F4] = a.lds_end_f4;
    pk[RT_PK_N_F2INNER] = a.n_f2inner;
    pk[RT_PK_N_F2LEAVES] = a.n_f2leaves;
    pk[RT_PK_FASTDIV] = a.fastdiv;
    pk[RT_PK_BOX_ALL_CMP] = a.box_all_cmp;
    pk[RT_PK_BOX_INTERIOR] = a.box_interior;
    pk[RT_PK_SPH_PAIRS] = a.sph_pairs;
    pk[RT_PK_LEAF_PF] = a.leaf_pf;
    pk[RT_PK_MEDIA_SPH] = a.media_sph;
    pk[RT_PK_N_MEDIA] = a.n_media;
    pk[RT_PK_N_SPH_LDS] = a.n_sph_lds;
    pk[RT_PK_N_BOX_LDS] = a.n_box_lds;
    pk[RT_PK_PERLIN_LDS] = a.perlin_lds;
    pk[RT_PK_MEDIA_LDS] = a.media_lds;
    pk[RT_PK_SPH_LDS] = a.sph_lds;
    pk[RT_PK_BOX_CMP_LDS] = a.box_cmp_lds;
    pk[RT_PK_SPH_MAT_LDS] = a.sph_mat_lds;
    pk[RT_PK_BOX_MAT_LDS] = a.box_mat_lds;
    pk[RT_PK_TEX_LDS] = a.tex_lds;
    pk[RT_PK_PRETEST] = a.box_margin > 0.0f;
    pk[RT_PK_N_CHUNKS] = a.n_chunks;
    pk[RT_PK_SPINE_LEN] = a.spine_len;
    pk[RT_PK_WALK_FRAC] = a.walk_frac;
}

int rt_debug_plan_scene(const rt_debug_scene_in* in, rt_debug_scene_out* out) {
    if (!in || !out || !in->camera || in->first_frame < 1 || in->n_frames < 0 || in->waves < 0 || in->n_options < 0 ||
        (in->n_options && !in->options) || (in->n_mask > 0 && !in->mask))
        return RT_ERR_INVALID_ARG;
    // rt_resize's and rt_set_partition's argument checks
    if (in->width <= 0 || in->height <= 0 || in->width > RT_MAX_IMAGE_DIM || in->height > RT_MAX_IMAGE_DIM ||
        (size_t)in->width * in->height > ((size_t)1 << 30) || in->world < 1 || in->rank < 0 || in->rank >= in->world ||
        in->stripe_rows < 1 || in->max_depth < 0 || (in->bvh_mode != RT_BVH_REFERENCE && in->bvh_mode != RT_BVH_SAH))
        return RT_ERR_INVALID_ARG;
    static float4 there[1];   // stands for a buffer the device part of rt_render would hold
    int* const tile_frames = out->tile_frames;
    const int tile_cap = out->tile_cap;
    void* const links = out->links;
    void* const args = out->args;
    const size_t links_cap = out->links_cap, args_cap = out->args_cap;
    std::memset(out, 0, sizeof(*out));
    out->tile_frames = tile_frames; out->tile_cap = tile_cap;
    out->links = links; out->links_cap = links_cap;
    out->args = args; out->args_cap = args_cap;
    SceneState s;
    int r;
    for (int k = 0; k < in->n_options; k++)
        if ((r = set_option(s, in->options[2 * k], in->options[2 * k + 1], in->ab != 0, nullptr))) return r;
    s.bvh_mode = in->bvh_mode;
    for (int b = 0; b < 6; b++) {
        BufferPrep p;
        if ((r = prep_buffer(s, b, in->buf[b], in->buf_bytes[b], p, nullptr))) return r;
    }
    for (int t = 0; t < RT_MAX_TEXTURES; t++) {
        if (in->tex_w[t] == 0) continue;
        TexturePrep p;
        if ((r = prep_texture(t, in->tex_format[t], in->tex_w[t], in->tex_h[t], in->tex[t], p, nullptr))) return r;
        set_texture(s, t, in->tex_format[t], in->tex_w[t], in->tex_h[t], !p.pk.empty());
    }
    set_camera(s, in->camera);
    s.max_depth = in->max_depth;
    std::memcpy(s.background, in->background, 12);
    s.sqrt_spp = in->sqrt_spp;
    s.recip_sqrt_spp = in->recip_sqrt_spp;
    s.width = in->width; s.height = in->height;
    s.proc_rank = in->rank; s.proc_world = in->world; s.stripe_rows = in->stripe_rows;
    s.moments = in->moments != 0;
    const int local_rows = local_rows_of(s.height, in->rank, in->world, s.stripe_rows);
    const int nt = tile_count(s.width, local_rows);
    if (in->n_mask >= 0) {
        for (int k = 0; k < in->n_mask; k++)
            if (in->mask[k] < 0 || in->mask[k] >= nt || (k && in->mask[k] <= in->mask[k - 1])) return RT_ERR_INVALID_ARG;
        s.mask_set = true;
        s.act_list.assign(in->mask, in->mask + in->n_mask);
    }
    s.moments_frames = in->prev_frames;
    if (in->prev_tile_frames) s.tile_frames.assign(in->prev_tile_frames, in->prev_tile_frames + nt);
    // rt_render from here
    if ((r = validate(s, nullptr))) return r;
    rt_kernel_args a;
    if ((r = scene_args(s, a, nullptr))) return r;
    const bool mom = s.moments && in->n_frames > 0 && local_rows > 0;
    if (s.mask_set && !pooled_variant(s.variant)) return RT_ERR_STATE;
    FrameCounts after;
    after.all = s.moments_frames;
    after.tiles = s.tile_frames;
    if (in->n_frames > 0 && local_rows > 0)
        after = step_frame_counts(s.moments_frames, s.tile_frames, nt, s.mask_set ? &s.act_list : nullptr, in->first_frame,
                                  in->n_frames);
    out->frames_all = after.all;
    out->n_tile_frames = (int)after.tiles.size();
    if (!after.tiles.empty()) {
        if (!tile_frames || tile_cap < (int)after.tiles.size()) return RT_ERR_LIMIT;
        std::memcpy(tile_frames, after.tiles.data(), after.tiles.size() * sizeof(int32_t));
    }
    out->links_f4 = (int)s.walk_links.size();
    if (links) {
        if (links_cap < s.walk_links.size() * sizeof(float4)) return RT_ERR_LIMIT;
        if (!s.walk_links.empty()) std::memcpy(links, s.walk_links.data(), s.walk_links.size() * sizeof(float4));
    }
    out->args_bytes = sizeof(rt_kernel_args);
    if (args && args_cap < sizeof(rt_kernel_args)) return RT_ERR_LIMIT;
    int info[RT_LI_N] = {0};
    if (!(s.mask_set && s.act_list.empty()) && in->n_frames > 0 && local_rows > 0) {
        // the device's part of rt_render (render_device) as numbers: bind_device's stripe, then the plans
        a.local_rows = local_rows;
        a.rank = in->rank;
        a.world = in->world;
        const Split split = plan_device(s, local_rows, in->waves, in->free_bytes, mom, in->n_frames, a);
        a.tile_list = s.mask_set ? (const int*)there : nullptr;
        const LaunchPlan p = plan_launch(s, split, mom, in->waves, in->first_frame, in->n_frames, 0, a);
        a.samples = p.stage ? there : nullptr;
        a.sflags = p.sparse ? (uint8_t*)there : nullptr;
        a.wbuf = p.wave_slots ? there : nullptr;
        out->launched = 1;
        pk_from_args(a, out->pk);
        out->per_launch = split.per_launch; out->chunks_wanted = split.chunks_wanted; out->staged = split.staged;
        out->n_chunks = a.n_chunks; out->chunk_frames = a.chunk_frames; out->tail_chunks = a.tail_chunks;
        out->stage = p.stage;
        rt_kernel_args planned = a;   // (plan_kernel edits its copy: args stays what rt_render assembled)
        const KernelPlan k = plan_kernel(planned, in->ab != 0);
        if (k.ok) std::memcpy(info, k.info, sizeof(info));
        launch_report(s, a, info, out->first_leaf);
        out->bvh_mode = info[RT_LI_BVH_MODE]; out->vnodes = info[RT_LI_VNODES];
        out->collapsed = info[RT_LI_COLLAPSED]; out->rebuilt = info[RT_LI_REBUILT];
        std::memcpy(out->first_leaf_args, a.first_leaf, sizeof(out->first_leaf_args));
        out->spine_start = a.spine_start;
        a.samples = nullptr; a.sflags = nullptr; a.wbuf = nullptr; a.tile_list = nullptr;
        if (args) std::memcpy(args, &a, sizeof(a));
    } else if (args) {
        std::memset(args, 0, sizeof(rt_kernel_args));
    }
    return RT_OK;
}

int rt_debug_perlin_pack(const float* texels, int w, int h, void* out, size_t out_cap) {
    if (!texels || w <= 0 || h <= 0) return RT_ERR_INVALID_ARG;
    std::vector<float4> pk;
    if (!perlin_pack(texels, w, h, pk)) return 0;
    if (out) {
        if (out_cap < pk.size() * sizeof(float4)) return RT_ERR_INVALID_ARG;
        if (!pk.empty()) std::memcpy(out, pk.data(), pk.size() * sizeof(float4));
    }
    return 1;
}

int rt_debug_sphere_pair_leaves(const void* bvh, size_t nbytes, int* permille) {
    if (!bvh || !permille || nbytes % sizeof(rt_bvh_node)) return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)bvh, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    *permille = pair_leaves_permille(build_links(dn), (int)dn.size());
    return RT_OK;
}

int rt_debug_fast_tables(const void* bvh, size_t nbytes, const void* quads, size_t qbytes, const void* boxes,
                         size_t bbytes, int n_spheres, void* nodes_out, size_t nodes_cap, int* n_per_octant,
                         uint32_t* info_out, size_t info_cap, int* slots_out, int* n_slots) {
    if (!bvh || nbytes % sizeof(rt_bvh_node) || qbytes % sizeof(rt_quad) || bbytes % sizeof(rt_box) || n_spheres < 0 ||
        !n_per_octant || !n_slots || (qbytes && !quads) || (bbytes && !boxes))
        return RT_ERR_INVALID_ARG;
    std::vector<rt_dnode> dn;
    int r = thread_bvh((const rt_bvh_node*)bvh, (int)(nbytes / sizeof(rt_bvh_node)), dn, nullptr);
    if (r) return r;
    FastTables F = build_fast(dn, (size_t)n_spheres, (const rt_quad*)quads, qbytes / sizeof(rt_quad),
                              (const rt_box*)boxes, bbytes / sizeof(rt_box));
    *n_per_octant = F.n_per;
    *n_slots = F.fm_n;
    if (nodes_out) {
        if (nodes_cap < F.nodes.size() * sizeof(rt_dnode)) return RT_ERR_INVALID_ARG;
        if (!F.nodes.empty()) std::memcpy(nodes_out, F.nodes.data(), F.nodes.size() * sizeof(rt_dnode));
    }
    if (info_out) {
        if (info_cap < F.info.size() * sizeof(uint32_t)) return RT_ERR_INVALID_ARG;
        if (!F.info.empty()) std::memcpy(info_out, F.info.data(), F.info.size() * sizeof(uint32_t));
    }
    if (slots_out)
        for (int j = 0; j < F.fm_n; j++) {
            slots_out[4 * j + 0] = F.fm_medium[j];
            slots_out[4 * j + 1] = F.fm_leaf[j];
            slots_out[4 * j + 2] = F.fm_track[j];
            slots_out[4 * j + 3] = F.fm_flags[j];
        }
    return (F.ok && boxes_nest(dn)) ? 1 : 0;
}

int rt_debug_build_sah_bvh(const void* spheres, size_t sph_bytes, const void* quads, size_t quad_bytes,
                           const void* media, size_t med_bytes, const void* boxes, size_t box_bytes,
                           const void* bvh, size_t bvh_bytes, int order, const float eye[3],
                           float prim_cost, void* out, size_t out_cap, size_t* nbytes) {
    if (!nbytes || (bvh_bytes && !bvh) || order < 0 || order > 2 || !(prim_cost > 0.0f)) return RT_ERR_INVALID_ARG;
    rt_sah::Input in;
    in.sph = (const rt_sphere*)spheres;
    in.n_sph = spheres ? sph_bytes / sizeof(rt_sphere) : 0;
    in.quad = (const rt_quad*)quads;
    in.n_quad = quads ? quad_bytes / sizeof(rt_quad) : 0;
    in.med = (const rt_medium*)media;
    in.n_med = media ? med_bytes / sizeof(rt_medium) : 0;
    in.box = (const rt_box*)boxes;
    in.n_box = boxes ? box_bytes / sizeof(rt_box) : 0;
    in.ref = (const rt_bvh_node*)bvh;
    in.n_ref = bvh_bytes / sizeof(rt_bvh_node);
    std::vector<rt_bvh_node> t;
    rt_sah::Builder b(in, order, eye, prim_cost);
    if (!b.build(t)) return RT_ERR_INVALID_ARG;
    *nbytes = t.size() * sizeof(rt_bvh_node);
    if (!out) return RT_OK;
    if (out_cap < *nbytes) return RT_ERR_LIMIT;
    std::memcpy(out, t.data(), *nbytes);
    return RT_OK;
}

}  // extern "C"
