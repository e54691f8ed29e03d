// rt_args.cpp — from the host's copy of a scene to the render kernel's arguments (rt_args.h): plain
// C++, no HIP runtime call and no device, built once and linked into both libraries like rt_prep.cpp.
// rt_capi.hip's entries call these and then do the device's part; rt_debug_plan_scene
// (rt_debug_host.cpp) calls the same and reports the result.
#include <cstddef>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>

#include "rt_args.h"
#include "bvh_sah.h"

namespace rt_impl {

namespace {
int fail(std::string* err, int code, const char* m) {
    if (err) *err = m;
    return code;
}
const size_t kRecord[6] = {sizeof(rt_sphere), sizeof(rt_bvh_node), sizeof(rt_quad), sizeof(rt_medium), sizeof(rt_box), 4};
}  // namespace

size_t SceneState::n_records(int binding) const { return host_buf[binding].size() / kRecord[binding]; }

bool all_boxes_compact(const SceneState& s) {
    const size_t nb = s.n_records(RT_BIND_BOXES);
    return s.compact_boxes && nb > 0 && s.n_boxc_ok == (int)nb;
}

int set_option(SceneState& s, int option, int v, bool ab, std::string* err) {
    auto bad = [&]() { return fail(err, RT_ERR_INVALID_ARG, "option value out of range"); };
    switch (option) {
        case RT_OPTION_BOX_PRETEST: s.box_pretest = v != 0; break;
        case RT_OPTION_FASTDIV: s.fastdiv = v != 0; break;
        case RT_OPTION_SPH_LDS: s.sph_lds = v != 0; break;
        case RT_OPTION_BIG_WG: s.big_wg = v != 0; break;
        case RT_OPTION_COMPACT_BOXES: s.compact_boxes = v != 0; break;
        case RT_OPTION_SPINE: s.spine = v != 0; break;
        case RT_OPTION_TL_LEAF_LDS: s.tl_leaf_lds = v != 0; break;
        case RT_OPTION_PERLIN_PACKED: s.perlin_pk = v != 0; break;
        case RT_OPTION_SPARSE_STAGE: s.sparse_stage = v != 0; break;
        case RT_OPTION_SPHERE_PAIRS: if (v < 0 || v > 2) return bad(); s.sphere_pairs = v; break;
        case RT_OPTION_LEAF_PREFETCH: s.leaf_prefetch = v != 0; break;
        case RT_OPTION_TL_SMALL_LDS: s.tl_small_lds = v != 0; break;
        case RT_OPTION_SHADE_LDS: s.shade_lds = v != 0; break;
        case RT_OPTION_BOX_VNODES: s.box_vnodes = v != 0; break;
        case RT_OPTION_BOX_INTERIOR: s.box_interior = v != 0; break;
        case RT_OPTION_ZERO_DIR_END: s.zero_dir_end = v != 0; break;
        case RT_OPTION_FIRST_LEAF: s.first_leaf = v != 0; break;
        case RT_OPTION_COLLAPSE: s.collapse = v != 0; break;
        case RT_OPTION_REBUILD: if (v < 0 || v > 2) return bad(); s.rebuild = v; break;
        case RT_OPTION_CHUNK_TARGET: if (v < 0) return bad(); s.chunk_target = v; break;
        case RT_OPTION_STAGED_CHUNK_TARGET: if (v < 1) return bad(); s.staged_chunk_target = v; break;
        case RT_OPTION_STAGE_TILES: if (v < 0) return bad(); s.stage_tiles = v; break;
        case RT_OPTION_SM_BATCH: if (v < 1 || v > 64) return bad(); s.sm_batch = v; break;
        case RT_OPTION_SM_FRAC: if (v < 0 || v > 64) return bad(); s.sm_frac = v; break;
        case RT_OPTION_WALK_FRAC: if (v < 0 || v > 64) return bad(); s.walk_frac = v; break;
        case RT_OPTION_WATCHDOG_MS: if (v < 0) return bad(); s.watchdog_ticks = (unsigned long long)v * 100000ull; break;
        case RT_OPTION_CHUNK_WAIT_MS: if (v < 0) return bad(); s.chunk_wait_ticks = (unsigned long long)v * 100000ull; break;
        case RT_OPTION_LDS_NODE_CAP: if (v < 0) return bad(); s.lds_node_cap = v; break;
        case RT_OPTION_TAIL_CHUNKS: if (v < -1 || v > RT_MAX_FRAMES_PER_LAUNCH) return bad(); s.tail_chunks = v; break;
        case RT_OPTION_KERNEL_VARIANT:
            if (!ab) return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
            if (!(v == 0 || v == 30 || v == 31 || v == 37 || v == 38 || v == 39 || v == 61 || v == 69)) return bad();
            s.variant = v;
            break;
        case RT_OPTION_DEBUG_FLAGS:
            if (!ab) return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
            s.debug_flags = v;
            break;
        default: return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
    }
    return RT_OK;
}

int get_option(const SceneState& s, int option, int* v, bool ab, std::string* err) {
    switch (option) {
        case RT_OPTION_BOX_PRETEST: *v = s.box_pretest; break;
        case RT_OPTION_FASTDIV: *v = s.fastdiv; break;
        case RT_OPTION_SPH_LDS: *v = s.sph_lds; break;
        case RT_OPTION_BIG_WG: *v = s.big_wg; break;
        case RT_OPTION_COMPACT_BOXES: *v = s.compact_boxes; break;
        case RT_OPTION_SPINE: *v = s.spine; break;
        case RT_OPTION_TL_LEAF_LDS: *v = s.tl_leaf_lds; break;
        case RT_OPTION_PERLIN_PACKED: *v = s.perlin_pk; break;
        case RT_OPTION_SPARSE_STAGE: *v = s.sparse_stage; break;
        case RT_OPTION_SPHERE_PAIRS: *v = s.sphere_pairs; break;
        case RT_OPTION_LEAF_PREFETCH: *v = s.leaf_prefetch; break;
        case RT_OPTION_TL_SMALL_LDS: *v = s.tl_small_lds; break;
        case RT_OPTION_SHADE_LDS: *v = s.shade_lds; break;
        case RT_OPTION_BOX_VNODES: *v = s.box_vnodes; break;
        case RT_OPTION_BOX_INTERIOR: *v = s.box_interior; break;
        case RT_OPTION_ZERO_DIR_END: *v = s.zero_dir_end; break;
        case RT_OPTION_FIRST_LEAF: *v = s.first_leaf; break;
        case RT_OPTION_COLLAPSE: *v = s.collapse; break;
        case RT_OPTION_REBUILD: *v = s.rebuild; break;
        case RT_OPTION_CHUNK_TARGET: *v = s.chunk_target; break;
        case RT_OPTION_STAGED_CHUNK_TARGET: *v = s.staged_chunk_target; break;
        case RT_OPTION_STAGE_TILES: *v = s.stage_tiles; break;
        case RT_OPTION_SM_BATCH: *v = s.sm_batch; break;
        case RT_OPTION_SM_FRAC: *v = s.sm_frac; break;
        case RT_OPTION_WALK_FRAC: *v = s.walk_frac; break;
        case RT_OPTION_WATCHDOG_MS: *v = (int)std::min<unsigned long long>(INT_MAX, s.watchdog_ticks / 100000ull); break;
        case RT_OPTION_CHUNK_WAIT_MS: *v = (int)std::min<unsigned long long>(INT_MAX, s.chunk_wait_ticks / 100000ull); break;
        case RT_OPTION_LDS_NODE_CAP: *v = s.lds_node_cap; break;
        case RT_OPTION_TAIL_CHUNKS: *v = s.tail_chunks; break;
        case RT_OPTION_KERNEL_VARIANT:
            if (!ab) return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
            *v = s.variant;
            break;
        case RT_OPTION_DEBUG_FLAGS:
            if (!ab) return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
            *v = s.debug_flags;
            break;
        default: return fail(err, RT_ERR_INVALID_ARG, "unknown option (A/B options need librtamd_ab.so)");
    }
    return RT_OK;
}

int prep_buffer(SceneState& s, int binding, const void* bytes, size_t nbytes, BufferPrep& out, std::string* err) {
    if (binding < 0 || binding > 5) return fail(err, RT_ERR_INVALID_ARG, "binding must be 0..5");
    if (nbytes && !bytes) return fail(err, RT_ERR_INVALID_ARG, "NULL bytes");
    if (nbytes % kRecord[binding]) return fail(err, RT_ERR_INVALID_ARG, "size is not a multiple of the std430 record size");
    if (binding != RT_BIND_LIGHTS && nbytes / kRecord[binding] > RT_MAX_RECORDS)
        return fail(err, RT_ERR_LIMIT, "more than 65535 records");
    if (binding == RT_BIND_LIGHTS && nbytes < 4) return fail(err, RT_ERR_INVALID_ARG, "lights buffer needs the count word");
    out.src = bytes;
    out.n = nbytes;
    // Thread the incoming BVH before anything of the scene changes: a rejected
    // BVH leaves the previous one (host copy, threaded nodes, device buffers) intact.
    std::vector<rt_dnode> dn;
    if (binding == RT_BIND_BVH) {
        int r = thread_bvh((const rt_bvh_node*)bytes, (int)(nbytes / sizeof(rt_bvh_node)), dn, err);
        if (r) return r;
        out.threaded.assign((uint8_t*)dn.data(), (uint8_t*)dn.data() + dn.size() * sizeof(rt_dnode));
        out.src = out.threaded.data();
        out.n = out.threaded.size();
    }
    s.host_buf[binding].assign((const uint8_t*)bytes, (const uint8_t*)bytes + nbytes);
    s.uploaded[binding] = true;
    s.validated = false;
    s.scene_extent = -1.0f;
    if (binding == RT_BIND_BVH) {
        s.n_dnodes = (int)dn.size();
        s.spec_ok = boxes_nest(dn);
        s.dnodes.swap(dn);
        s.inj_hits.clear();   // measured node hits belong to the previous tree
        s.inj_walks = 0;
    } else if (binding == RT_BIND_QUADS) {
        s.fd_ok[binding] = prep_quads((const rt_quad*)bytes, nbytes / sizeof(rt_quad), out.faces);
    } else if (binding == RT_BIND_BOXES) {
        BoxPrep P = prep_boxes((const rt_quad*)bytes, nbytes / sizeof(rt_box));
        s.boxes_canon = P.canon;
        s.boxes_cond = P.cond;
        s.fd_ok[binding] = P.fd;
        s.n_boxc_ok = P.n_compact;
        s.boxc_host = P.boxc;
        out.faces.swap(P.faces);
        out.boxc.swap(P.boxc);
    } else if (binding == RT_BIND_SPHERES) {
        s.fd_ok[binding] = spheres_fd((const rt_sphere*)bytes, nbytes / sizeof(rt_sphere));
    } else if (binding == RT_BIND_LIGHTS) {
        out.src = (const uint8_t*)bytes + 4;
        out.n = nbytes - 4;
    }
    return RT_OK;
}

int prep_texture(int slot, int format, int w, int h, const void* texels, TexturePrep& out, std::string* err) {
    if (slot < 0 || slot >= RT_MAX_TEXTURES) return fail(err, RT_ERR_LIMIT, "texture slot must be 0..7");
    if (w <= 0 || h <= 0 || !texels) return fail(err, RT_ERR_INVALID_ARG, "bad texture size or NULL texels");
    if ((size_t)w * h > (size_t)1 << 28) return fail(err, RT_ERR_LIMIT, "texture too large");
    const size_t n = (size_t)w * h;
    out.src = texels;
    out.bytes = n * 4;
    if (format == RT_TEX_RGB8) {
        out.rgba.resize(n);
        const uint8_t* p = (const uint8_t*)texels;
        for (size_t i = 0; i < n; i++)
            out.rgba[i] = (uint32_t)p[3 * i] | ((uint32_t)p[3 * i + 1] << 8) | ((uint32_t)p[3 * i + 2] << 16) | 0xFF000000u;
        out.src = out.rgba.data();
    } else if (format != RT_TEX_RGBA8 && format != RT_TEX_R32F) {
        return fail(err, RT_ERR_INVALID_ARG, "unknown texture format");
    }
    // A Perlin table (texture.glsl:38-77: R32F, 6 x 256, columns ranvec x y z, perm x y z) whose
    // perm entries are whole numbers 0..255 is also kept as 256 float4 (ranvec x y z, the three
    // perm entries packed as bytes 0 / 1 / 2 of the fourth word): the kernel's noise then reads
    // one float4 per lattice corner and needs no float-to-int conversions or bounds checks
    // (every index is & 255 or an xor of bytes), the same values as the reference's texelFetch +
    // int() of the texture (rt_kernel.hip perlin_noise_pk).
    if (format == RT_TEX_R32F && !perlin_pack((const float*)texels, w, h, out.pk)) out.pk.clear();
    return RT_OK;
}

void set_texture(SceneState& s, int slot, int format, int w, int h, bool packed) {
    if (packed) s.perlin_pk_slot = slot;
    else if (s.perlin_pk_slot == slot) s.perlin_pk_slot = -1;
    s.tex_format[slot] = format;
    s.tex_w[slot] = w;
    s.tex_h[slot] = h;
}

void set_camera(SceneState& s, const float ubo[28]) {
    std::memcpy(&s.cam, ubo, sizeof(rt_camera_ubo));
    s.have_cam = true;
    s.scene_extent = -1.0f;
    s.fd_cam = true;   // the camera's points and vectors within the fast-division regime's 2^20
    for (int i = 0; i < 28; i++) s.fd_cam = s.fd_cam && fd_coord(ubo[i]);
    if (s.bvh_mode == RT_BVH_SAH) s.validated = false;   // the SAH tree orders children by the camera
}

int build_sah(const SceneState& s, std::vector<rt_bvh_node>& out, std::string* err) {
    rt_sah::Input in;
    in.sph = (const rt_sphere*)s.host_buf[RT_BIND_SPHERES].data();
    in.n_sph = s.n_records(RT_BIND_SPHERES);
    in.quad = (const rt_quad*)s.host_buf[RT_BIND_QUADS].data();
    in.n_quad = s.n_records(RT_BIND_QUADS);
    in.med = (const rt_medium*)s.host_buf[RT_BIND_MEDIA].data();
    in.n_med = s.n_records(RT_BIND_MEDIA);
    in.box = (const rt_box*)s.host_buf[RT_BIND_BOXES].data();
    in.n_box = s.n_records(RT_BIND_BOXES);
    in.ref = (const rt_bvh_node*)s.host_buf[RT_BIND_BVH].data();
    in.n_ref = s.n_records(RT_BIND_BVH);
    rt_sah::Builder b(in, 2, s.cam.camera_pos);
    if (!b.build(out)) return fail(err, RT_ERR_INVALID_ARG, "SAH BVH: the uploaded BVH's prims cannot be rebuilt");
    if (out.size() > RT_MAX_RECORDS) return fail(err, RT_ERR_LIMIT, "SAH BVH exceeds 65535 nodes");
    return RT_OK;
}

int validate(SceneState& s, std::string* err) {
    if (s.validated) return RT_OK;
    const size_t ns = s.n_records(RT_BIND_SPHERES), nq = s.n_records(RT_BIND_QUADS), nb = s.n_records(RT_BIND_BOXES),
                 nm = s.n_records(RT_BIND_MEDIA);
    auto check_ref = [&](int type, int idx) -> bool {
        switch (type) {
            case RT_MODEL_SPHERE: return (size_t)idx < ns;
            case RT_MODEL_QUAD: return (size_t)idx < nq;
            case RT_MODEL_BOX: return (size_t)idx < nb;
            case RT_MODEL_CONSTANT_MEDIUM: return (size_t)idx < nm;
            default: return true;   // unknown types never hit (hit_model returns false)
        }
    };
    const rt_bvh_node* nodes = (const rt_bvh_node*)s.host_buf[RT_BIND_BVH].data();
    const size_t nn = s.n_records(RT_BIND_BVH);
    for (size_t i = 0; i < nn; i++) {
        int lt = nodes[i].left_id & 0xFFFF;
        if (lt == 0) continue;
        if (!check_ref(lt, (nodes[i].left_id >> 16) & 0xFFFF) || !check_ref(nodes[i].right_id & 0xFFFF, (nodes[i].right_id >> 16) & 0xFFFF))
            return fail(err, RT_ERR_INVALID_ARG, "BVH leaf references a missing record");
    }
    const rt_medium* media = (const rt_medium*)s.host_buf[RT_BIND_MEDIA].data();
    s.uv_always = false;
    for (size_t i = 0; i < nm; i++) {
        int bt = media[i].boundary_type;
        if (bt == RT_MODEL_CONSTANT_MEDIUM) return fail(err, RT_ERR_INVALID_ARG, "medium boundary cannot be a medium");
        if (!check_ref(bt, media[i].boundary_idx) || media[i].boundary_idx < 0)
            return fail(err, RT_ERR_INVALID_ARG, "medium boundary references a missing record");
        if (((media[i].texture_id >> 28) & 0xF) == RT_TEXTYPE_IMAGE) s.uv_always = true;
    }
    const std::vector<uint8_t>& L = s.host_buf[RT_BIND_LIGHTS];
    if (L.size() >= 4) {
        int32_t count;
        std::memcpy(&count, L.data(), 4);
        if (count < 0 || (size_t)(count + 1) * 4 > L.size()) return fail(err, RT_ERR_INVALID_ARG, "lights count exceeds buffer");
        for (int i = 0; i < count; i++) {
            int32_t p;
            std::memcpy(&p, L.data() + 4 + 4 * i, 4);
            int t = (p >> 16) & 0xFFFF, ix = p & 0xFFFF;
            if ((t == RT_MODEL_SPHERE || t == RT_MODEL_QUAD) && !check_ref(t, ix))
                return fail(err, RT_ERR_INVALID_ARG, "light references a missing record");
        }
    }
    // exact near-first walk tables (variant 60): rebuilt after every upload
    s.fast = build_fast(s.dnodes, ns, (const rt_quad*)s.host_buf[RT_BIND_QUADS].data(), nq,
                        (const rt_box*)s.host_buf[RT_BIND_BOXES].data(), nb);
    s.fast.ok = s.fast.ok && s.spec_ok && !s.uv_always;
    if (s.bvh_mode == RT_BVH_SAH) {
        std::vector<rt_bvh_node> sah;
        int r = build_sah(s, sah, err);
        if (r) return r;
        std::vector<rt_dnode> dn;
        r = thread_bvh(sah.data(), (int)sah.size(), dn, err);
        if (r) return r;
        s.links = build_links(dn);
        s.n_link_nodes = (int)dn.size();
        s.sah_bvh.assign((const uint8_t*)sah.data(), (const uint8_t*)(sah.data() + sah.size()));
        s.walk_dn.swap(dn);
    } else {
        s.links = build_links(s.dnodes);
        s.n_link_nodes = s.n_dnodes;
        s.sah_bvh.clear();
        s.walk_dn = s.dnodes;
    }
    s.walk_stale = true;
    s.pair_leaves = -1;
    s.fast_gen++;
    s.validated = true;
    return RT_OK;
}

void refresh_walk(SceneState& s, float box_margin) {
    const size_t nb = s.n_records(RT_BIND_BOXES);
    const bool pooled = pooled_variant(s.variant);
    const bool use_v = s.box_vnodes && all_boxes_compact(s) && box_margin > 0.0f && pooled &&
                       s.boxc_host.size() == nb * RT_BOXC_F4;
    // node collapse (plan_collapse): planned for the camera, so rebuilt when it or the image size changes
    const bool use_c = s.collapse && pooled && s.have_cam;
    const bool cam_moved = use_c && (std::memcmp(&s.walk_cam, &s.cam, sizeof(rt_camera_ubo)) != 0 ||
                                     s.walk_w != s.width || s.walk_h != s.height);
    const bool use_r = s.rebuild > 0 && pooled;
    if (!(s.walk_stale || use_v != s.walk_v || (use_v && box_margin != s.walk_v_margin) || use_c != s.walk_c ||
          cam_moved || use_r != s.walk_r || s.rebuild != s.walk_rmode))
        return;
    if (s.walk_stale) s.rb_mode = -1;   // a new walk_dn (validate)
    if (use_r && s.rb_mode != s.rebuild) {
        s.rb_dn = rebuild_inner(s.walk_dn, s.rebuild);
        s.rb_mode = s.rebuild;
    }
    static const std::vector<rt_dnode> none;
    const std::vector<rt_dnode>& rb = use_r ? s.rb_dn : none;
    const std::vector<rt_dnode>& wdn = rb.empty() ? s.walk_dn : rb;
    std::vector<uint8_t> drop;
    if (use_c) {
        try {
            if (!s.inj_hits.empty() && s.inj_hits.size() >= wdn.size()) {
                // measured hits, given per link node (breadth-first): back to dn's order
                std::vector<uint32_t> order{0u};
                for (size_t q = 0; q < order.size() && order.size() <= wdn.size(); q++) {
                    const uint32_t k = order[q];
                    if ((wdn[k].meta & 0xF0000u) != 0 || k + 1 >= wdn.size()) continue;
                    order.push_back(k + 1);
                    order.push_back(wdn[k + 1].meta & 0xFFFFu);
                }
                std::vector<int64_t> H(wdn.size(), 0);
                if (order.size() == wdn.size())
                    for (size_t q = 0; q < order.size(); q++)
                        if (order[q] < wdn.size()) H[order[q]] = s.inj_hits[q];
                drop = plan_from_hits(wdn, H, s.inj_walks);
            } else {
                drop = plan_collapse(wdn, s.cam, s.width, s.height);
            }
        } catch (const std::bad_alloc&) {   // no plan: the walk keeps every node
            drop.clear();
        }
    }
    s.n_dropped = 0;
    for (uint8_t x : drop) s.n_dropped += x;
    const std::vector<uint8_t>* dp = s.n_dropped ? &drop : nullptr;
    if (use_v) {
        // the kernel's pre-test bounds (leaf_prims_t): compact record c0 = (mn.x, mn.y, mn.z,
        // mx.x), c1 = (mx.y, mx.z, ..), each grown by the margin with the same float operations
        const float m = box_margin;
        std::vector<float> vb(6 * nb);
        for (size_t b = 0; b < nb; b++) {
            const float4 c0 = s.boxc_host[b * RT_BOXC_F4], c1 = s.boxc_host[b * RT_BOXC_F4 + 1];
            const float g[6] = {c0.x - m, c0.w + m, c0.y - m, c1.x + m, c0.z - m, c1.y + m};
            std::memcpy(&vb[6 * b], g, sizeof(g));
        }
        int nn = 0;
        s.walk_links = build_links(wdn, &vb, &nn, dp);
        s.n_walk_nodes = nn;
        s.n_vnodes = std::max(0, nn - ((int)wdn.size() - (dp ? s.n_dropped : 0)));
    } else if (dp || !rb.empty()) {
        int nn = 0;
        s.walk_links = build_links(wdn, nullptr, &nn, dp);
        s.n_walk_nodes = nn;
    } else {
        s.walk_links = s.links;
        s.n_walk_nodes = s.n_link_nodes;
    }
    if (!use_v) s.n_vnodes = 0;
    s.walk_c = use_c;
    s.walk_r = use_r;
    s.walk_rmode = s.rebuild;
    s.n_rebuilt = rb.empty() ? 0 : (int)rb.size();
    s.walk_cam = s.cam;
    s.walk_w = s.width;
    s.walk_h = s.height;
    s.walk_v = use_v;
    s.walk_v_margin = use_v ? box_margin : -1.0f;
    s.walk_stale = false;
    s.pair_leaves = -1;
    s.fast_gen++;   // re-upload the links (rt_render's device part)
}

int scene_args(SceneState& s, rt_kernel_args& a, std::string* err) {
    std::memset(&a, 0, sizeof(a));
    if (s.bvh_mode == RT_BVH_SAH && !pooled_variant(s.variant))
        return fail(err, RT_ERR_STATE, "the SAH BVH runs on the default kernel structure only");
    a.watchdog_ticks = s.watchdog_ticks;
    a.chunk_wait_ticks = s.chunk_wait_ticks;
    int32_t lc = 0;
    if (s.host_buf[RT_BIND_LIGHTS].size() >= 4) std::memcpy(&lc, s.host_buf[RT_BIND_LIGHTS].data(), 4);
    a.lights_count = lc;
    // (tests/test_shading_cases_design.py reads this word from rt_debug_plan_scene's argument block)
    static_assert(offsetof(rt_kernel_args, uv_always) == 80, "tests read uv_always at byte 80 of rt_kernel_args");
    a.uv_always = s.uv_always;
    a.boxes_canon = s.boxes_canon ? 1 : 0;
    // Box pre-test (rt_kernel.hip leaf_prims_t): a face the exact test accepts lies, with
    // the ray's point at its t, within ~2^-20 of the scene's extent of the box's bounds
    // (the face tests' rounding, amplified at most 2x by a well-conditioned 2-D solve:
    // boxes_cond); the kernel's slab test of the bounds grown by 2^-13 of that extent
    // cannot miss it.
    if (s.scene_extent < 0.0f)
        s.scene_extent = scene_extent((const rt_sphere*)s.host_buf[RT_BIND_SPHERES].data(), s.n_records(RT_BIND_SPHERES),
                                      (const rt_quad*)s.host_buf[RT_BIND_QUADS].data(), s.n_records(RT_BIND_QUADS),
                                      (const rt_quad*)s.host_buf[RT_BIND_BOXES].data(),
                                      s.host_buf[RT_BIND_BOXES].size() / sizeof(rt_quad), s.cam);
    a.box_margin = (s.boxes_cond && s.box_pretest && s.scene_extent <= 0x1p60f)
                       ? std::max(s.scene_extent, 1.0f) * 0x1p-13f
                       : 0.0f;
    a.fastdiv = (s.fastdiv && s.fd_cam && s.fd_ok[RT_BIND_SPHERES] && s.fd_ok[RT_BIND_QUADS] && s.fd_ok[RT_BIND_BOXES])
                    ? 1
                    : 0;
    a.variant = s.variant;
    a.zero_dir_end = s.zero_dir_end ? 1 : 0;
    a.sm_batch = s.sm_batch;
    a.walk_frac = s.walk_frac ? s.walk_frac : walk_frac_for(s.n_link_nodes);   // by the tree, not the pre-test nodes
    const FastTables& F = s.fast;
    a.fast_ok = F.ok ? 1 : 0;
    a.n_f2inner = (int)(F.inner2.size() / 4);
    a.n_f2leaves = (int)F.leaves2.size();
    a.f2depth = F.depth;
    std::memcpy(a.finfo_base, F.base, sizeof(a.finfo_base));
    a.fm_n = F.fm_n;
    std::memcpy(a.fm_medium, F.fm_medium, sizeof(a.fm_medium));
    std::memcpy(a.fm_leaf, F.fm_leaf, sizeof(a.fm_leaf));
    std::memcpy(a.fm_track, F.fm_track, sizeof(a.fm_track));
    std::memcpy(a.fm_flags, F.fm_flags, sizeof(a.fm_flags));
    a.fl_n = F.fl_n;
    std::memcpy(a.fl_medium, F.fl_medium, sizeof(a.fl_medium));
    std::memcpy(a.fl_rank, F.fl_rank, sizeof(a.fl_rank));
    a.debug_flags = s.debug_flags;
    a.box_interior = s.box_interior ? 1 : 0;
    refresh_walk(s, a.box_margin);
    a.box_vnodes = s.walk_v && s.n_vnodes > 0 ? 1 : 0;
    a.n_nodes = s.n_walk_nodes;
    a.n_lnode_f4 = (int)s.walk_links.size();
    a.box_all_cmp = all_boxes_compact(s) ? 1 : 0;
    // (a chain that ends at its leaf counts at any length where the kernel may hold the first-leaf
    // prologue: the compact-box kernels with the division-free box test, rt_plan.cpp)
    const bool leaf_chain = s.first_leaf && s.box_interior && a.box_all_cmp && pooled_variant(s.variant);
    plan_spine(s.walk_links, s.n_walk_nodes, s.cam, s.spine, leaf_chain, a);
    // the first-leaf prologue (rt_kernel.hip render_stream; option first_leaf): armed when the spine is
    // on and ends at the chain's leaf; the kernel gets that leaf's record as the walk's leaf stage reads it
    if (s.first_leaf && a.spine_len > 0 && (a.spine_start & RT_LINK_LEAF) && a.spine_start != RT_LINK_END) {
        const size_t ord = a.spine_start & 0x7FFFFFFFu, nf4 = 2 * (size_t)s.n_walk_nodes;
        if (nf4 + ord / 2 < s.walk_links.size()) {
            uint32_t w[4];
            std::memcpy(w, &s.walk_links[nf4 + ord / 2], 16);
            a.first_leaf[0] = 1u;
            a.first_leaf[1] = w[2 * (ord & 1)];
            a.first_leaf[2] = w[2 * (ord & 1) + 1];
        }
    }
    const int n_sph = (int)s.n_records(RT_BIND_SPHERES), n_box = (int)s.n_records(RT_BIND_BOXES),
              n_med = (int)s.n_records(RT_BIND_MEDIA);
    a.n_media = n_med;
    a.media_sph = 1;
    for (int k = 0; k < n_med; k++) {
        rt_medium m;
        std::memcpy(&m, s.host_buf[RT_BIND_MEDIA].data() + k * sizeof(rt_medium), sizeof m);
        if (m.boundary_type != RT_MODEL_SPHERE) a.media_sph = 0;
    }
    a.n_sph_lds = n_sph;
    a.n_box_lds = n_box;
    // the sphere-pair kernels (rt_kernel.hip leaf_prims_t SPAIR) for a BVH whose leaves are mostly
    // two spheres (scene 0: 485 spheres); measured slower where they are not
    if (s.pair_leaves < 0) s.pair_leaves = pair_leaves_permille(s.walk_links, s.n_walk_nodes);
    // option sphere_pairs = 2: the pair kernels whatever the share, compact-box kernels included
    a.sph_pairs = s.sphere_pairs == 2 ? 2 : (s.sphere_pairs && s.pair_leaves >= 500) ? 1 : 0;
    // the shading batch threshold by kernel: 50/64 of the walking lanes in the compact-box kernels, 52 in
    // the sphere-pair kernels (round 6, on their branchless walk: scene 0 -0.4%, twice,
    // profiles/r06_ag_opts_s0.log, r06_ah_opts_s0.log), 56 otherwise
    a.sm_frac = s.sm_frac ? s.sm_frac : (a.box_all_cmp ? 50 : (a.sph_pairs == 1 ? 52 : 56));
    for (int t = 0; t < RT_MAX_TEXTURES; t++) {
        a.tex[t].w = s.tex_w[t];
        a.tex[t].h = s.tex_h[t];
        a.tex[t].is_float = s.tex_format[t] == RT_TEX_R32F;
    }
    a.perlin_slot = -1;
    for (int t = 0; t < RT_MAX_TEXTURES && a.perlin_slot < 0; t++)
        if (s.tex_format[t] == RT_TEX_R32F && s.tex_w[t] == 6) a.perlin_slot = t;
    a.perlin_packed = (a.perlin_slot >= 0 && a.perlin_slot == s.perlin_pk_slot && s.perlin_pk) ? 1 : 0;
    {   // the LDS layout (plan_lds) and what decides it
        LdsIn in{};
        in.variant = s.variant; in.n_walk_nodes = s.n_walk_nodes; in.n_lnode_f4 = a.n_lnode_f4;
        in.n_sph = n_sph; in.n_box = n_box; in.n_med = n_med;
        in.box_all_cmp = a.box_all_cmp != 0; in.perlin_packed = a.perlin_packed != 0;
        std::memcpy(in.tex_w, s.tex_w, sizeof(in.tex_w));
        std::memcpy(in.tex_h, s.tex_h, sizeof(in.tex_h));
        in.sph_lds = s.sph_lds; in.big_wg = s.big_wg; in.tl_small_lds = s.tl_small_lds;
        in.tl_leaf_lds = s.tl_leaf_lds; in.shade_lds = s.shade_lds; in.leaf_prefetch = s.leaf_prefetch;
        in.lds_node_cap = s.lds_node_cap; in.walk_frac = s.walk_frac;
        plan_lds(in, a);
    }
    a.cam = s.cam;
    std::memcpy(a.background, s.background, 12);
    a.max_depth = s.max_depth;
    a.sqrt_spp = s.sqrt_spp;
    a.recip_sqrt_spp = s.recip_sqrt_spp;
    a.width = s.width;
    a.height = s.height;
    a.stripe_rows = s.stripe_rows;
    return RT_OK;
}

Split plan_device(const SceneState& s, int local_rows, long long waves, size_t free_bytes, bool mom, int n_frames,
                  rt_kernel_args& a) {
    a.n_pixels = (size_t)local_rows * s.width;
    // under a mask the split counts the active tiles, so a sparse one is still cut into enough units
    // per resident wave; staging stays indexed by pixel (its layout and size do not change)
    a.n_active = s.mask_set ? (int)s.act_list.size() : tile_count(s.width, local_rows);
    return plan_split(a.n_active, waves, n_frames, s.chunk_target, s.staged_chunk_target, s.stage_tiles, mom, a.n_pixels,
                      s.sample_budget, free_bytes);
}

LaunchPlan plan_launch(const SceneState& s, const Split& split, bool mom, long long waves, int first_frame, int n_frames,
                       int f0, rt_kernel_args& a) {
    const bool pooled = pooled_variant(s.variant);
    const int nf = std::min(split.per_launch, n_frames - f0);
    a.first_frame = first_frame + f0;
    a.n_frames = nf;
    const int tail = s.tail_chunks >= 0 ? s.tail_chunks : tail_chunks_for(s.n_link_nodes);
    const Chunks ch = plan_chunks(nf, split.chunks_wanted, split.staged, mom, tail, pooled);
    a.n_chunks = ch.n_chunks;
    a.chunk_frames = ch.chunk_frames;
    a.tail_chunks = ch.tail_chunks;
    LaunchPlan p;
    p.stage = ch.stage;
    // Sparse staging (render_stream): most samples' colours are exactly zero (scene 8: 96%:
    // a path that ends without reaching the light), so each sample writes a flag byte and
    // only the others their 16-byte colour; fold_kernel reads a clear flag as the zero
    // colour.  (A per-(chunk, pixel) bit word set by atomics measured slower: scene 6 +2.5%.)
    p.sparse = ch.stage && s.sparse_stage && pooled;
    // pooled units fold per wave; two slots per wave (render_stream keeps two units in flight)
    p.wave_slots = !ch.stage && pooled;
    p.launch_frames = (size_t)std::min(split.per_launch, std::max(n_frames, 1));
    a.wbuf_waves = p.wave_slots ? (int)waves : 0;
    return p;
}

void launch_report(const SceneState& s, const rt_kernel_args& a, int* info, int first_leaf_last[4]) {
    info[RT_LI_BVH_MODE] = s.bvh_mode;
    info[RT_LI_VNODES] = a.box_vnodes ? s.n_vnodes : 0;
    info[RT_LI_COLLAPSED] = s.walk_c ? s.n_dropped : 0;
    info[RT_LI_REBUILT] = s.n_rebuilt > 0 ? 1 : 0;
    // (rt_debug_first_leaf) the prologue is compiled into the RT_OPT_BOXQ kernels alone
    const bool fl = a.first_leaf[0] != 0 && info[RT_LI_BOXQ] != 0;
    first_leaf_last[0] = fl ? 1 : 0;
    first_leaf_last[1] = fl ? (int)a.spine_start : 0;
    first_leaf_last[2] = fl ? (int)(a.first_leaf[1] & 0xFFu) : 0;
    first_leaf_last[3] = fl ? (int)a.first_leaf[2] : 0;
}

FrameCounts step_frame_counts(int before_all, const std::vector<int32_t>& before_tiles, int n_tiles,
                              const std::vector<int32_t>* mask, int first_frame, int n_frames) {
    auto step = [&](int cnt) {
        return (first_frame == 1 || (cnt > 0 && first_frame == cnt + 1)) ? first_frame - 1 + n_frames : 0;
    };
    FrameCounts out;
    if (!mask && before_tiles.empty()) {
        out.all = step(before_all);
        return out;
    }
    out.tiles = before_tiles;
    if (out.tiles.empty()) out.tiles.assign((size_t)n_tiles, before_all);
    if (mask) {
        for (int32_t t : *mask) out.tiles[(size_t)t] = step(out.tiles[(size_t)t]);
    } else {
        for (int32_t& v : out.tiles) v = step(v);
    }
    out.all = n_tiles > 0 ? *std::min_element(out.tiles.begin(), out.tiles.end()) : 0;
    if (n_tiles == 0 || out.all == *std::max_element(out.tiles.begin(), out.tiles.end())) out.tiles.clear();
    return out;
}

}  // namespace rt_impl
