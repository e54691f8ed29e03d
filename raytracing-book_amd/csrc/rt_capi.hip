// rt_capi.hip — implementation of include/rt/rt.h (the drop-in C ABI).
//
// Host-side responsibilities that the reference's Java/GL layer had:
// buffer/texture upload (BufferObject.uploadData, Texture.putData), uniforms
// (ShaderProgram.setUniform*), dispatch (RaytraceExecutor.raytrace), readback
// (glGetTexImage) and timing (QueryTimer).  Plus the MI355X-specific parts:
// RGB8->RGBA8 texture expansion, stripe partitioning across devices/processes
// and caller-owned device images.  The scene preparation (the threaded-BVH
// re-layout among it) is rt_prep.cpp, the launch planning rt_plan.cpp, RCCL
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
#include "bvh_sah.h"

using namespace rt_impl;

namespace rt_impl __attribute__((visibility("hidden"))) {

// The fast mode's tree (bvh_sah.h) over the uploaded BVH's prims; child order: the one nearer the
// camera first.
int build_sah(rt_ctx* c, std::vector<rt_bvh_node>& out) {
    rt_sah::Input in;
    in.sph = (const rt_sphere*)c->host_buf[RT_BIND_SPHERES].data();
    in.n_sph = c->host_buf[RT_BIND_SPHERES].size() / sizeof(rt_sphere);
    in.quad = (const rt_quad*)c->host_buf[RT_BIND_QUADS].data();
    in.n_quad = c->host_buf[RT_BIND_QUADS].size() / sizeof(rt_quad);
    in.med = (const rt_medium*)c->host_buf[RT_BIND_MEDIA].data();
    in.n_med = c->host_buf[RT_BIND_MEDIA].size() / sizeof(rt_medium);
    in.box = (const rt_box*)c->host_buf[RT_BIND_BOXES].data();
    in.n_box = c->host_buf[RT_BIND_BOXES].size() / sizeof(rt_box);
    in.ref = (const rt_bvh_node*)c->host_buf[RT_BIND_BVH].data();
    in.n_ref = c->host_buf[RT_BIND_BVH].size() / sizeof(rt_bvh_node);
    rt_sah::Builder b(in, 2, c->cam.camera_pos);
    if (!b.build(out)) return set_err(c, RT_ERR_INVALID_ARG, "SAH BVH: the uploaded BVH's prims cannot be rebuilt");
    if (out.size() > RT_MAX_RECORDS) return set_err(c, RT_ERR_LIMIT, "SAH BVH exceeds 65535 nodes");
    return RT_OK;
}

int validate(rt_ctx* c) {
    if (c->validated) return RT_OK;
    size_t ns = c->host_buf[RT_BIND_SPHERES].size() / sizeof(rt_sphere);
    size_t nq = c->host_buf[RT_BIND_QUADS].size() / sizeof(rt_quad);
    size_t nb = c->host_buf[RT_BIND_BOXES].size() / sizeof(rt_box);
    size_t nm = c->host_buf[RT_BIND_MEDIA].size() / sizeof(rt_medium);
    auto check_ref = [&](int type, int idx) -> bool {
        switch (type) {
            case RT_MODEL_SPHERE: return (size_t)idx < ns;
            case RT_MODEL_QUAD: return (size_t)idx < nq;
            case RT_MODEL_BOX: return (size_t)idx < nb;
            case RT_MODEL_CONSTANT_MEDIUM: return (size_t)idx < nm;
            default: return true;   // unknown types never hit (hit_model returns false)
        }
    };
    const rt_bvh_node* nodes = (const rt_bvh_node*)c->host_buf[RT_BIND_BVH].data();
    size_t nn = c->host_buf[RT_BIND_BVH].size() / sizeof(rt_bvh_node);
    for (size_t i = 0; i < nn; i++) {
        int lt = nodes[i].left_id & 0xFFFF;
        if (lt == 0) continue;
        if (!check_ref(lt, (nodes[i].left_id >> 16) & 0xFFFF) || !check_ref(nodes[i].right_id & 0xFFFF, (nodes[i].right_id >> 16) & 0xFFFF))
            return set_err(c, RT_ERR_INVALID_ARG, "BVH leaf references a missing record");
    }
    const rt_medium* media = (const rt_medium*)c->host_buf[RT_BIND_MEDIA].data();
    c->uv_always = false;
    for (size_t i = 0; i < nm; i++) {
        int bt = media[i].boundary_type;
        if (bt == RT_MODEL_CONSTANT_MEDIUM) return set_err(c, RT_ERR_INVALID_ARG, "medium boundary cannot be a medium");
        if (!check_ref(bt, media[i].boundary_idx) || media[i].boundary_idx < 0)
            return set_err(c, RT_ERR_INVALID_ARG, "medium boundary references a missing record");
        if (((media[i].texture_id >> 28) & 0xF) == RT_TEXTYPE_IMAGE) c->uv_always = true;
    }
    const std::vector<uint8_t>& L = c->host_buf[RT_BIND_LIGHTS];
    if (L.size() >= 4) {
        int32_t count;
        std::memcpy(&count, L.data(), 4);
        if (count < 0 || (size_t)(count + 1) * 4 > L.size()) return set_err(c, RT_ERR_INVALID_ARG, "lights count exceeds buffer");
        for (int i = 0; i < count; i++) {
            int32_t p;
            std::memcpy(&p, L.data() + 4 + 4 * i, 4);
            int t = (p >> 16) & 0xFFFF, ix = p & 0xFFFF;
            if ((t == RT_MODEL_SPHERE || t == RT_MODEL_QUAD) && !check_ref(t, ix))
                return set_err(c, RT_ERR_INVALID_ARG, "light references a missing record");
        }
    }
    // exact near-first walk tables (variant 60): rebuilt after every upload
    const std::vector<uint8_t>& QB = c->host_buf[RT_BIND_QUADS];
    const std::vector<uint8_t>& BB = c->host_buf[RT_BIND_BOXES];
    c->fast = build_fast(c->dnodes, ns, (const rt_quad*)QB.data(), nq, (const rt_box*)BB.data(), nb);
    c->fast.ok = c->fast.ok && c->spec_ok && !c->uv_always;
    if (c->bvh_mode == RT_BVH_SAH) {
        std::vector<rt_bvh_node> sah;
        int r = build_sah(c, sah);
        if (r) return r;
        std::vector<rt_dnode> dn;
        r = thread_bvh(sah.data(), (int)sah.size(), dn, &c->err);
        if (r) return r;
        c->links = build_links(dn);
        c->n_link_nodes = (int)dn.size();
        c->sah_bvh.assign((const uint8_t*)sah.data(), (const uint8_t*)(sah.data() + sah.size()));
        c->walk_dn.swap(dn);
    } else {
        c->links = build_links(c->dnodes);
        c->n_link_nodes = c->n_dnodes;
        c->sah_bvh.clear();
        c->walk_dn = c->dnodes;
    }
    c->walk_stale = true;
    c->pair_leaves = -1;
    c->fast_gen++;
    c->validated = true;
    return RT_OK;
}

}  // namespace rt_impl

namespace {

// every tile holds frames 1 .. n (0: none valid): the uniform form of the per-tile counts (rt_ctx.h)
void set_all_frames(rt_ctx* c, int n) {
    c->moments_frames = n;
    c->tile_frames.clear();
}

// the links the launch walks: with the box pre-test nodes (option box_vnodes) when every box has a
// compact record and the pre-test is on (its margin is the nodes' growth: rebuilt when it changes)
void refresh_walk(rt_ctx* c, float box_margin) {
    const size_t nb = c->host_buf[RT_BIND_BOXES].size() / sizeof(rt_box);
    const bool all_cmp = c->compact_boxes && nb > 0 && c->n_boxc_ok == (int)nb;
    const bool use_v = c->box_vnodes && all_cmp && box_margin > 0.0f && (c->variant == 0 || c->variant == 39) &&
                       c->boxc_host.size() == nb * RT_BOXC_F4;
    // node collapse (plan_collapse): planned for the camera, so rebuilt when it or the image size changes
    const bool use_c = c->collapse && (c->variant == 0 || c->variant == 39) && c->have_cam;
    const bool cam_moved = use_c && (std::memcmp(&c->walk_cam, &c->cam, sizeof(rt_camera_ubo)) != 0 ||
                                     c->walk_w != c->width || c->walk_h != c->height);
    const bool use_r = c->rebuild > 0 && (c->variant == 0 || c->variant == 39);
    if (c->walk_stale || use_v != c->walk_v || (use_v && box_margin != c->walk_v_margin) ||
        use_c != c->walk_c || cam_moved || use_r != c->walk_r || c->rebuild != c->walk_rmode) {
        if (c->walk_stale) c->rb_mode = -1;   // a new walk_dn (validate)
        if (use_r && c->rb_mode != c->rebuild) {
            c->rb_dn = rebuild_inner(c->walk_dn, c->rebuild);
            c->rb_mode = c->rebuild;
        }
        static const std::vector<rt_dnode> none;
        const std::vector<rt_dnode>& rb = use_r ? c->rb_dn : none;
        const std::vector<rt_dnode>& wdn = rb.empty() ? c->walk_dn : rb;
        std::vector<uint8_t> drop;
        if (use_c) {
            try {
                if (!c->inj_hits.empty() && c->inj_hits.size() >= wdn.size()) {
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
                            if (order[q] < wdn.size()) H[order[q]] = c->inj_hits[q];
                    drop = plan_from_hits(wdn, H, c->inj_walks);
                } else {
                    drop = plan_collapse(wdn, c->cam, c->width, c->height);
                }
            } catch (const std::bad_alloc&) {   // no plan: the walk keeps every node
                drop.clear();
            }
        }
        c->n_dropped = 0;
        for (uint8_t x : drop) c->n_dropped += x;
        const std::vector<uint8_t>* dp = c->n_dropped ? &drop : nullptr;
        if (use_v) {
            // the kernel's pre-test bounds (leaf_prims_t): compact record c0 = (mn.x, mn.y, mn.z,
            // mx.x), c1 = (mx.y, mx.z, ..), each grown by the margin with the same float operations
            const float m = box_margin;
            std::vector<float> vb(6 * nb);
            for (size_t b = 0; b < nb; b++) {
                const float4 c0 = c->boxc_host[b * RT_BOXC_F4], c1 = c->boxc_host[b * RT_BOXC_F4 + 1];
                const float g[6] = {c0.x - m, c0.w + m, c0.y - m, c1.x + m, c0.z - m, c1.y + m};
                std::memcpy(&vb[6 * b], g, sizeof(g));
            }
            int nn = 0;
            c->walk_links = build_links(wdn, &vb, &nn, dp);
            c->n_walk_nodes = nn;
            c->n_vnodes = std::max(0, nn - ((int)wdn.size() - (dp ? c->n_dropped : 0)));
        } else if (dp || !rb.empty()) {
            int nn = 0;
            c->walk_links = build_links(wdn, nullptr, &nn, dp);
            c->n_walk_nodes = nn;
        } else {
            c->walk_links = c->links;
            c->n_walk_nodes = c->n_link_nodes;
        }
        if (!use_v) c->n_vnodes = 0;
        c->walk_c = use_c;
        c->walk_r = use_r;
        c->walk_rmode = c->rebuild;
        c->n_rebuilt = rb.empty() ? 0 : (int)rb.size();
        c->walk_cam = c->cam;
        c->walk_w = c->width;
        c->walk_h = c->height;
        c->walk_v = use_v;
        c->walk_v_margin = use_v ? box_margin : -1.0f;
        c->walk_stale = false;
        c->pair_leaves = -1;
        c->fast_gen++;   // re-upload the links (rt_render's device loop)
    }

}

// the device's copies of the scene, its image, counters and stripe in the kernel arguments
void bind_device(const rt_ctx* c, const Device& d, rt_kernel_args& a) {
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
    for (int t = 0; t < 8; t++) {
        a.tex[t].data = d.tex[t].ptr;
        a.tex[t].w = c->tex_w[t];
        a.tex[t].h = c->tex_h[t];
        a.tex[t].is_float = c->tex_format[t] == RT_TEX_R32F;
    }
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
    if (binding < 0 || binding > 5) return set_err(c, RT_ERR_INVALID_ARG, "binding must be 0..5");
    if (nbytes && !bytes) return set_err(c, RT_ERR_INVALID_ARG, "NULL bytes");
    static const size_t rec[6] = {sizeof(rt_sphere), sizeof(rt_bvh_node), sizeof(rt_quad), sizeof(rt_medium),
                                  sizeof(rt_box), 4};
    if (nbytes % rec[binding]) return set_err(c, RT_ERR_INVALID_ARG, "size is not a multiple of the std430 record size");
    if (binding != RT_BIND_LIGHTS && nbytes / rec[binding] > RT_MAX_RECORDS)
        return set_err(c, RT_ERR_LIMIT, "more than 65535 records");
    if (binding == RT_BIND_LIGHTS && nbytes < 4) return set_err(c, RT_ERR_INVALID_ARG, "lights buffer needs the count word");
    std::vector<uint8_t> dev_bytes;
    const void* src = bytes;
    size_t n = nbytes;
    // Thread the incoming BVH before anything of the context changes: a rejected
    // BVH leaves the previous one (host copy, threaded nodes, device buffers) intact.
    std::vector<rt_dnode> dn;
    if (binding == RT_BIND_BVH) {
        int r = thread_bvh((const rt_bvh_node*)bytes, (int)(nbytes / sizeof(rt_bvh_node)), dn, &c->err);
        if (r) return r;
        dev_bytes.assign((uint8_t*)dn.data(), (uint8_t*)dn.data() + dn.size() * sizeof(rt_dnode));
        src = dev_bytes.data();
        n = dev_bytes.size();
    }
    std::vector<uint8_t>& H = c->host_buf[binding];
    H.assign((const uint8_t*)bytes, (const uint8_t*)bytes + nbytes);
    c->uploaded[binding] = true;
    c->validated = false;
    c->scene_extent = -1.0f;
    if (binding == RT_BIND_BVH) {
        c->n_dnodes = (int)dn.size();
        c->spec_ok = boxes_nest(dn);
        c->dnodes.swap(dn);
        c->inj_hits.clear();   // measured node hits belong to the previous tree
        c->inj_walks = 0;
    }
    std::vector<float4> faces;   // intersection-only copy of quads / box sides
    std::vector<float4> boxc;    // compact canonical box records
    if (binding == RT_BIND_QUADS) {
        c->fd_ok[binding] = prep_quads((const rt_quad*)bytes, nbytes / sizeof(rt_quad), faces);
    } else if (binding == RT_BIND_BOXES) {
        BoxPrep P = prep_boxes((const rt_quad*)bytes, nbytes / sizeof(rt_box));
        c->boxes_canon = P.canon;
        c->boxes_cond = P.cond;
        c->fd_ok[binding] = P.fd;
        c->n_boxc_ok = P.n_compact;
        c->boxc_host = P.boxc;
        faces.swap(P.faces);
        boxc.swap(P.boxc);
    } else if (binding == RT_BIND_SPHERES) {
        c->fd_ok[binding] = spheres_fd((const rt_sphere*)bytes, nbytes / sizeof(rt_sphere));
    }
    if (binding == RT_BIND_LIGHTS) {
        src = (const uint8_t*)bytes + 4;
        n = nbytes - 4;
    }
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
        int r = dev_alloc_copy(c, d, *b, src, n);
        if (r) return r;
        if (binding == RT_BIND_QUADS || binding == RT_BIND_BOXES) {
            r = dev_alloc_copy(c, d, binding == RT_BIND_QUADS ? d.dquads : d.dboxes, faces.data(),
                               faces.size() * sizeof(float4));
            if (r) return r;
        }
        if (binding == RT_BIND_BOXES) {
            r = dev_alloc_copy(c, d, d.dboxc, boxc.data(), boxc.size() * sizeof(float4));
            if (r) return r;
        }
    }
    return RT_OK;
}

int rt_upload_texture(rt_ctx* c, int slot, int format, int w, int h, const void* texels) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (slot < 0 || slot >= RT_MAX_TEXTURES) return set_err(c, RT_ERR_LIMIT, "texture slot must be 0..7");
    if (w <= 0 || h <= 0 || !texels) return set_err(c, RT_ERR_INVALID_ARG, "bad texture size or NULL texels");
    if ((size_t)w * h > (size_t)1 << 28) return set_err(c, RT_ERR_LIMIT, "texture too large");
    size_t n = (size_t)w * h;
    std::vector<uint32_t> rgba;
    const void* src = texels;
    size_t bytes = n * 4;
    if (format == RT_TEX_RGB8) {
        rgba.resize(n);
        const uint8_t* p = (const uint8_t*)texels;
        for (size_t i = 0; i < n; i++)
            rgba[i] = (uint32_t)p[3 * i] | ((uint32_t)p[3 * i + 1] << 8) | ((uint32_t)p[3 * i + 2] << 16) | 0xFF000000u;
        src = rgba.data();
    } else if (format != RT_TEX_RGBA8 && format != RT_TEX_R32F) {
        return set_err(c, RT_ERR_INVALID_ARG, "unknown texture format");
    }
    // A Perlin table (texture.glsl:38-77: R32F, 6 x 256, columns ranvec x y z, perm x y z) whose
    // perm entries are whole numbers 0..255 is also kept as 256 float4 (ranvec x y z, the three
    // perm entries packed as bytes 0 / 1 / 2 of the fourth word): the kernel's noise then reads
    // one float4 per lattice corner and needs no float-to-int conversions or bounds checks
    // (every index is & 255 or an xor of bytes), the same values as the reference's texelFetch +
    // int() of the texture (rt_kernel.hip perlin_noise_pk).
    std::vector<float4> pk;
    if (format == RT_TEX_R32F && !perlin_pack((const float*)texels, w, h, pk)) pk.clear();
    for (Device& d : c->devs) {
        int r = dev_alloc_copy(c, d, d.tex[slot], src, bytes);
        if (r) return r;
        if (!pk.empty()) {
            r = dev_alloc_copy(c, d, d.perlin_pk, pk.data(), pk.size() * sizeof(float4));
            if (r) return r;
        }
    }
    if (!pk.empty()) c->perlin_pk_slot = slot;
    else if (c->perlin_pk_slot == slot) c->perlin_pk_slot = -1;
    c->tex_format[slot] = format;
    c->tex_w[slot] = w;
    c->tex_h[slot] = h;
    return RT_OK;
}

int rt_set_camera(rt_ctx* c, const float ubo[28]) {
    if (!c || !ubo) return set_err(c, RT_ERR_INVALID_ARG, "NULL camera");
    std::memcpy(&c->cam, ubo, sizeof(rt_camera_ubo));
    c->have_cam = true;
    c->scene_extent = -1.0f;
    c->fd_cam = true;   // the camera's points and vectors within the fast-division regime's 2^20
    for (int i = 0; i < 28; i++) c->fd_cam = c->fd_cam && fd_coord(ubo[i]);
    if (c->bvh_mode == RT_BVH_SAH) c->validated = false;   // the SAH tree orders children by the camera
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
    std::memset(&a, 0, sizeof(a));
    if (c->bvh_mode == RT_BVH_SAH && c->variant != 0 && c->variant != 39)
        return set_err(c, RT_ERR_STATE, "the SAH BVH runs on the default kernel structure only");
    a.watchdog_ticks = c->watchdog_ticks;
    a.chunk_wait_ticks = c->chunk_wait_ticks;
    int32_t lc = 0;
    if (c->host_buf[RT_BIND_LIGHTS].size() >= 4) std::memcpy(&lc, c->host_buf[RT_BIND_LIGHTS].data(), 4);
    a.lights_count = lc;
    a.uv_always = c->uv_always;
    a.boxes_canon = c->boxes_canon ? 1 : 0;
    // Box pre-test (rt_kernel.hip leaf_prims_t): a face the exact test accepts lies, with
    // the ray's point at its t, within ~2^-20 of the scene's extent of the box's bounds
    // (the face tests' rounding, amplified at most 2x by a well-conditioned 2-D solve:
    // boxes_cond); the kernel's slab test of the bounds grown by 2^-13 of that extent
    // cannot miss it.
    if (c->scene_extent < 0.0f) {
        const auto &S = c->host_buf[RT_BIND_SPHERES], &Q = c->host_buf[RT_BIND_QUADS], &B = c->host_buf[RT_BIND_BOXES];
        c->scene_extent = scene_extent((const rt_sphere*)S.data(), S.size() / sizeof(rt_sphere), (const rt_quad*)Q.data(),
                                       Q.size() / sizeof(rt_quad), (const rt_quad*)B.data(), B.size() / sizeof(rt_quad), c->cam);
    }
    a.box_margin = (c->boxes_cond && c->box_pretest && c->scene_extent <= 0x1p60f)
                       ? std::max(c->scene_extent, 1.0f) * 0x1p-13f
                       : 0.0f;
    a.fastdiv = (c->fastdiv && c->fd_cam && c->fd_ok[RT_BIND_SPHERES] && c->fd_ok[RT_BIND_QUADS] &&
                 c->fd_ok[RT_BIND_BOXES])
                    ? 1
                    : 0;
    a.variant = c->variant;
    a.zero_dir_end = c->zero_dir_end ? 1 : 0;
    a.sm_batch = c->sm_batch;
    a.walk_frac = c->walk_frac ? c->walk_frac : walk_frac_for(c->n_link_nodes);   // by the tree, not the pre-test nodes
    const FastTables& F = c->fast;
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
    a.debug_flags = c->debug_flags;
    a.box_interior = c->box_interior ? 1 : 0;
    refresh_walk(c, a.box_margin);
    a.box_vnodes = c->walk_v && c->n_vnodes > 0 ? 1 : 0;
    a.n_nodes = c->n_walk_nodes;
    a.n_lnode_f4 = (int)c->walk_links.size();
    // (a chain that ends at its leaf counts at any length where the kernel may hold the first-leaf
    // prologue: the compact-box kernels with the division-free box test, rt_plan.cpp)
    const size_t nb_all = c->host_buf[RT_BIND_BOXES].size() / sizeof(rt_box);
    const bool leaf_chain = c->first_leaf && c->box_interior && c->compact_boxes && nb_all > 0 &&
                            c->n_boxc_ok == (int)nb_all && (c->variant == 0 || c->variant == 39);
    plan_spine(c->walk_links, c->n_walk_nodes, c->cam, c->spine, leaf_chain, a);
    // the first-leaf prologue (rt_kernel.hip render_stream; option first_leaf): armed when the spine is
    // on and ends at the chain's leaf; the kernel gets that leaf's record as the walk's leaf stage reads it
    if (c->first_leaf && a.spine_len > 0 && (a.spine_start & RT_LINK_LEAF) && a.spine_start != RT_LINK_END) {
        const size_t ord = a.spine_start & 0x7FFFFFFFu, nf4 = 2 * (size_t)c->n_walk_nodes;
        if (nf4 + ord / 2 < c->walk_links.size()) {
            uint32_t w[4];
            std::memcpy(w, &c->walk_links[nf4 + ord / 2], 16);
            a.first_leaf[0] = 1u;
            a.first_leaf[1] = w[2 * (ord & 1)];
            a.first_leaf[2] = w[2 * (ord & 1) + 1];
        }
    }
    const bool pooled = c->variant == 0 || c->variant == 39;
    const int n_sph = (int)(c->host_buf[RT_BIND_SPHERES].size() / sizeof(rt_sphere));
    const int n_box = (int)(c->host_buf[RT_BIND_BOXES].size() / sizeof(rt_box));
    const int n_med = (int)(c->host_buf[RT_BIND_MEDIA].size() / sizeof(rt_medium));
    a.n_media = n_med;
    a.media_sph = 1;
    for (int k = 0; k < n_med; k++) {
        rt_medium m;
        std::memcpy(&m, c->host_buf[RT_BIND_MEDIA].data() + k * sizeof(rt_medium), sizeof m);
        if (m.boundary_type != RT_MODEL_SPHERE) a.media_sph = 0;
    }
    a.n_sph_lds = n_sph;
    a.n_box_lds = n_box;
    a.box_all_cmp = (c->compact_boxes && n_box > 0 && c->n_boxc_ok == n_box) ? 1 : 0;
    // the sphere-pair kernels (rt_kernel.hip leaf_prims_t SPAIR) for a BVH whose leaves are mostly
    // two spheres (scene 0: 485 spheres); measured slower where they are not
    if (c->pair_leaves < 0) c->pair_leaves = pair_leaves_permille(c->walk_links, c->n_walk_nodes);
    // option sphere_pairs = 2: the pair kernels whatever the share, compact-box kernels included
    a.sph_pairs = c->sphere_pairs == 2 ? 2 : (c->sphere_pairs && c->pair_leaves >= 500) ? 1 : 0;
    // the shading batch threshold by kernel: 50/64 of the walking lanes in the compact-box kernels, 52 in
    // the sphere-pair kernels (round 6, on their branchless walk: scene 0 -0.4%, twice,
    // profiles/r06_ag_opts_s0.log, r06_ah_opts_s0.log), 56 otherwise
    a.sm_frac = c->sm_frac ? c->sm_frac : (a.box_all_cmp ? 50 : (a.sph_pairs == 1 ? 52 : 56));
    a.perlin_slot = -1;
    for (int t = 0; t < RT_MAX_TEXTURES && a.perlin_slot < 0; t++)
        if (c->tex_format[t] == RT_TEX_R32F && c->tex_w[t] == 6) a.perlin_slot = t;
    a.perlin_packed = (a.perlin_slot >= 0 && a.perlin_slot == c->perlin_pk_slot && c->perlin_pk) ? 1 : 0;
    {   // the LDS layout (plan_lds) and what decides it
        LdsIn in{};
        in.variant = c->variant; in.n_walk_nodes = c->n_walk_nodes; in.n_lnode_f4 = a.n_lnode_f4;
        in.n_sph = n_sph; in.n_box = n_box; in.n_med = n_med;
        in.box_all_cmp = a.box_all_cmp != 0; in.perlin_packed = a.perlin_packed != 0;
        std::memcpy(in.tex_w, c->tex_w, sizeof(in.tex_w));
        std::memcpy(in.tex_h, c->tex_h, sizeof(in.tex_h));
        in.sph_lds = c->sph_lds; in.big_wg = c->big_wg; in.tl_small_lds = c->tl_small_lds;
        in.tl_leaf_lds = c->tl_leaf_lds; in.shade_lds = c->shade_lds; in.leaf_prefetch = c->leaf_prefetch;
        in.lds_node_cap = c->lds_node_cap; in.walk_frac = c->walk_frac;
        plan_lds(in, a);
    }
    a.cam = c->cam;
    std::memcpy(a.background, c->background, 12);
    a.max_depth = c->max_depth;
    a.sqrt_spp = c->sqrt_spp;
    a.recip_sqrt_spp = c->recip_sqrt_spp;
    a.width = c->width;
    a.height = c->height;
    a.stripe_rows = c->stripe_rows;
    // Sample moments: every launch staged (one frame or one chunk too) and folded by
    // fold_moments_kernel.  The moments follow frames 1 .. moments_frames: a render from frame 1
    // restarts them (the fold zeroes them at frame 1), one from moments_frames + 1 extends them,
    // any other leaves them invalid.
    const bool mom = c->moments && n_frames > 0 && c->devs[0].local_rows > 0;   // (a rank may own no row)
    if (mom && !c->devs[0].m2.ptr) return set_err(c, RT_ERR_STATE, "sample moments: no buffer (rt_resize)");
    // A tile mask (rt_set_active_tiles): the units run over the active tiles alone.
    const bool masked = c->mask_set;
    if (masked && c->variant != 0 && c->variant != 39)
        return set_err(c, RT_ERR_STATE, "a tile mask runs on the default kernel structure only");
    // The per-tile frame counts (rt_ctx.h) of the tiles this call samples: from frame 1 they restart,
    // from their count + 1 they extend, anything else leaves them invalid; the other tiles keep theirs.
    // A single-device context keeps them with the moments off too (the image's frames).
    const bool track = (mom || c->devs.size() == 1) && n_frames > 0 && c->devs[0].local_rows > 0;
    int all_after = c->moments_frames;
    std::vector<int32_t> tiles_after;
    if (track) {
        auto step = [&](int cnt) {
            return (first_frame == 1 || (cnt > 0 && first_frame == cnt + 1)) ? first_frame - 1 + n_frames : 0;
        };
        if (!masked && c->tile_frames.empty()) {
            all_after = step(c->moments_frames);
        } else {
            const int nt = ((c->width + 7) / 8) * ((c->devs[0].local_rows + 7) / 8);
            tiles_after = c->tile_frames;
            if (tiles_after.empty()) tiles_after.assign((size_t)nt, c->moments_frames);
            if (masked) {
                for (int32_t t : c->act_list) tiles_after[(size_t)t] = step(tiles_after[(size_t)t]);
            } else {
                for (int32_t& v : tiles_after) v = step(v);
            }
            all_after = nt > 0 ? *std::min_element(tiles_after.begin(), tiles_after.end()) : 0;
            if (nt == 0 || all_after == *std::max_element(tiles_after.begin(), tiles_after.end())) tiles_after.clear();
        }
        if (!masked || !c->act_list.empty()) set_all_frames(c, 0);   // until every launch is queued
    }
    for (Device& d : c->devs) {
        HIPCHK(c, hipSetDevice(d.id));
        if (masked && c->act_list.empty()) {
            // no tile to sample: nothing is launched or read; the events keep rt_sync / rt_last_render_ns working
            HIPCHK(c, hipEventRecord(d.ev_start, d.stream));
            HIPCHK(c, hipEventRecord(d.ev_stop, d.stream));
            d.timed = true;
            c->last_launch[RT_LI_TILES_ACTIVE] = 0;   // (the other fields keep the previous launch's)
            c->launched = c->launched || n_frames > 0;
            continue;
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
        // frames per launch and the unit split (plan_split); a staged launch's colours take at most
        // half the device's free memory (what this context already holds counts as free)
        const int n_tiles = ((c->width + 7) / 8) * ((d.local_rows + 7) / 8);
        const long long waves = rt_resident_waves();
        const size_t n_pixels = (size_t)d.local_rows * c->width;
        size_t free_b = 0, total_b = 0;
        const size_t avail = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b + d.samples.bytes : SIZE_MAX;
        // under a mask the split counts the active tiles, so a sparse one is still cut into enough units
        // per resident wave; staging stays indexed by pixel (its layout and size do not change)
        const int n_act = masked ? (int)c->act_list.size() : n_tiles;
        a.tile_list = masked ? (const int*)d.tile_list.ptr : nullptr;
        a.n_active = n_act;
        const Split split = plan_split(n_act, waves, n_frames, c->chunk_target, c->staged_chunk_target, c->stage_tiles,
                                       mom, n_pixels, c->sample_budget, avail);
        const int per_launch = split.per_launch, chunks_wanted = split.chunks_wanted;
        const bool staged = split.staged;
        const size_t launch_frames = (size_t)std::min(per_launch, std::max(n_frames, 1));
        if (staged && (r = ensure(c, d, d.samples, n_pixels * sizeof(float4) * launch_frames))) return r;
        a.n_pixels = n_pixels;
        if (!staged && chunks_wanted > 1 && (r = ensure(c, d, d.tile_done, sizeof(unsigned) * (size_t)n_tiles))) return r;
        a.tile_done = (unsigned*)d.tile_done.ptr;
        a.fault = (unsigned*)d.counter.ptr + 1;
        HIPCHK(c, hipEventRecord(d.ev_start, d.stream));
        for (int f0 = 0; f0 < n_frames; f0 += per_launch) {
            int nf = std::min(per_launch, n_frames - f0);
            a.first_frame = first_frame + f0;
            a.n_frames = nf;
            const int tail = c->tail_chunks >= 0 ? c->tail_chunks : tail_chunks_for(c->n_link_nodes);
            const Chunks ch = plan_chunks(nf, chunks_wanted, staged, mom, tail, pooled);
            a.n_chunks = ch.n_chunks;
            a.chunk_frames = ch.chunk_frames;
            a.tail_chunks = ch.tail_chunks;
            a.samples = ch.stage ? (float4*)d.samples.ptr : nullptr;
            // Sparse staging (render_stream): most samples' colours are exactly zero (scene 8: 96%:
            // a path that ends without reaching the light), so each sample writes a flag byte and
            // only the others their 16-byte colour; fold_kernel reads a clear flag as the zero
            // colour.  (A per-(chunk, pixel) bit word set by atomics measured slower: scene 6 +2.5%.)
            a.sflags = nullptr;
            if (a.samples && c->sparse_stage && pooled) {
                if ((r = ensure(c, d, d.sflags, n_pixels * launch_frames))) return r;
                a.sflags = (uint8_t*)d.sflags.ptr;
            }
            a.wbuf = nullptr;
            a.wbuf_waves = 0;
            if (!a.samples && pooled) {
                // pooled units fold per wave; two slots per wave (render_stream keeps two units in flight)
                if ((r = ensure(c, d, d.wbuf, (size_t)waves * 2 * 64 * (size_t)a.chunk_frames * sizeof(float4)))) return r;
                a.wbuf = (float4*)d.wbuf.ptr;
                a.wbuf_waves = (int)waves;
            }
            std::memcpy(a.rand_factors, rand_factors + f0, sizeof(float) * nf);
            int slot = d.ring_pos++ % Device::kRing;
            HIPCHK(c, hipEventSynchronize(d.ring_ev[slot]));   // the copy that last used this slot is done
            d.ring[slot] = a;
            if (rt_launch_render(d.ring[slot], (rt_kernel_args*)d.args.ptr, d.stream,
                                 &d == &c->devs[0] ? c->last_launch : nullptr, mom ? d.m2.ptr : nullptr))
                return set_err(c, RT_ERR_DEVICE, std::string("kernel launch failed: ") +
                                                     hipGetErrorString(hipGetLastError()));
            HIPCHK(c, hipEventRecord(d.ring_ev[slot], d.stream));
            if (&d == &c->devs[0]) {
                c->staged_frames = a.samples ? nf : 0;
                c->staged_sparse = a.samples && a.sflags;
                c->last_launch[RT_LI_BVH_MODE] = c->bvh_mode;
                c->last_launch[RT_LI_VNODES] = a.box_vnodes ? c->n_vnodes : 0;
                c->last_launch[RT_LI_COLLAPSED] = c->walk_c ? c->n_dropped : 0;
                c->last_launch[RT_LI_REBUILT] = c->n_rebuilt > 0 ? 1 : 0;
                // (rt_debug_first_leaf) the prologue is compiled into the RT_OPT_BOXQ kernels alone
                const bool fl = a.first_leaf[0] != 0 && c->last_launch[RT_LI_BOXQ] != 0;
                c->first_leaf_last[0] = fl ? 1 : 0;
                c->first_leaf_last[1] = fl ? (int)a.spine_start : 0;
                c->first_leaf_last[2] = fl ? (int)(a.first_leaf[1] & 0xFFu) : 0;
                c->first_leaf_last[3] = fl ? (int)a.first_leaf[2] : 0;
            }
        }
        HIPCHK(c, hipEventRecord(d.ev_stop, d.stream));
        d.timed = true;
        c->launched = c->launched || n_frames > 0;
    }
    if (track) {
        c->moments_frames = all_after;
        c->tile_frames.swap(tiles_after);
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
    const int n = ((c->width + 7) / 8) * ((d.local_rows + 7) / 8);
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
int tile_count(const rt_ctx* c) { return ((c->width + 7) / 8) * ((c->devs[0].local_rows + 7) / 8); }
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
        c->validated = false;   // validate() rebuilds the links (and a new fast_gen re-uploads them)
    }
    return RT_OK;
}

}  // extern "C"
