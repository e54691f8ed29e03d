// rt_features.hip — the first-hit pass (rt.h rt_render_features / rt_read_features): per pixel the
// centre ray's closest solid hit as two float4 buffers, normal_depth = (N, t) and albedo_id = (A, id).
// A translation unit of its own over rt_kernel_common.h, like rt_ops_eval.hip: the render kernels'
// code objects (rt_kernel.hip) do not see it, and it calls the device functions they call -- the
// link walk, the leaf tests, texture_color -- so a hit here has the bits of the render's.
//
// One lane per pixel, a wave = one 8x8 tile (the render's tile: coherent rays), four tiles per
// workgroup; no atomics, no persistent loop, no LDS.  The walk reads a plain link buffer
// (SceneState::links: rt_prep.cpp build_links of the current tree, reference or SAH, without
// pre-test nodes, collapse or spine) from global memory from the root: the same leaves in the same
// order as whatever form the render's launch plan walks.  The argument block is the
// pass's own: every LDS table off (-1), so the shared functions take their global-memory forms, and
// no box pre-test (box_margin 0).  Leaf slots of type RT_MODEL_CONSTANT_MEDIUM are cleared before the
// leaf tests (plain_walk's MEDIA = false), so no rand() is drawn anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>

#include "rt/rt.h"
#include "rt_ctx.h"
#include "rt_denoise.h"
#include "rt_kernel_common.h"
#include "rt_plain_walk.h"

namespace {

constexpr int kTilesPerBlock = 4;   // 256 threads: four waves, one 8x8 tile each

__global__ void __launch_bounds__(256) features_kernel(const KP* __restrict__ Pp, const float4* __restrict__ links,
                                                       int n_nodes, float4* __restrict__ nd, float4* __restrict__ ai) {
    const KP& P = *Pp;
    const int W = P.width, H = P.local_rows;
    const int tiles_x = (W + 7) >> 3, n_tiles = tiles_x * ((H + 7) >> 3);
    const int tile = (int)blockIdx.x * kTilesPerBlock + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    if (tile >= n_tiles) return;
    const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const size_t px = (size_t)y * W + x;
    // the pixel's base point with no sub-pixel offset, from a pinhole
    const float fx = (float)x, fy = (float)y;
    const v3 o = ld3(P.cam.camera_pos), d = sub3(pixel_base(P.cam, fx, fy), o);
    const float time = 0.0f;

    // the plain walk (rt_plain_walk.h) with media cleared: rf is never read (no medium is tested)
    Hit h;
    bool has;
    float tmax, rf = 0.0f;
    plain_walk<false, false>(P, links, n_nodes, o, d, time, rf, fx, fy, h, has, tmax);
    if (!has) {
        nd[px] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        ai[px] = make_float4(P.background[0], P.background[1], P.background[2], __uint_as_float(RT_FEATURE_MISS));
        return;
    }
    // shade()'s hit record from the records in global memory (every LDS table is off); its medium
    // branch is unreachable here: media slots are cleared before the leaf tests
    const float t = tmax;
    const v3 p = add3(o, scale3(d, t));
    const HitSurface hs = hit_surface<false, false>(P, h, d, p, time);
    // this hit's uv as after_trace() leaves it: the walk's last accepted hit is its closest
    UvSrc uvs = {0, 0.0f, 0.0f, 0.0f};
    walk_uv(h, o, d, uvs);
    const int mid = (hs.material >> 16) & 0xFFFF;
    const v3 alb = mid == RT_MAT_DIFFUSE_LIGHT ? hs.emis : texture_color<false, false>(P, p, hs.tex_id, uvs, time);
    const v3 normal = hs.normal;
    nd[px] = make_float4(normal.x, normal.y, normal.z, t);
    ai[px] = make_float4(alb.x, alb.y, alb.z, __uint_as_float((uint32_t)h.tif));
}

}  // namespace

namespace rt_impl {

void features_free(rt_ctx* c) {
    for (Device& d : c->devs) {
        dev_free(d.ft_nd);
        dev_free(d.ft_ai);
        dev_free(d.ft_links);
        dev_free(d.ft_args);
    }
    c->ft_args_host.clear();
    c->ft_valid = c->ft_links_ok = false;
}

}  // namespace rt_impl

using namespace rt_impl;

extern "C" {

int rt_render_features(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "rt_render_features needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, "rt_render_features: not under rt_set_partition");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "rt_resize before rt_render_features");
    if (!c->have_cam) return set_err(c, RT_ERR_STATE, "rt_set_camera before rt_render_features");
    if (!c->uploaded[RT_BIND_BVH]) return set_err(c, RT_ERR_STATE, "no BVH uploaded");
    int r = validate(c);
    if (r) return r;
    if (c->n_link_nodes > 0 && c->links.empty())
        return set_err(c, RT_ERR_LIMIT, "rt_render_features: the BVH has no link form (more than 65535 nodes)");
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows;
    const size_t n = (size_t)W * H;
    c->ft_valid = false;
    c->ft_gen++;   // whatever the buffers held, a reprojected result made from it no longer matches them
    if ((r = ensure(c, d, d.ft_nd, n * sizeof(float4)))) return r;
    if ((r = ensure(c, d, d.ft_ai, n * sizeof(float4)))) return r;
    if (!c->ft_links_ok) {   // (the copy waits for the stream: a queued pass keeps the links it was given)
        if ((r = dev_alloc_copy(c, d, d.ft_links, c->links.data(), c->links.size() * sizeof(float4)))) return r;
        c->ft_links_ok = true;
    }
    // the pass's argument block: the scene's records in global memory, no LDS table, no box pre-test
    rt_kernel_args a;
    std::memset(&a, 0, sizeof(a));
    a.perlin_slot = -1;
    clear_lds_tables(a, LDS_ALL);
    bind_scene(d, a);
    for (int t = 0; t < 8; t++) {
        a.tex[t].w = c->tex_w[t];
        a.tex[t].h = c->tex_h[t];
        a.tex[t].is_float = c->tex_format[t] == RT_TEX_R32F;
    }
    a.cam = c->cam;
    std::memcpy(a.background, c->background, sizeof(a.background));
    a.n_nodes = c->n_link_nodes;
    a.width = W;
    a.height = c->height;
    a.local_rows = H;
    a.world = 1;
    a.stripe_rows = c->stripe_rows;
    a.n_pixels = n;
    if (c->ft_args_host.size() != sizeof(a) || std::memcmp(c->ft_args_host.data(), &a, sizeof(a)) != 0 || !d.ft_args.ptr) {
        c->ft_args_host.clear();
        if ((r = ensure(c, d, d.ft_args, sizeof(a)))) return r;
        if ((r = h2d(c, d, d.ft_args.ptr, &a, sizeof(a)))) return r;
        c->ft_args_host.assign((const uint8_t*)&a, (const uint8_t*)&a + sizeof(a));
    }
    if (n == 0) {
        c->ft_valid = true;
        return RT_OK;
    }
    const int n_tiles = ((W + 7) / 8) * ((H + 7) / 8);
    hipLaunchKernelGGL(features_kernel, dim3((unsigned)((n_tiles + kTilesPerBlock - 1) / kTilesPerBlock)), dim3(256), 0,
                       d.stream, (const rt_kernel_args*)d.ft_args.ptr, (const float4*)d.ft_links.ptr, c->n_link_nodes,
                       (float4*)d.ft_nd.ptr, (float4*)d.ft_ai.ptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return set_err(c, RT_ERR_DEVICE, std::string("rt_render_features launch failed: ") + hipGetErrorString(e));
    c->ft_valid = true;
    return RT_OK;
}

int rt_read_features(rt_ctx* c, float* normal_depth, float* albedo_id) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!c->ft_valid || c->devs.size() != 1 || !c->devs[0].ft_nd.ptr || !c->devs[0].ft_ai.ptr)
        return set_err(c, RT_ERR_STATE, "rt_read_features: no first-hit features held (rt_render_features first)");
    int r = rt_sync(c);
    if (r) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    const size_t bytes = (size_t)d.local_rows * c->width * 16;
    if (normal_depth && (r = d2h(c, d, normal_depth, d.ft_nd.ptr, bytes))) return r;
    if (albedo_id && (r = d2h(c, d, albedo_id, d.ft_ai.ptr, bytes))) return r;
    return RT_OK;
}

}  // extern "C"
