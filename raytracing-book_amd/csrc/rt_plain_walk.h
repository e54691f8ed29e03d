// rt_plain_walk.h -- the plain closest-hit walk of one ray: the link walk from the root over a plain
// link buffer in global memory (SceneState::links: rt_prep.cpp build_links of the current tree, without
// pre-test nodes, collapse or spine) and the generic leaf tests, one leaf at a time.  The same leaves
// in the same order, under the same ray_t.max, as whatever form the render's launch plan walks
// (DESIGN §2).  Used by the first-hit pass (rt_features.hip) and by rt_debug_eval_shade_op's
// RT_SOP_TRACE (rt_shade_eval.hip); the render kernels' translation units do not include it.
#ifndef RT_PLAIN_WALK_H
#define RT_PLAIN_WALK_H

#include "rt_kernel_common.h"

namespace {

// A new walk's set-up as rt_kernel.hip render_stream writes it out (its BEGIN block; kept in step by
// hand), then rounds of link_walk + leaf_prims_t<false, FD> until the walk ends.  On return `has`
// says whether anything was hit, tmax is the closest hit's t (RT_INFINITY on a miss), h its tif and
// the uv the walk wrote, rf the rand factor after the media's draws.
// MEDIA false: leaf slots of type RT_MODEL_CONSTANT_MEDIUM are cleared before the leaf tests, so no
// rand() is drawn and rf is never read.
template <bool FD, bool MEDIA>
__device__ __forceinline__ void plain_walk(const KP& P, const float4* __restrict__ links, int n_nodes, v3 o, v3 d,
                                           float time, float& rf, float px, float py, Hit& h, bool& has,
                                           float& tmax) {
    h.t = 0.0f; h.tif = 0;
    h.uv_kind_idx = 0; h.uv_a = 0.0f; h.uv_b = 0.0f;
    has = false;
    tmax = RT_INFINITY;
    const bool dir_zero = (d.x == 0.0f) && (d.y == 0.0f) && (d.z == 0.0f);   // hits nothing (bounce())
    if (dir_zero || n_nodes <= 0) return;
    const v3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const float a = g_dot(d, d);
    const bool exact = (inv.x == -INFINITY) || (inv.y == -INFINITY) || (inv.z == -INFINITY);
    const NodeSrc ns = {nullptr, reinterpret_cast<const char*>(links), 0u, nullptr};   // every node from global memory
    const uint2* leaves = reinterpret_cast<const uint2*>(links + 2 * (size_t)n_nodes);
    uint32_t nx = 0;
    for (;;) {
        nx = exact ? link_walk<true, false, true>(ns, nx, o, inv, 0.001f, tmax, nullptr)
                   : link_walk<false, false, true>(ns, nx, o, inv, 0.001f, tmax, nullptr);
        if (nx == RT_LINK_END) break;
        const uint2 lf = ldg_u2(leaves + (nx & 0x7FFFFFFFu));
        uint32_t ty = lf.x & 0xFFu;
        if (!MEDIA) {   // the leaf's two type nibbles with a medium's cleared: an empty slot tests nothing
            if ((ty & 0xFu) == RT_MODEL_CONSTANT_MEDIUM) ty &= 0xF0u;
            if ((ty >> 4) == RT_MODEL_CONSTANT_MEDIUM) ty &= 0x0Fu;
        }
        leaf_prims_t<false, FD>(P, ty << 16, lf.y, o, d, inv, a, time, 0.001f, tmax, rf, px, py, h, has, nullptr);
        nx = lf.x >> 8;   // the leaf's skip node
        if (nx == RT_LINK_NEXT_END) break;
    }
}

}  // namespace

#endif
