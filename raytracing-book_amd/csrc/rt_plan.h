// rt_plan.h — launch planning of rt_render as pure functions (rt_plan.cpp): the LDS layout of the
// link-format shapes, the frames per launch and the split of one launch into chunks.  Host-only
// and context-free: every input is a plain value, so which inputs decide a layout can be read
// off the signatures.
#pragma once

#include <cstddef>

#include "rt_device.h"

namespace rt_impl __attribute__((visibility("hidden"))) {

struct LdsIn {
    int variant;
    int n_walk_nodes, n_lnode_f4;   // the links the launch walks: their nodes, their float4
    int n_sph, n_box, n_med;
    bool box_all_cmp;               // every box's record is compact
    bool perlin_packed;             // the packed Perlin table is there to stage
    int tex_w[8], tex_h[8];
    // options (rt_debug.h RT_OPTION_*)
    bool sph_lds, big_wg, tl_small_lds, tl_leaf_lds, shade_lds, leaf_prefetch;
    int lds_node_cap;
    int walk_frac;                  // the override (0: by the tree)
};

// Sets a.block, lds_node_f4, leaf_lds, perlin_lds, media_lds, sph_lds, box_cmp_lds, sph_mat_lds,
// box_mat_lds, tex_lds, tex_lds_off[], lds_end_f4, leaf_pf, and walk_frac = 32 for the two-level
// walk without an override; reads nothing of a.
void plan_lds(const LdsIn& in, rt_kernel_args& a);

struct Split {
    int per_launch;      // frames per launch (equal launches)
    int chunks_wanted;   // chunks per tile aimed at
    bool staged;         // chunked launches stage their per-frame colours
};
// free_bytes: the device's free memory plus what the staging buffer already holds
Split plan_split(int n_tiles, long long waves, int n_frames, int chunk_target, int staged_chunk_target, int stage_tiles,
                 bool moments, size_t n_pixels, size_t sample_budget, size_t free_bytes);

struct Chunks {
    int n_chunks, chunk_frames, tail_chunks;
    bool stage;   // this launch stages (false: one chunk without moments folds in place)
};
// One launch of nf frames; tail: the one-frame chunks a staged launch of the pooled kernels ends with.
Chunks plan_chunks(int nf, int chunks_wanted, bool staged, bool moments, int tail, bool pooled);

}  // namespace rt_impl
