// rt_plan.h — launch planning of rt_render as pure functions (rt_plan.cpp): the LDS layout of the
// link-format shapes, the frames per launch and the split of one launch into chunks.  Host-only
// and context-free: every input is a plain value, so which inputs decide a layout can be read
// off the signatures.
#pragma once

#include <cstddef>

#include "rt_device.h"

// OPT bits of the render kernel template (rt_kernel.hip render_persistent<MINW, STATS, BLOCK, OPT>)
#define RT_OPT_POOL 1   // pooled units (render_pool): without it a lane owns a pixel (variant 37)
#define RT_OPT_SM 2     // with RT_OPT_POOL and the link walk: walks and shading in batches (render_stream)
#define RT_OPT_FD 4     // with RT_OPT_SM: the scene is in the shared-reciprocal division regime (P.fastdiv)
#define RT_OPT_STREAM 8 // with RT_OPT_SM: the wave streams over units (render_stream) instead of one at a time
#define RT_OPT_TL 16    // with RT_OPT_STREAM: two-level walk (top levels in LDS, the rest of the nodes global)
#define RT_OPT_BOXC 32  // with RT_OPT_STREAM: every box has a compact record (box_test_compact), no full box test
#define RT_OPT_SPAIR 64 // with RT_OPT_STREAM: leaves of two spheres tested at once (leaf_prims_t; most leaves are)
#define RT_OPT_BOXQ 256 // with RT_OPT_FD, RT_OPT_BOXC and RT_OPT_STD: the compact box test with one reciprocal per
                        // axis and no division per face (box_test_compact_q; option box_interior), and the leaf
                        // stage's prefetched record address by selects (rt_kernel_common.h RT_WT_DISPATCH)
#define RT_OPT_MASK 512 // with RT_OPT_STREAM: the units run over the active tiles of a tile mask (P.tile_list, P.n_active;
                        // rt_kernel.hip unit_geo); without it the code is the unmasked kernel's, unchanged
#define RT_OPT_STD 128  // the default launch's configuration, compiled in (plan_kernel's std_cfg takes these
                        // kernels when it holds): staged chunks with sparse staging (P.samples, P.sflags), every
                        // medium bounded by a sphere (P.media_sph; no out-of-line boundary call), the leaf and
                        // shading tables in LDS (spheres, media, box records, sphere materials, texture
                        // descriptors) and with RT_OPT_BOXC the compact boxes' materials and the leaf record
                        // prefetch (P.leaf_pf: the leaf stage holds only the prefetched forms).  Fewer wave-uniform
                        // flags live through the rounds: the C3 kernel 128 -> 117 VGPRs, SGPR spills 34 -> 0
// every release kernel streams pooled samples in batches
#define RT_OPT_SM_STREAM (RT_OPT_POOL | RT_OPT_SM | RT_OPT_STREAM)

// The instantiated render kernels, X(BLOCK, OPT): the link shape with everything in LDS as 2 x 512
// or 1 x 1024 threads per CU, and the two-level walk (1024 only; no RT_OPT_SPAIR, and no RT_OPT_BOXQ:
// SGPR spills), each over {plain, shared-reciprocal division} x {full, compact boxes} with the
// RT_OPT_STD forms of the division kernels.  Every entry also has its twin for a launch under a tile
// mask (OPT | RT_OPT_MASK), and in the A/B library its stats twin (STATS, OPT without RT_OPT_BOXQ).
// rt_kernel.hip instantiates and dispatches from this list; plan_kernel chooses only from it
// (tests/test_launch_plan.py: some input of plan_kernel chooses each entry, and nothing else is chosen).
// rt_render reaches all but four: the two-level kernels with RT_OPT_STD and their mask twins, since
// plan_lds stages no shading table for a two-level walk and std_cfg needs tex_lds
// (tests/test_kernel_matrix.py; tests/test_gpu_kernel_matrix.py launches the other 52).
#define RT_RENDER_KERNELS_LDS(X, BLOCK)                                                          \
    X(BLOCK, RT_OPT_SM_STREAM)                                                                   \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_BOXC)                                                     \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_SPAIR)                                                    \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD)                                                       \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_STD)                                          \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_SPAIR)                                        \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_SPAIR | RT_OPT_STD)                           \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_BOXC)                                         \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_BOXC | RT_OPT_SPAIR)                          \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_BOXC | RT_OPT_STD)                            \
    X(BLOCK, RT_OPT_SM_STREAM | RT_OPT_FD | RT_OPT_BOXC | RT_OPT_STD | RT_OPT_BOXQ)
#define RT_RENDER_KERNELS(X)                                                                     \
    RT_RENDER_KERNELS_LDS(X, 512)                                                                \
    RT_RENDER_KERNELS_LDS(X, 1024)                                                               \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL)                                                        \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL | RT_OPT_BOXC)                                          \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL | RT_OPT_FD)                                            \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL | RT_OPT_FD | RT_OPT_STD)                               \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL | RT_OPT_FD | RT_OPT_BOXC)                              \
    X(1024, RT_OPT_SM_STREAM | RT_OPT_TL | RT_OPT_FD | RT_OPT_BOXC | RT_OPT_STD)

namespace rt_impl __attribute__((visibility("hidden"))) {

// the pooled kernel structure (the default and its stats twin): the only one the SAH tree, tile masks,
// the collapse, rebuild and box pre-test nodes, sparse staging and the per-wave slots run on
inline bool pooled_variant(int variant) { return variant == 0 || variant == 39; }
// 8x8 tiles of `rows` rows of an image
inline int tile_count(int width, int rows) { return ((width + 7) / 8) * ((rows + 7) / 8); }

// The LDS tables of rt_kernel_args: their float4 offsets in the dynamic LDS, -1 = not staged (the shared
// device functions then take their global-memory forms).  A table added to rt_kernel_args is listed here.
constexpr int rt_kernel_args::* LDS_TABLES[] = {
    &rt_kernel_args::perlin_lds,  &rt_kernel_args::media_lds,   &rt_kernel_args::sph_lds, &rt_kernel_args::box_cmp_lds,
    &rt_kernel_args::sph_mat_lds, &rt_kernel_args::box_mat_lds, &rt_kernel_args::tex_lds};
// No table staged.  LDS_LEAF: nor the leaf records (leaf_lds); LDS_TEXELS: nor any slot's texels (tex_lds_off[]).
enum { LDS_LEAF = 1, LDS_TEXELS = 2, LDS_ALL = LDS_LEAF | LDS_TEXELS };
inline void clear_lds_tables(rt_kernel_args& a, int also) {
    for (int rt_kernel_args::* t : LDS_TABLES) a.*t = -1;
    if (also & LDS_LEAF) a.leaf_lds = -1;
    if (also & LDS_TEXELS)
        for (int& o : a.tex_lds_off) o = -1;
}

struct KernelId {
    int block, opt;
};
// the release library's instantiations, mask twins included
constexpr KernelId RENDER_KERNELS[] = {
#define RT_X(BLOCK, OPT) {BLOCK, OPT}, {BLOCK, (OPT) | RT_OPT_MASK},
    RT_RENDER_KERNELS(RT_X)
#undef RT_X
};
constexpr int N_RENDER_KERNELS = (int)(sizeof(RENDER_KERNELS) / sizeof(RENDER_KERNELS[0]));

// What one render launch runs (plan_kernel).
struct KernelPlan {
    bool ok;          // false: the launch is refused before anything is launched (nothing below is set)
    int shape;        // RT_SHAPE_* (rt_device.h)
    bool stats;       // the region-timer stats twin (A/B library)
    bool pool;        // pooled samples (false: one pixel per lane, A/B library)
    int block;        // workgroup size
    int opt;          // the instantiation's OPT: a RENDER_KERNELS entry for the pooled link shapes (the
                      // stats twins: without RT_OPT_BOXQ), 0 for the A/B library's other structures
    size_t lds;       // dynamic LDS bytes
    int info[RT_LI_N];   // rt_debug_last_launch's fields; those rt_render fills itself stay 0
};
// The launch decision of rt_launch_render: which kernel, with how much LDS, and what the launch
// reports.  ab: the A/B library (its structures by a.variant; the release library ignores a.variant).
// Reads of a: variant, block (512 or 1024, plan_lds), n_active, n_nodes, n_lnode_f4, lds_node_f4,
// lds_end_f4, n_f2inner, n_f2leaves, fastdiv, box_all_cmp, box_interior, sph_pairs, leaf_pf, media_sph,
// n_media, n_sph_lds, n_box_lds, the table offsets (perlin_lds, media_lds, sph_lds, box_cmp_lds,
// sph_mat_lds, box_mat_lds, tex_lds), box_margin, n_chunks, spine_len, walk_frac, and whether
// samples, sflags, wbuf and tile_list are null.
// Writes to a: the table offsets = -1 for the A/B shapes that stage none of them (both near-first
// shapes, global meta-word nodes), whether or not the launch is then refused; and, unless refused,
// leaf_pf (cleared when a table the prefetch reads is not staged) and acc_lds.
KernelPlan plan_kernel(rt_kernel_args& a, bool ab);

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
