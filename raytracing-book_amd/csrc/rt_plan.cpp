// rt_plan.cpp — launch planning (rt_plan.h): pure functions of plain values.
#include "rt_plan.h"

#include <algorithm>

namespace rt_impl __attribute__((visibility("hidden"))) {

// LDS plan of the link-format shapes (rt_kernel.hip rt_launch_render): from address 0 the
// nodes, then the leaf records, the Perlin table (6 x 256 R32F), the media records with
// their sphere boundaries, the spheres' intersection halves (A, B) and the canonical
// boxes' compact records -- each when it fits.  512-thread workgroups (2 per CU,
// RT_LDS_DYN_BYTES each) when everything fits them, else one of 1024 threads per CU
// (RT_LDS_BIG_BYTES); when not even the nodes and leaves fit that, the two-level walk:
// the top levels (breadth-first prefix) in LDS, the rest of the nodes and the leaf
// records in global memory.  The A/B structures 37 (one pixel per lane: 512 threads,
// the lanes' running means after what is staged) and 61 (its own tree) plan below too.
void plan_lds(const LdsIn& in, rt_kernel_args& a) {
    const bool fast_walk = in.variant == 61 || in.variant == 69;
    const bool pooled = pooled_variant(in.variant);
    const int n_sph = in.n_sph, n_box = in.n_box, n_med = in.n_med;
    const size_t node_f4 = 2 * (size_t)in.n_walk_nodes;
    const size_t leaf_f4 = (size_t)in.n_lnode_f4 > node_f4 ? (size_t)in.n_lnode_f4 - node_f4 : 0;
    // the Perlin table is staged in its packed form only (else its noise reads the texture)
    const size_t perlin_f4 = in.perlin_packed ? 256 : 0;
    const size_t media_f4 = (n_med > 0 && n_med <= 64) ? 3 * (size_t)n_med : 0;
    const size_t sph_f4 = (in.sph_lds && pooled) ? 2 * (size_t)n_sph : 0;
    const size_t box_f4 = (size_t)RT_BOXC_F4 * n_box;   // every box's record (bounds; compact faces)
    const bool stats_twin = in.variant == 39;   // static LDS counters beside the dynamic region
    const size_t cap_s = RT_LDS_DYN_BYTES / 16,
                 cap_b = (stats_twin ? RT_LDS_BIG_STATS_BYTES : RT_LDS_BIG_BYTES) / 16;
    const size_t ess = node_f4 + leaf_f4 + perlin_f4 + media_f4;   // what every walk and shade reads
    const size_t all = ess + sph_f4 + box_f4;
    const size_t node_cap = in.lds_node_cap > 0 ? (size_t)in.lds_node_cap / 32 * 2 : node_f4;
    const bool big_ok = in.big_wg && pooled;
    // A/B: threaded meta-word nodes (variant 30, or 37 when the link nodes do not fit 512 threads)
    const bool meta = !fast_walk && !pooled && (in.variant == 30 || in.variant == 31 || ess > cap_s);
    size_t cap;
    bool tl = false;
    if (fast_walk) {
        cap = 0;   // variant 61 stages its own tree (rt_launch_render)
    } else if (meta) {
        cap = cap_s;
    } else if (node_cap < node_f4 && pooled) {
        tl = true;
        cap = cap_b;
    } else if (all <= cap_s || (ess <= cap_s && !(big_ok && all <= cap_b))) {
        cap = cap_s;
    } else if (big_ok && ess <= cap_b) {
        cap = cap_b;
    } else {
        tl = pooled;
        cap = tl ? cap_b : cap_s;
    }
    a.block = cap == cap_b ? 1024 : 512;
    // the two-level walk's rounds: 32 (its walks wait on global nodes; 16 / 24 / 32 / 48 / 64 on
    // the 4000-sphere cloud at a 32 KB cap and the 9000-sphere cloud: 32 best, -1.7% against 48,
    // profiles/r04_bvh_walk_frac_*.log)
    if (tl && !in.walk_frac) a.walk_frac = 32;
    size_t at = 0;
    a.lds_node_f4 = 0;
    clear_lds_tables(a, LDS_ALL);
    if (meta) {
        at = node_f4;   // the threaded nodes (32 B each) from address 0 (rt_launch_render: META_LDS)
    } else if (!fast_walk && in.n_lnode_f4 > 0) {
        if (tl) {
            // the top levels, then the leaf records (8 B per leaf, read on every leaf visit) when
            // they take at most half of the room, then the small tables the shading reads; room
            // is reserved for the sphere / compact box records that take at most 1/16 of it (a
            // few nodes' worth), and each table is staged below whenever it still fits (option
            // tl_small_lds; a larger table can fit after a node cap -- tests/test_gpu_adversarial.py
            // forces both layouts)
            const size_t room0 = cap - perlin_f4 - media_f4;
            const size_t rsv = (in.tl_small_lds && sph_f4 && 16 * sph_f4 <= room0 ? sph_f4 : 0) +
                               (in.tl_small_lds && box_f4 && 16 * box_f4 <= room0 ? box_f4 : 0);
            const size_t room = room0 - rsv;
            const size_t lf_f4 = (in.tl_leaf_lds && 2 * leaf_f4 <= room) ? leaf_f4 : 0;
            a.lds_node_f4 = (int)(std::min(std::min(node_f4, node_cap), room - lf_f4) & ~(size_t)1);
            at = (size_t)a.lds_node_f4;
            if (lf_f4) {
                a.leaf_lds = (int)at;
                at += lf_f4;
            }
        } else {
            a.lds_node_f4 = (int)node_f4;
            a.leaf_lds = (int)node_f4;
            at = node_f4 + leaf_f4;
        }
    }
    if (!fast_walk) {
        if (perlin_f4 && at + perlin_f4 <= cap) { a.perlin_lds = (int)at; at += perlin_f4; }
        if (media_f4 && at + media_f4 <= cap) { a.media_lds = (int)at; at += media_f4; }
        if (!tl || in.tl_small_lds) {
            if (sph_f4 && at + sph_f4 <= cap) { a.sph_lds = (int)at; at += sph_f4; }
            if (box_f4 && at + box_f4 <= cap) { a.box_cmp_lds = (int)at; at += box_f4; }
        }
        // the shading tables (option shade_lds): every sphere's third float4, every compact
        // box's (emission, material), the texture slots' descriptors and the texels of the
        // small slots (at most 1024 words: the solid and checker colour tables), each when
        // it fits -- so a hit's material, texture and colour need no global read
        if (in.shade_lds && pooled && !tl) {
            if (a.sph_lds >= 0 && at + (size_t)n_sph <= cap) { a.sph_mat_lds = (int)at; at += (size_t)n_sph; }
            if (a.box_cmp_lds >= 0 && in.box_all_cmp && at + (size_t)n_box <= cap) {
                a.box_mat_lds = (int)at;
                at += (size_t)n_box;
            }
            size_t need = 8;
            for (int t = 0; t < 8; t++) {
                const size_t words = (size_t)in.tex_w[t] * (size_t)in.tex_h[t];
                if (in.tex_w[t] > 0 && in.tex_h[t] > 0 && words <= 1024) need += (words + 3) / 4;
            }
            if (at + need <= cap) {
                a.tex_lds = (int)at;
                size_t off = at + 8;
                for (int t = 0; t < 8; t++) {
                    const size_t words = (size_t)in.tex_w[t] * (size_t)in.tex_h[t];
                    a.tex_lds_off[t] = -1;
                    if (in.tex_w[t] > 0 && in.tex_h[t] > 0 && words <= 1024) {
                        a.tex_lds_off[t] = (int)off;
                        off += (words + 3) / 4;
                    }
                }
                at = off;
            }
        }
    }
    a.lds_end_f4 = (int)at;
    // the leaf stage's record prefetch reads 3 float4 at any of these tables' offsets: every
    // table it can index is staged (and a sphere's 3rd float4 stays inside the staged region)
    a.leaf_pf = (in.leaf_prefetch && a.sph_lds >= 0 && a.box_cmp_lds >= 0 &&
                 (n_med == 0 || a.media_lds >= 0) && a.box_cmp_lds > a.sph_lds) ? 1 : 0;
}

// The release library has one kernel structure (tests/test_gpu_*.py pin it to the oracle):
// pooled samples streamed over units with walks and shading in batches (render_stream) over
// link-format nodes staged in LDS with the Perlin table, media, sphere and box records the
// host placed after them (a.lds_end_f4), 4 waves per SIMD, as 2 x 512 or 1 x 1024 threads
// per CU (a.block); when the nodes do not fit (a.lds_node_f4 < 2 n_nodes) the two-level
// walk reads the nodes below the staged top levels from global memory (1024 threads).
// Each in a shared-reciprocal division form (a.fastdiv) and the plain one.
// The A/B library adds the other structures, all bit-identical (RT_OPTION_KERNEL_VARIANT):
// 37 the link walk with one pixel per lane (the round-1 default), 30 threaded meta-word nodes
// (LDS when they fit, else global), 61 the exact near-first stack walk, and the region-timer
// stats twins 39 / 38 / 31 / 69.
KernelPlan plan_kernel(rt_kernel_args& a, bool ab) {
    KernelPlan k = {};
    if (a.n_active <= 0) return k;   // the units divide by it (unit_geo); the caller skips an empty mask
    int shape = RT_SHAPE_LINK_LDS;
    size_t staged = (size_t)a.lds_end_f4 * 16;
    bool stats = false, pool = true;
    const bool tl = a.n_lnode_f4 > 0 && a.lds_node_f4 < 2 * a.n_nodes;
    if (tl) shape = RT_SHAPE_LINK_TL;
    if (ab) {
        stats = a.variant == 38 || a.variant == 31 || a.variant == 69 || a.variant == 39;
        pool = pooled_variant(a.variant);
        if (a.variant == 61 || a.variant == 69) {
            const size_t stack_b = (size_t)RT_FAST_STACK * 512 * sizeof(short);
            const size_t tree_b = (size_t)a.n_f2inner * 64 + (size_t)((a.n_f2leaves + 1) / 2) * 16;
            shape = tree_b + stack_b <= RT_LDS_DYN_BYTES ? RT_SHAPE_FAST_LDS : RT_SHAPE_FAST_GLOBAL;
            staged = shape == RT_SHAPE_FAST_LDS ? tree_b + stack_b : stack_b;
        } else if (a.variant == 30 || a.variant == 31 || (!pool && tl)) {
            // threaded meta-word nodes, then what the host placed after the link-format nodes
            const size_t lds_t = (size_t)a.n_nodes * sizeof(rt_dnode);
            staged = std::max(lds_t, staged);
            shape = (lds_t <= RT_LDS_NODE_BYTES && staged <= RT_LDS_DYN_BYTES) ? RT_SHAPE_META_LDS : RT_SHAPE_META_GLOBAL;
        }
        if (shape == RT_SHAPE_FAST_LDS || shape == RT_SHAPE_FAST_GLOBAL || shape == RT_SHAPE_META_GLOBAL) {
            if (shape == RT_SHAPE_META_GLOBAL) staged = 0;   // nothing else staged
            clear_lds_tables(a, 0);   // (leaf_lds and tex_lds_off[] stay: nothing of these shapes reads them)
        }
    }
    const bool link = shape == RT_SHAPE_LINK_LDS || shape == RT_SHAPE_LINK_TL;
    if (link && staged > (a.block == 1024 ? RT_LDS_BIG_BYTES : RT_LDS_DYN_BYTES)) return k;
    if (shape == RT_SHAPE_LINK_TL && (a.block != 1024 || !pool)) return k;
    if (pool && !a.samples && !a.wbuf) return k;   // pooled ordered / one-chunk units need the per-wave slots
    // the leaf record prefetch reads only tables that are staged (the A/B shapes above may drop them)
    a.leaf_pf = (a.leaf_pf && a.box_all_cmp && a.sph_lds >= 0 && a.box_cmp_lds > a.sph_lds &&
                 (a.n_media == 0 || a.media_lds >= 0)) ? 1 : 0;
    // the one-pixel-per-lane kernels (A/B) keep the lanes' running means in LDS after what is staged
    a.acc_lds = (int)(staged / 16);
    k.ok = true;
    k.shape = shape;
    k.stats = stats;
    k.pool = pool;
    k.lds = staged + (pool ? 0 : RT_LDS_ACC_BYTES);
    k.block = 512;   // the A/B library's other structures: one instantiation per shape, OPT 0
    const bool stream = pool && link;   // a RENDER_KERNELS entry
    if (stream) {
        // the default launch's configuration (RT_OPT_STD) holds: the kernels with it compiled in
        const bool std_cfg = a.samples && a.sflags && a.media_sph &&
                             (a.n_sph_lds == 0 || (a.sph_lds >= 0 && a.sph_mat_lds >= 0)) &&
                             (a.n_media == 0 || a.media_lds >= 0) && (a.n_box_lds == 0 || a.box_cmp_lds >= 0) &&
                             (!a.box_all_cmp || (a.leaf_pf && a.box_mat_lds >= 0)) && a.tex_lds >= 0;
        const bool fd = a.fastdiv != 0, boxc = a.box_all_cmp != 0;
        // a scene whose leaves are mostly sphere pairs (a.sph_pairs): without compact boxes, or
        // (2: always) with them in the division regime; not the two-level kernels
        const bool spair = shape == RT_SHAPE_LINK_LDS && ((a.sph_pairs && !boxc) || (a.sph_pairs == 2 && fd));
        const bool std_k = std_cfg && fd && !(spair && boxc);
        // the division-free box test: not the two-level kernel (SGPR spills), not the stats twins
        const bool boxq = std_k && boxc && a.box_interior && shape == RT_SHAPE_LINK_LDS && !stats;
        k.block = a.block == 1024 ? 1024 : 512;
        k.opt = RT_OPT_SM_STREAM | (tl ? RT_OPT_TL : 0) | (fd ? RT_OPT_FD : 0) | (boxc ? RT_OPT_BOXC : 0) |
                (spair ? RT_OPT_SPAIR : 0) | (std_k ? RT_OPT_STD : 0) | (boxq ? RT_OPT_BOXQ : 0) |
                (a.tile_list ? RT_OPT_MASK : 0);
    }
    int* info = k.info;
    info[RT_LI_SHAPE] = shape;
    info[RT_LI_BLOCK] = link ? a.block : 512;
    info[RT_LI_FASTDIV] = a.fastdiv;
    info[RT_LI_PRETEST] = a.box_margin > 0.0f;
    info[RT_LI_LDS] = (int)k.lds;
    info[RT_LI_LDS_NODES] = link ? a.lds_node_f4 / 2 : 0;
    info[RT_LI_COMPACT] = a.box_all_cmp + 2 * (a.box_cmp_lds >= 0);
    info[RT_LI_STAGED] = a.samples != nullptr;
    info[RT_LI_CHUNKS] = a.n_chunks;
    info[RT_LI_SPINE] = pool ? a.spine_len : 0;
    info[RT_LI_SPARSE] = a.samples && a.sflags ? 1 : 0;
    // the report and the launch part ways here: the sphere-pair kernel runs whether or not the
    // spheres are staged, and is reported only when they are (kept as it was)
    info[RT_LI_SPAIR] = (k.opt & RT_OPT_SPAIR) && a.sph_lds >= 0 ? 1 : 0;
    info[RT_LI_LEAF_PF] = stream ? a.leaf_pf : 0;
    info[RT_LI_WALK_FRAC] = a.walk_frac;
    info[RT_LI_TILES_ACTIVE] = a.n_active;
    info[RT_LI_SHADE_LDS] = (a.sph_mat_lds >= 0) + 2 * (a.box_mat_lds >= 0) + 4 * (a.tex_lds >= 0);
    info[RT_LI_BOXQ] = (k.opt & RT_OPT_BOXQ) ? 1 : 0;
    return k;
}

// Frames per launch and the unit split.  Units = tiles x chunks; with too
// few tiles per resident wave (small images, N-GPU stripes) the frames
// are split into ordered chunks so the dynamic schedule has enough units
// to balance (rt_kernel.hip wait_chunk / publish_chunk).
Split plan_split(int n_tiles, long long waves, int n_frames, int chunk_target, int staged_chunk_target, int stage_tiles,
                 bool moments, size_t n_pixels, size_t sample_budget, size_t free_bytes) {
    int per_launch = RT_MAX_FRAMES_PER_LAUNCH;
    int chunks_wanted = 1;
    const bool few_tiles = (long long)n_tiles < (long long)stage_tiles * waves;
    if (chunk_target > 0 && n_tiles > 0) {
        const long long target = few_tiles ? staged_chunk_target : chunk_target;
        chunks_wanted = (int)std::min<long long>(RT_MAX_FRAMES_PER_LAUNCH, (target * waves + n_tiles - 1) / n_tiles);
    }
    const bool staged = moments || (chunks_wanted > 1 && few_tiles);
    if (staged) {
        // staged colours per launch: at most sample_budget and half the device's free memory
        // (what this context already holds counts as free), and at most 2^31 samples (the
        // kernel's 32-bit sample index)
        const size_t budget = std::min(sample_budget, free_bytes / 2);
        const size_t per_frame = n_pixels * sizeof(float4);
        size_t frames = std::min<size_t>(RT_MAX_FRAMES_PER_LAUNCH, budget / per_frame);
        frames = std::min<size_t>(frames, ((size_t)1 << 31) / std::max<size_t>(n_pixels, 1));
        per_launch = (int)std::max<size_t>(1, frames);
    }
    {   // equal launches: no short last launch that the whole grid waits on
        const int n_launch = (std::max(n_frames, 1) + per_launch - 1) / per_launch;
        per_launch = (std::max(n_frames, 1) + n_launch - 1) / n_launch;
    }
    return {per_launch, chunks_wanted, staged};
}

Chunks plan_chunks(int nf, int chunks_wanted, bool staged, bool moments, int tail, bool pooled) {
    Chunks k;
    k.n_chunks = std::max(1, std::min(chunks_wanted, nf));
    k.chunk_frames = (nf + k.n_chunks - 1) / k.n_chunks;
    k.n_chunks = (nf + k.chunk_frames - 1) / k.chunk_frames;
    k.stage = staged && (k.n_chunks > 1 || moments);   // one chunk: the running mean in place
    // staged: the last frames as one-frame chunks (the units claimed last are then short,
    // so the grid's waves finish close together); the chunks before keep their size
    k.tail_chunks = 0;
    if (k.stage && tail > 0 && k.n_chunks > 1 && pooled) {
        const int tc = std::min(tail, nf - 1);
        const int nm = nf - tc;
        const int cm = (nm + k.chunk_frames - 1) / k.chunk_frames;
        k.n_chunks = cm + tc;
        k.tail_chunks = tc;
    }
    return k;
}

}  // namespace rt_impl
