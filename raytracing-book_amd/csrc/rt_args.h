// rt_args.h — the host's copy of a scene with its options (SceneState), and the way from it to the
// render kernel's arguments (rt_args.cpp): validation, the walk's trees, the host halves of the
// uploads, the scene's half of rt_kernel_args, the per-launch split and the frame counts.  Plain
// C++ like rt_prep.h and rt_plan.h: no HIP runtime call, no device, no rt_ctx (the HIP headers only
// give float4 and friends).  rt_ctx (rt_ctx.h) derives from SceneState and adds the devices;
// rt_debug_plan_scene (rt_debug_host.cpp) runs the same functions on a SceneState of its own.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rt/rt.h"
#include "rt/rt_debug.h"
#include "rt/rt_types.h"
#include "rt_device.h"
#include "rt_plan.h"
#include "rt_prep.h"

namespace rt_impl __attribute__((visibility("hidden"))) {

// Who writes which group: the uploads (prep_buffer, set_texture, set_camera) write group 1 and reset
// group 3's keys; the rt.h setters (params, size, partition, BVH mode, moments, tile mask) write
// group 2; validate() and refresh_walk() alone write group 3; set_option() alone writes group 4
// (rt_create's environment knobs of the A/B library too); rt_render commits group 5 from
// step_frame_counts (the setters that invalidate an image reset it).
struct SceneState {
    // ---- 1. the scene as uploaded, and what the uploads derive from single bindings
    std::vector<uint8_t> host_buf[6];
    bool uploaded[6] = {false, false, false, false, false, false};
    int tex_format[8] = {0}, tex_w[8] = {0}, tex_h[8] = {0};
    rt_camera_ubo cam{};
    bool have_cam = false;
    int n_dnodes = 0;
    std::vector<rt_dnode> dnodes;   // host copy of the threaded BVH (fast-walk tables are built from it)
    bool spec_ok = false;   // every child box lies inside its parent's (the near-first walk needs it)
    std::vector<float4> boxc_host;  // the compact box records (host copy of Device::dboxc)
    bool boxes_canon = false;   // every box has Box.java's axis-aligned face layout (dboxes[18..20])
    bool fd_ok[6] = {true, true, true, true, true, true};   // per binding: records in the fast-division regime
    bool fd_cam = true;
    bool boxes_cond = false;   // every box face's 2-D Cramer system is well conditioned (box pre-test)
    int n_boxc_ok = 0;           // boxes whose compact record reproduces their faces
    int perlin_pk_slot = -1;     // texture slot whose Perlin table has its packed copy (Device::perlin_pk)
    // the collapse plan from measured node hits (rt_debug_set_collapse_hits): per node of the walk's
    // tree in its breadth-first link order, the box tests that hit, and the walks begun at the root
    std::vector<int64_t> inj_hits;
    int64_t inj_walks = 0;
    // ---- 2. what the rt.h setters hold
    int max_depth = 5;
    float background[3] = {0, 0, 0};
    float sqrt_spp = 1.0f, recip_sqrt_spp = 1.0f;
    int width = 0, height = 0;
    int proc_rank = 0, proc_world = 1, stripe_rows = 16;
    // the BVH the link walk runs on (rt_set_bvh_mode): the uploaded one (RT_BVH_REFERENCE), or the
    // binned-SAH tree built from its prims at validation (RT_BVH_SAH, non-parity fast mode, bvh_sah.h)
    int bvh_mode = RT_BVH_REFERENCE;
    // Sample moments (rt_set_moments; single-device contexts): every launch is staged and folded by
    // the fold with the moments.
    bool moments = false;
    // rt_set_active_tiles: the mask in effect (mask_set), its tiles' indices in ascending order
    // (Device::tile_list holds the same on the device)
    bool mask_set = false;
    std::vector<int32_t> act_list;
    // ---- 3. derived by validate() and refresh_walk(), with the keys they were derived for
    bool validated = false;
    bool uv_always = false;
    FastTables fast;
    int n_link_nodes = 0;
    std::vector<float4> links;   // build_links(dnodes), empty when unavailable
    std::vector<uint8_t> sah_bvh;   // the SAH tree in the reference's node format (rt_debug_walk_bvh)
    std::vector<rt_dnode> walk_dn;  // threaded nodes of the BVH the link walk uses (reference or SAH)
    int fast_gen = 0;               // counts the changes of `fast` and walk_links (Device::fast_gen: re-upload)
    float scene_extent = -1.0f;   // max |coordinate| over records and camera (< 0: not computed)
    // the links the launch walks: links, or (option box_vnodes) the same with every all-box leaf's
    // box pre-tests as nodes of the walk (build_links with vbox); rebuilt when the margin changes
    std::vector<float4> walk_links;
    int n_walk_nodes = 0;
    bool walk_v = false;
    float walk_v_margin = -1.0f;
    bool walk_stale = true;
    bool walk_r = false;            // walk_links were built on the rebuilt inner nodes
    int walk_rmode = 0;             // ... of this mode
    std::vector<rt_dnode> rb_dn;    // rebuild_inner(walk_dn, rb_mode), kept across camera moves
    int rb_mode = -1;               // -1: not built for the current walk_dn
    bool walk_c = false;            // walk_links were built with a collapse plan ...
    rt_camera_ubo walk_cam{};       // ... for this camera and image size
    int walk_w = 0, walk_h = 0;
    int n_dropped = 0;              // inner nodes the walk leaves out
    int n_rebuilt = 0;              // nodes of the rebuilt tree (0: the tree as uploaded / built)
    int n_vnodes = 0;               // box pre-test nodes in walk_links
    int pair_leaves = -1;        // per mille of the link-format leaves that hold two spheres (< 0: not counted)
    // ---- 4. options (rt_debug.h RT_OPTION_*; set_option)
    bool box_vnodes = true;         // option box_vnodes
    bool box_interior = true;       // option box_interior
    bool zero_dir_end = true;       // option zero_dir_end (rt_kernel.hip render_stream)
    bool first_leaf = true;         // option first_leaf: a walk that starts at the spine's leaf tests it where
                                    // it begins (rt_kernel.hip render_stream; the RT_OPT_BOXQ kernels)
    bool collapse = true;           // option collapse: the walk leaves out inner nodes (plan_collapse)
    int rebuild = 2;                // option rebuild: the walk's inner nodes rebuilt over its leaves (rebuild_inner mode)
    int debug_flags = 0;    // env RT_DEBUG_FLAGS: ablation runs only (bit 0: Perlin -> 0.5; bit 3: compact boxes hit on their planes alone)
    int variant = 0;   // kernel structure variant (env RT_KERNEL_VARIANT; A/B only)
    // Work split: aim for chunk_target work units per resident wave (env
    // RT_CHUNK_TARGET; 0 = one chunk per tile), staged_chunk_target when staged
    // (RT_STAGED_CHUNK_TARGET).  With at least stage_tiles tiles
    // per resident wave (env RT_STAGE_TILES) the chunks are ordered (the running
    // mean is handed from wave to wave, rt_kernel.hip wait_chunk); with fewer, a
    // tile's frames would be one long serial chain, so the chunks run in parallel,
    // stage their per-frame colours (at most sample_budget bytes) and the fold (rt_moments.hip)
    // applies the running mean in frame order.  The default stage_tiles stages
    // every chunked launch: with render_stream that measured fastest at N = 1 too
    // (scene 8 -5% against ordered chunks).
    int chunk_target = 16;          // ordered chunks (RT_CHUNK_TARGET)
    int staged_chunk_target = 48;   // staged chunks (RT_STAGED_CHUNK_TARGET)
    int tail_chunks = -1;           // option tail_chunks: staged launches end with this many one-frame chunks
                                    // (-1: tail_chunks_for the tree)
    int stage_tiles = 1 << 20;      // in effect always staged (the measured best with render_stream)
    bool fastdiv = true;   // shared-reciprocal divisions where exact (env RT_FASTDIV=0 disables; A/B)
    bool box_pretest = true;   // the canonical box tests' bounds pre-test (env RT_BOX_PRETEST=0 disables; A/B)
    int sm_batch = 64;   // render_stream's shading batch (env RT_SM_BATCH) ...
    int sm_frac = 0;     // ... or fraction of the lanes with a walk, in 64ths (env RT_SM_FRAC); 0 = by kernel:
                         // 50 for the compact-box kernels (scene 8 1080p -1.1%, 4K -1.6% against 56), 56 else
                         // (scene 6 +1.4% at 52; profiles/r03_sm_frac_knobs.log)
    bool shade_lds = true;       // shading tables in LDS (sphere / box materials, small textures; option):
                                 // scenes 8 / 0 / 6 -0.3 / -1.0 / -1.2% (profiles/r04_shade_lds_ab_s*.log)
    bool tl_small_lds = true;    // two-level walk: small sphere / box tables staged beside the top levels (option)
    bool leaf_prefetch = true;   // leaf records prefetched before the type blocks when all are in LDS (option)
    int walk_frac = 0;   // render_stream: node walks stop at this fraction of lanes ready, in 64ths (env RT_WALK_FRAC);
                         // 0 = by BVH size: 8 up to 64 nodes, 32 up to 1024, 48 above (walk_frac_for)
    bool big_wg = true;    // 1024-thread workgroups with sphere + box records in LDS when they fit (env RT_BIG_WG=0: A/B)
    bool sph_lds = true;   // sphere records' first two float4 in LDS when they fit (env RT_SPH_LDS=0 disables; A/B)
    bool compact_boxes = true;   // boxes' compact records when every box has one (box_test_compact; option 0: A/B)
    bool spine = true;           // walks start past the spine when they hit it for sure (plan_spine)
    int lds_node_cap = 0;        // bytes of BVH nodes staged in LDS, 0 = as many as fit (tests: force the two-level walk)
    bool tl_leaf_lds = true;     // two-level walk: the leaf records in LDS beside the top levels (when they fit)
    bool sparse_stage = true;    // staged chunks store only the colours that are not exactly zero (option)
    int sphere_pairs = 1;        // the sphere-pair kernels when most leaves hold two spheres (option; 2: always,
                                 // compact-box kernels included)
    bool perlin_pk = true;       // stage the packed Perlin table (option; else the texture as uploaded)
    unsigned long long watchdog_ticks = 120ull * 100000000ull;     // render_stream progress bound (100 MHz ticks)
    unsigned long long chunk_wait_ticks = 30ull * 100000000ull;    // ordered-chunk wait bound
    size_t sample_budget = (size_t)32 << 30;   // staged colours per launch, at most (and at most half the free memory)
    // ---- 5. frame counts (step_frame_counts).  moments_frames = the frames 1 .. n the image (and with
    // the moments on Device::m2) holds, 0 = invalid (nothing rendered yet, a first_frame gap, the image
    // overwritten or resized).
    int moments_frames = 0;
    // Per-tile frame counts (rt_read_tile_frames): the frames 1 .. n each 8x8 tile of the first device's
    // image holds, 0 = invalid.  While every tile holds the same count tile_frames is empty and
    // moments_frames is that count; once they differ (a launch under a tile mask) tile_frames holds
    // one count per tile and moments_frames their minimum, so "valid" stays moments_frames >= 1.
    // Single-device contexts keep them whether or not the moments are on.
    std::vector<int32_t> tile_frames;

    size_t n_records(int binding) const;   // records of an uploaded binding (the lights: words)
};

// ---- one spelling each
// (pooled_variant and tile_count: rt_plan.h)
// every box has a compact record and the option is on: the compact-box kernels
bool all_boxes_compact(const SceneState& s);

// ---- options: rt_debug_set_option / rt_debug_get_option (ab: the A/B library's options >= 100 exist).
// RT_OK, or RT_ERR_INVALID_ARG with its text in *err.
int set_option(SceneState& s, int option, int v, bool ab, std::string* err);
int get_option(const SceneState& s, int option, int* v, bool ab, std::string* err);

// ---- the host halves of the uploads (errors: code returned, text in *err, may be NULL)
// What rt_upload_buffer copies to each device: src / n the binding's own buffer (the threaded nodes
// for the BVH, the ids without the count word for the lights, else the bytes as given), and the
// derived records of quads (faces) and boxes (faces, boxc).
struct BufferPrep {
    const void* src = nullptr;
    size_t n = 0;
    std::vector<uint8_t> threaded;   // RT_BIND_BVH: what src points to
    std::vector<float4> faces;       // Device::dquads / dboxes
    std::vector<float4> boxc;        // Device::dboxc
};
// Checks binding, size and record count, threads an incoming BVH, and only then changes s: a rejected
// upload leaves the previous one (host copy, threaded nodes, flags) intact.  Writes host_buf, uploaded,
// the binding's derived flags of group 1, clears inj_* with a new BVH, validated and scene_extent.
int prep_buffer(SceneState& s, int binding, const void* bytes, size_t nbytes, BufferPrep& out, std::string* err);
// What rt_upload_texture copies: src / bytes the texels (RGB8 expanded to RGBA8 in rgba), pk the packed
// Perlin table when the texture qualifies (perlin_pack), else empty.  Changes nothing of s;
// set_texture records the slot once the copies are made.
struct TexturePrep {
    const void* src = nullptr;
    size_t bytes = 0;
    std::vector<uint32_t> rgba;
    std::vector<float4> pk;
};
int prep_texture(int slot, int format, int w, int h, const void* texels, TexturePrep& out, std::string* err);
void set_texture(SceneState& s, int slot, int format, int w, int h, bool packed);
void set_camera(SceneState& s, const float ubo[28]);   // cam, have_cam, fd_cam; resets scene_extent (SAH: validated)

// ---- validation and the walk's trees
// The fast mode's tree (bvh_sah.h) over the uploaded BVH's prims; child order: the one nearer the camera first.
int build_sah(const SceneState& s, std::vector<rt_bvh_node>& out, std::string* err);
// Checks the uploaded records against each other and derives group 3 up to walk_dn (no-op while validated).
int validate(SceneState& s, std::string* err);
// the links the launch walks: with the box pre-test nodes (option box_vnodes) when every box has a
// compact record and the pre-test is on (its margin is the nodes' growth: rebuilt when it changes)
void refresh_walk(SceneState& s, float box_margin);

// ---- the scene's half of the kernel arguments
// Zeroes a and fills every field that depends on neither a device nor the launch's frame range.
// Reads of s: a validated scene (validate() first) -- host_buf, the texture sizes and formats, cam,
// group 2 but the moments and the mask, `fast`, every option -- and group 1's flags.
// Writes to s: scene_extent and pair_leaves where not yet computed, and through refresh_walk() the
// walk's links and their keys (fast_gen counts a change).
// Writes to a: watchdog / chunk_wait ticks, lights_count, uv_always, boxes_canon, box_margin, fastdiv,
// variant, zero_dir_end, sm_batch, sm_frac, walk_frac, the near-first tables' scalars (fast_ok .. fl_rank),
// debug_flags, box_interior, box_vnodes, n_nodes, n_lnode_f4, the spine (plan_spine), first_leaf,
// n_media, media_sph, n_sph_lds, n_box_lds, box_all_cmp, sph_pairs, the texture descriptors' sizes and
// formats, perlin_slot, perlin_packed, what
// plan_lds sets (rt_plan.h), cam, background, max_depth, the spp factors, width, height, stripe_rows.
// Left zero: every pointer, local_rows / rank / world and the census
// (bind_device), and what plan_device and plan_launch set.
// RT_ERR_STATE (text in *err) when the SAH tree is asked of another kernel structure.
int scene_args(SceneState& s, rt_kernel_args& a, std::string* err);

// ---- per device and per launch, as numbers
// A device's share of one rt_render call: sets a.n_pixels and a.n_active (the mask's tiles, else the
// stripe's) and returns the frames per launch and the unit split (plan_split).  waves: the resident
// waves; free_bytes: the device's free memory plus what its staging buffer holds.
Split plan_device(const SceneState& s, int local_rows, long long waves, size_t free_bytes, bool mom, int n_frames,
                  rt_kernel_args& a);
// One launch of the call: frames [f0, f0 + split.per_launch) of n_frames.  Sets a.first_frame, n_frames,
// n_chunks, chunk_frames, tail_chunks and wbuf_waves; says which buffers the launch needs (the caller
// allocates them and sets a.samples, a.sflags, a.wbuf -- or leaves them NULL).
struct LaunchPlan {
    bool stage;             // staged colours: launch_frames x n_pixels float4
    bool sparse;            // ... with a flag byte per sample
    bool wave_slots;        // pooled units without staging: 2 x 64 x chunk_frames float4 per resident wave
    size_t launch_frames;   // frames the staging buffers are sized for
};
LaunchPlan plan_launch(const SceneState& s, const Split& split, bool mom, long long waves, int first_frame, int n_frames,
                       int f0, rt_kernel_args& a);
// rt_debug_last_launch's fields that belong to the scene (RT_LI_BVH_MODE .. RT_LI_REBUILT), and
// rt_debug_first_leaf's words; info[RT_LI_BOXQ] must hold the launched kernel's (plan_kernel).
void launch_report(const SceneState& s, const rt_kernel_args& a, int* info, int first_leaf_last[4]);

// ---- frame counts
// The rule of group 5 for one rt_render call that samples frames first_frame .. first_frame + n_frames - 1
// (n_frames > 0) of n_tiles tiles, or with mask != NULL only of the tiles it lists: a tile sampled from
// frame 1 restarts, from its count + 1 extends, anything else leaves it invalid (0); the other tiles
// keep theirs.  before_all / before_tiles and the result are the two forms of SceneState's counts
// (tiles empty: uniform).
struct FrameCounts {
    int all = 0;
    std::vector<int32_t> tiles;
};
FrameCounts step_frame_counts(int before_all, const std::vector<int32_t>& before_tiles, int n_tiles,
                              const std::vector<int32_t>* mask, int first_frame, int n_frames);

}  // namespace rt_impl
