/*
 * rt_debug.h — test/diagnostic hooks exported by librtamd.so (not part of the
 * reference's interface; used by tests/ to check device-side pieces directly).
 */
#ifndef RT_DEBUG_H
#define RT_DEBUG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Evaluate a GLSL built-in of rt_glsl.h on `device` (fn: 0 sin, 1 cos, 2 log,
 * 3 acos, 4 atan2(x, y), 5 fract, 6 sqrt). */
int rt_debug_eval_builtin(int device, int fn, const float* x, const float* y, float* out, int n);

/* Evaluate one of the render kernels' own operations on `device`, one lane per row, by the device
 * function the kernels call (csrc/rt_ops_eval.hip; tests/test_gpu_ops.py compares every form with
 * the CPU oracle bit for bit).  Rows run in whole waves in input order (a batch that is no
 * multiple of 64 is padded with copies of its last row), so the wave-wide ballots that choose a
 * division form see the 64 rows the caller put together.
 * Row i of `rows`: RT_OPS_ROW_F floats -- o[3], d[3], tmin, tmax, time, one int word, 2 unused.
 * Row i of `out`: RT_OPS_OUT_W 32-bit words (floats as their bits; unused words 0).
 * `recs`: one record per row as the scene uploads carry it; the host half prepares the device
 * records with the functions the uploads run.
 *   op                    recs per row            form                                   out words
 *   RT_OP_SPHERE          rt_sphere (48 B)        0 '/', 1 shared reciprocal (sphere_t_ab), hit, t
 *                                                 2 / 3 the same through sphere_t
 *   RT_OP_MEDIUM_SPHERE   rt_sphere               0 '/', 1 shared reciprocal (sphere_bounds)  ok, t1, t2
 *   RT_OP_QUAD            rt_quad (80 B)          0 '/', 1 shared reciprocal (quad_test)  hit, t, alpha, beta
 *   RT_OP_BOX             6 rt_quad (480 B)       0 / 1 box_test plain / fd, 2 / 3         hit, t, face, alpha, beta
 *                                                 box_test_compact plain / fd, 4 box_test_compact_q
 *   RT_OP_NODE            6 floats (xmin, xmax,   0 aabb_fast, 1 aabb_pk, 2 the exact     hit
 *                         ymin, ymax, zmin, zmax) per-axis slab (inv = 1 / d)
 *   RT_OP_PERLIN          none; tex = the 6 x 256 0 perlin_turb_global, 1 perlin_turb_lds  |turbulence| at p = o
 *                         R32F table              (the packed table staged in LDS)
 *   RT_OP_SPHERE_UV       none                    0 (sphere_uv)                            u, v at p = o
 *   RT_OP_TEXTURE         none; tex = slot 0's    0 (texture_color's checker and image     r, g, b
 *                         texture                 branches: p = o, uv = (d.x, d.y), the
 *                                                 texture id = the row's int word)
 * t, t1, t2, face, alpha, beta mean something only where hit / ok is 1.
 * flags (may be NULL) gets what the host half computed:
 *   flags[0] 1 when every record is in the shared-reciprocal regime (spheres_fd, prep_quads,
 *            prep_boxes: the product takes the fd forms only then), 1 for ops without records
 *   flags[1] RT_OP_BOX: boxes whose 48-byte record is compact (forms 2..4 need all n);
 *            RT_OP_PERLIN: 1 when the table packs (form 1 needs it)
 *   flags[2] waves of the batch that hold a row whose a = dot(d, d) is not >= 2^-60 (such a wave
 *            takes '/' in the fd sphere forms), flags[3] such rows
 * device < 0: the host half alone (flags), nothing is launched and out is not written.
 * Returns RT_ERR_INVALID_ARG for a form the records do not allow (a compact form with a box that
 * is not compact, the packed form with a table that does not pack). */
enum {
    RT_OP_SPHERE = 0, RT_OP_MEDIUM_SPHERE, RT_OP_QUAD, RT_OP_BOX, RT_OP_NODE, RT_OP_PERLIN, RT_OP_SPHERE_UV,
    RT_OP_TEXTURE, RT_OP_N
};
#define RT_OPS_ROW_F 12
#define RT_OPS_OUT_W 8
int rt_debug_eval_op(int device, int op, int form, const void* recs, size_t rec_bytes, const float* rows, int n,
                     int tex_format, int tex_w, int tex_h, const void* tex, unsigned int* out, int flags[4]);

/* Evaluate one of the render kernels' sampling, light, camera or shading operations on the first
 * device of `ctx`, one lane per row, by the device function the kernels call (csrc/rt_shade_eval.hip;
 * tests/test_gpu_shade_ops.py compares every form with the CPU oracle's oracle_eval_shade_op word for
 * word).  Rows run in whole waves in input order, padded with copies of the last row, as in
 * rt_debug_eval_op.  The scene is the one the context uploaded: spheres, quads, boxes, dquads, media,
 * lights, textures, camera, background and sqrt_spp.  The argument block comes from the functions
 * rt_render uses (csrc/rt_args.h scene_args) with every LDS offset set to -1, so all records are read
 * from global memory.
 * Row i of `rows`: RT_SOP_ROW_F floats (ints as their bits):
 *   [0..2] o   [3..5] d   [6] hit t   [7] tif (prim type | box face << 4 | prim index << 16)
 *   [8] time   [9] px   [10] py   [11] rf   [12..14] acc   [15] UvSrc kind_idx   [16..18] UvSrc a, b, c
 *   [19] frame_count
 * Row i of `out`: RT_SOP_OUT_W 32-bit words (floats as their bits; unused words 0).
 *   op                     device function     in                                  out words
 *   RT_SOP_RAND            rnd                 px, py, rf                          6 successive draws, rf after
 *   RT_SOP_ONB             transform_onb       vec = [0..2], normal = [3..5]       x, y, z
 *   RT_SOP_UNIT_VEC        rand_unit_vec       px, py, rf                          x, y, z, rf after
 *   RT_SOP_MEDIUM_TAIL     medium_tail         [0] neg_inv_density, [1] t1, [2] t2, hit, t (0 on a miss), rf after
 *                                              [3] a = dot(d, d), [4] tmin,
 *                                              [5] tmax, px, py, rf
 *   RT_SOP_LIGHT_PDF       lights_pdf_value    o, d, time                          pdf
 *   RT_SOP_LIGHT_DIR       lights_random       o, px, py, rf                       x, y, z, rf after
 *   RT_SOP_CAMERA_RAY      start_path (base as px, py, frame_count, rf (= rf0)     time, o, d, rf after
 *                          the render kernel
 *                          writes it)
 *   RT_SOP_SHADE           shade<>             o, d, t, tif, time, px, py, rf,     ended; result r, g, b when ended,
 *                                              acc, UvSrc                          else o, d, acc (words 1..9);
 *                                                                                  word 10 rf after
 *   RT_SOP_TRACE           plain_walk, walk_uv o, d, time, px, py, rf, UvSrc          hit, t, tif (t and tif 0 on a miss),
 *                          (rt_plain_walk.h)                                       UvSrc after the walk (words 3..6:
 *                                                                                  kind_idx, a, b, c), word 7 rf after
 * RT_SOP_TRACE is ray_color's closest-hit walk over ray_t = [0.001, infinity): one lane per row runs the plain
 * link walk (the context's plain link buffer, from global memory, from the root: no spine, collapse or pre-test
 * nodes) and the generic leaf tests with media on -- the loop the first-hit pass runs with media cleared -- then
 * hands the walk's uv over as after_trace() does.  A zero direction hits nothing and draws nothing.  The words
 * are those of the oracle's op 8 (oracle/rt_oracle.h) except words 8..10, which stay 0 here: the oracle's
 * visited-node count, leaf-slot count and visit hash describe the reference's stack walk, and the link walk's
 * nodes differ from it by design (the same leaves in the same order).  Form 0: leaf_prims_t<false, false>
 * under the context's box pre-test margin (option box_pretest on or off gives the same words); form 1:
 * leaf_prims_t<false, true>, the shared-reciprocal divisions, RT_ERR_INVALID_ARG unless the scene is in that
 * regime (rt_debug_last_launch out[2] of a render of it).  The link walk is acyclic, so it ends on any input.
 * form: 0, except RT_SOP_TRACE (above) and RT_SOP_SHADE: 0 shade<false, false, false, false>, 1 shade<false, false, false, true>
 * (the per-pass trims of the compact-box kernels: the no-light mixture).  Form 1 gives form 0's words
 * but one: on a scene without lights, a row whose mixture draw is below 0.5 leaves rf one draw short of
 * form 0's (word 10 is one float32 addition of 0.001 less), because the trim leaves out lights_random,
 * whose draw nothing reads: such a row's path has ended, or goes on along vec3(0) and draws no more.
 * The call runs validate() and scene_args() on the context, as rt_render does, so it may refresh the
 * context's planned state (the walk's links, the scene extent, the leaf census); it renders nothing.
 * The guard below checks the rows, not the scene: a hit's texture id is used as the scene holds it.
 * Input guard: the rejection loops of rand_unit_vec and start_path never end on draws that are NaN, so
 * unless every row's px and py are finite and in [0, 16384) and its rf is finite and in [0, 4096) the
 * call returns RT_ERR_INVALID_ARG before anything is launched; likewise for a RT_SOP_SHADE row whose
 * tif or UvSrc names a record the scene does not hold.  Other fields may be NaN or infinite.
 * device < 0: the guard alone (ctx may be NULL), nothing is launched and out is not written. */
enum {
    RT_SOP_RAND = 0, RT_SOP_ONB, RT_SOP_UNIT_VEC, RT_SOP_MEDIUM_TAIL, RT_SOP_LIGHT_PDF, RT_SOP_LIGHT_DIR,
    RT_SOP_CAMERA_RAY, RT_SOP_SHADE, RT_SOP_TRACE, RT_SOP_N
};
#define RT_SOP_ROW_F 20
#define RT_SOP_OUT_W 12
struct rt_ctx;
int rt_debug_eval_shade_op(struct rt_ctx* ctx, int device, int op, int form, const float* rows, int n,
                           unsigned int* out);

/* Host-only: the threaded-BVH re-layout rt_upload_buffer(RT_BIND_BVH) builds
 * (32-byte rt_dnode records); out may be NULL to query the count. */
int rt_debug_threaded_bvh(const void* nodes, size_t nbytes, void* out, size_t out_cap, int* n_out);

/* Host-only: the exact near-first walk's tables (RT_KERNEL_VARIANT=60) for a
 * reference BVH upload plus its quad and box records: 8 octant layouts of
 * n_per_octant threaded rt_dnode records, one word per solid prim (spheres,
 * then quads, then boxes: reference rank << 16 | reference leaf node) and the
 * media slots in visit order (4 ints each: medium, leaf, tracker, flags).
 * Returns 1 when the walk is usable, 0 when every ray takes the exact walk. */
int rt_debug_fast_tables(const void* bvh, size_t nbytes, const void* quads, size_t qbytes, const void* boxes,
                         size_t bbytes, int n_spheres, void* nodes_out, size_t nodes_cap, int* n_per_octant,
                         unsigned int* info_out, size_t info_cap, int* slots_out, int* n_slots);

/* Host-only: the link-format copy of a reference BVH upload that the default
 * kernel walks (rt_device.h RT_LINK_*): the threaded nodes placed breadth-first,
 * two float4 each (box, hit / miss successor byte addresses), then the leaves'
 * (types | next address << 8, prims) as uint2.  *n_f4 = its float4 count, 0 when
 * there is no BVH. */
int rt_debug_link_nodes(const void* bvh, size_t nbytes, void* out, size_t out_cap, int* n_f4);
/* The same with the box pre-test nodes (option box_vnodes): vbox = 6 floats per box (its
 * pre-test bounds: xmin, xmax, ymin, ymax, zmin, zmax); *n_nodes = tree + pre-test nodes. */
int rt_debug_link_nodes_vbox(const void* bvh, size_t nbytes, const float* vbox, int n_box, void* out,
                             size_t out_cap, int* n_f4, int* n_nodes);
/* The link-format nodes of `bvh` as the walk of a context uses them: with rebuild != 0 the inner
 * nodes rebuilt over the leaf sequence (option rebuild, rt_prep.cpp rebuild_inner), then the node
 * collapse of option collapse (plan_collapse) planned for camera `cam` (rt_camera_ubo, 28
 * floats) and a width x height image; drop (may be NULL) gets one byte per threaded node of that
 * tree (1 = left out), *n_dropped their count.  Host-side, no device needed
 * (tests/test_link_nodes.py replays the walk). */
int rt_debug_collapse_links(const void* bvh, size_t nbytes, const float cam[28], int width, int height, int rebuild,
                            void* out, size_t out_cap, int* n_f4, unsigned char* drop, size_t drop_cap,
                            int* n_dropped);

/* Host-only: the packed Perlin table rt_upload_texture keeps beside an R32F 6 x 256 texture
 * whose perm columns (3..5) hold whole numbers 0..255: 256 float4 (ranvec x, y, z; the three
 * perm entries as bytes 0, 1, 2 of the fourth word).  Returns 1 (table written to out when
 * out != NULL), 0 when the texture does not qualify (the kernel then reads it as uploaded). */
int rt_debug_perlin_pack(const float* texels, int w, int h, void* out, size_t out_cap);

/* Host-only: per mille of a reference BVH upload's leaves that hold two spheres; rt_render
 * takes the sphere-pair kernels at >= 500 (and when the boxes are not all canonical). */
int rt_debug_sphere_pair_leaves(const void* bvh, size_t nbytes, int* permille);

/* Host-only: rt_read_image's device de-interleave (deinterleave_kernel) with the same
 * row indexing (rt_device.h rt_gathered_row), on the host (tests compare it with
 * rt_deinterleave_rows). */
int rt_debug_deinterleave(const float* gathered, int width, int height, int world, int stripe_rows, float* out);

/* Host-only: the boxes' 48-byte records rt_upload_buffer(RT_BIND_BOXES) builds
 * (rt_prep.cpp box_record: 3 float4 per box; float4[2].y = 1 for a compact record,
 * whose faces the kernel rebuilds from it) and how many are compact. */
int rt_debug_box_records(const void* boxes, size_t nbytes, void* out, size_t out_cap, int* n_compact);

/* Diagnostic build of the render kernel with wave-level region timers and
 * active-lane counters (never used for timed numbers).  enable=1 switches the
 * context to it and zeroes the counters; enable=2 also records the leaf census
 * (one record per wave leaf round: start cycle, cycles, workgroup | wave << 16 |
 * walking lanes << 24, slot 0's and slot 1's lanes per prim type as bytes: sphere,
 * quad, medium, box); read returns n <= 128 counters.  read_census copies the first
 * device's census (per resident wave its record count, then *cap records of 5 words
 * per wave); out may be NULL to query *needed (words), *waves and *cap.
 * The stats kernels exist only in the A/B build (librtamd_ab.so, built with
 * -DRT_AB_KNOBS); the release library returns RT_ERR_STATE. */
struct rt_ctx;
int rt_debug_enable_stats(struct rt_ctx* ctx, int enable);
int rt_debug_read_stats(struct rt_ctx* ctx, unsigned long long* out, int n);
int rt_debug_read_census(struct rt_ctx* ctx, unsigned int* out, size_t words, size_t* needed, int* waves, int* cap);
/* The stats twin's node-hit count (A/B experiments on the collapse plan, tools/collapse_hits_ab.py):
 * count_node_hits(ctx, 1) zeroes and arms it (0 frees it); read_node_hits gives, per link node of
 * the last launch's layout, the box tests that hit, then the walks begun at the root
 * (*n_out = nodes + 1 words; out may be NULL); set_collapse_hits plans the collapse from such counts
 * (per node of the walk's tree, breadth-first, as read with collapse and spine off) instead of the
 * camera grid (n = 0: the grid again). */
int rt_debug_count_node_hits(struct rt_ctx* ctx, int on);
int rt_debug_read_node_hits(struct rt_ctx* ctx, unsigned int* out, size_t words, size_t* n_out);
int rt_debug_set_collapse_hits(struct rt_ctx* ctx, const unsigned int* hits, size_t n, unsigned long long walks);

/* The first device's staged per-frame colours of the last launch, as
 * [n_frames][local_rows][W][4] floats (sparse staging decoded: a clear flag is the zero
 * colour; the fourth component is whatever the kernel stored, folds ignore it).  out may be
 * NULL to query *n_frames; RT_ERR_LIMIT if cap_floats is short, RT_ERR_STATE when the last
 * launch was not staged.  tests/test_gpu_moments.py replays the folds from them. */
int rt_debug_read_samples(struct rt_ctx* ctx, float* out, size_t cap_floats, int* n_frames);

/* Number of visible HIP devices (0 when none). */
int rt_debug_device_count(void);

/* 1 when this library is the A/B build (-DRT_AB_KNOBS: kernel variants, stats
 * twins, non-exact ablations and the RT_* environment knobs), 0 for the release
 * library, whose output depends on nothing but its inputs. */
int rt_debug_ab_build(void);

/* Per-context options for tests and A/B runs, set by explicit calls (never read
 * from the environment by the release library).  Every option below 100 changes
 * only how the work is laid out or which exact form of a test runs, never a bit
 * of the image (tests/ compare each against the default).  Options >= 100 exist
 * in the A/B build only (the release library returns RT_ERR_INVALID_ARG). */
enum {
    RT_OPTION_BOX_PRETEST = 1,          /* box bounds pre-test (1)                          */
    RT_OPTION_FASTDIV = 2,              /* shared-reciprocal division where exact (1)       */
    RT_OPTION_SPH_LDS = 3,              /* leaf records staged in LDS (1)                   */
    RT_OPTION_BIG_WG = 4,               /* 1024-thread workgroups when records fit (1)      */
    RT_OPTION_CHUNK_TARGET = 5,         /* ordered units per resident wave; 0 = one per tile (16) */
    RT_OPTION_STAGED_CHUNK_TARGET = 6,  /* staged units per resident wave (48)              */
    RT_OPTION_STAGE_TILES = 7,          /* stage chunks below this many tiles per wave (2^20) */
    RT_OPTION_SM_BATCH = 8,             /* shading batch, lanes (64)                        */
    RT_OPTION_SM_FRAC = 9,              /* shading batch, 64ths of the walking lanes (0 =   
                                           by kernel: 50 compact-box kernels, else 56)      */
    RT_OPTION_WALK_FRAC = 10,           /* partial node walks, 64ths (0: by BVH size)       */
    RT_OPTION_WATCHDOG_MS = 11,         /* a wave that stores no sample for this long sets
                                           the fault word and leaves (120000); 0 = at once  */
    RT_OPTION_CHUNK_WAIT_MS = 12,       /* ordered-chunk wait bound (30000); 0 = at once    */
    RT_OPTION_LDS_NODE_CAP = 13,        /* bytes of BVH nodes staged in LDS; the rest is
                                           read from global memory (0 = as many as fit)     */
    RT_OPTION_COMPACT_BOXES = 14,       /* canonical boxes from 48-byte LDS records (1)     */
    RT_OPTION_SPINE = 15,               /* walks start past the root's right spine when its
                                           boxes surely hold the ray's origin (1)           */
    RT_OPTION_TL_LEAF_LDS = 16,         /* two-level walk: leaf records in LDS beside the
                                           top levels when they take <= half of it (1)      */
    RT_OPTION_PERLIN_PACKED = 17,       /* Perlin table staged as 256 float4 with packed
                                           perm bytes when its entries allow it (1)         */
    RT_OPTION_SPARSE_STAGE = 18,        /* staged chunks write only colours that are not
                                           exactly zero, plus a flag byte per sample (1)    */
    RT_OPTION_SPHERE_PAIRS = 19,        /* kernels testing a two-sphere leaf's spheres at
                                           once, when most leaves are such pairs (1); 2:
                                           always, compact-box kernels included            */
    RT_OPTION_LEAF_PREFETCH = 20,       /* compact-box kernels: each leaf slot's record loaded
                                           before the prim-type blocks when spheres, boxes
                                           and media are all staged in LDS (1)              */
    RT_OPTION_TL_SMALL_LDS = 21,        /* two-level walk: room is reserved beside the top
                                           levels for the sphere / compact box records that
                                           take at most 1/16 of it, and each table is staged
                                           whenever it fits after the nodes (1); 0: neither */
    RT_OPTION_SHADE_LDS = 22,           /* shading tables in LDS: sphere and compact box
                                           materials, texture descriptors, small texture
                                           slots (1)                                        */
    RT_OPTION_BOX_VNODES = 23,          /* compact-box kernels: each all-box leaf's box bounds
                                           pre-tests as nodes of the walk, the leaf stage
                                           testing only the boxes they pass (1)            */
    RT_OPTION_ZERO_DIR_END = 24,        /* a path whose next direction is vec3(0) (the no-
                                           light branch) ends in its shading pass with the
                                           miss colour its next bounce would give (1)       */
    RT_OPTION_COLLAPSE = 25,            /* the link walk leaves out the inner nodes whose
                                           tests a grid of camera rays says cost more than
                                           they save (rt_prep.cpp plan_collapse) (1)        */
    RT_OPTION_REBUILD = 26,             /* the link walk's inner nodes rebuilt over the
                                           reference's leaf sequence (joined boxes: the same
                                           leaves, order and ray_t; rt_prep.cpp
                                           rebuild_inner): 1 greedy surface-area splits,
                                           2 the least summed inner-box area (default); 0 off */
    RT_OPTION_TAIL_CHUNKS = 27,         /* staged launches end with this many one-frame
                                           chunks: the units claimed last are short (only
                                           the grouping of samples into units changes);
                                           -1 (default): 1 above 1024 BVH nodes, else 0  */
    RT_OPTION_BOX_INTERIOR = 28,        /* compact-box kernels of the default launch: a box's
                                           planes from one reciprocal per axis, its faces
                                           accepted without dividing, alpha / beta divided
                                           once for the accepted face (1)                   */
    RT_OPTION_FIRST_LEAF = 29,          /* the same kernels: when the spine ends at its leaf, a
                                           walk that starts past the spine tests that leaf
                                           where it begins, from a wave-uniform record, before
                                           its first round (rt_debug_first_leaf) (1)        */
    RT_OPTION_KERNEL_VARIANT = 100,     /* A/B build: 0, 37, 30, 61 (+ stats twins)         */
    RT_OPTION_DEBUG_FLAGS = 101         /* A/B build: ablations, NOT exact                  */
};
int rt_debug_set_option(struct rt_ctx* ctx, int option, int value);
int rt_debug_get_option(struct rt_ctx* ctx, int option, int* value);

/* What the last rt_render launched on the context's first device (tests assert
 * that the intended path ran):
 *   out[0] launch shape (0 fast-lds, 1 fast-global, 2 link-lds, 3 meta-lds,
 *          4 meta-global, 5 link two-level: top nodes in LDS, the rest global)
 *   out[1] workgroup size          out[2] shared-reciprocal division on (1/0)
 *   out[3] box pre-test on (1/0)   out[4] dynamic LDS bytes
 *   out[5] BVH nodes staged in LDS out[6] box records: bit 0 compact tests, bit 1 in LDS
 *   out[7] staged chunks (1/0)     out[8] chunks per launch
 *   out[9] spine nodes a walk may skip (0 = off)
 *   out[10] sparse staging (1 = a flag byte per sample, only non-zero colours stored)
 *   out[11] sphere-pair kernel (1 = a two-sphere leaf's spheres tested at once)
 *   out[12] leaf record prefetch  out[13] shading tables in LDS (bits)  out[14] walk threshold
 *   out[15] the BVH the walk ran on: RT_BVH_REFERENCE (0) or RT_BVH_SAH (1, rt_set_bvh_mode)
 *   out[16] box pre-test nodes in the walk (option box_vnodes; 0 = none)
 *   out[17] inner nodes the walk leaves out (option collapse; 0 = none)
 *   out[18] the walk's inner nodes rebuilt over the leaf sequence (option rebuild; 1/0)
 *   out[19] division-free compact box test compiled into the kernel (option box_interior; 1/0)
 *   out[20] tiles the launch sampled: the active tiles of the mask (rt_set_active_tiles), every
 *           tile without one; 0 when the render launched nothing because no tile was active
 * n <= 21 ints are written; returns RT_ERR_STATE before the first render. */
int rt_debug_last_launch(struct rt_ctx* ctx, int* out, int n);

/* The first-leaf prologue of the last rt_render on the context's first device (option first_leaf):
 *   out[0] 1 when it was armed -- the option on, the spine on and ending at its leaf, and a kernel
 *          that holds the prologue (out[19] of rt_debug_last_launch) -- else 0, and the rest 0
 *   out[1] the leaf's link (the spine's start: sign bit | leaf ordinal)
 *   out[2] the leaf record's type byte (slot 0's type in bits 0-3, slot 1's in bits 4-7)
 *   out[3] its prim word (slot 0's index in bits 0-15, slot 1's in bits 16-31)
 * Returns RT_ERR_STATE before the first render. */
int rt_debug_first_leaf(struct rt_ctx* ctx, int out[4]);

/* Host-only: the launch decision of a render (which kernel instantiation, with how much LDS, and
 * the rt_debug_last_launch fields it reports) for the deciding inputs in[RT_PK_*] -- the launch's
 * scalar arguments, and 1/0 for each buffer it has -- as the release library decides it (ab = 0) or
 * the A/B library (ab = 1: the kernel variants of RT_PK_VARIANT), whichever library is asked.
 * out[RT_PKO_*] gets the plan and the arguments it edits, info[21] the fields of
 * rt_debug_last_launch it sets (15..18 stay 0); of a refused launch (out[RT_PKO_OK] 0) only the
 * edited arguments are given (from RT_PKO_ACC_LDS on), the rest is 0.  table (may be NULL) gets the release library's render kernel
 * instantiations as (workgroup size, OPT) pairs, *n_table (may be NULL) their count;
 * RT_ERR_LIMIT if table_cap (pairs) is short. */
enum {
    RT_PK_VARIANT = 0,   /* RT_OPTION_KERNEL_VARIANT                                              */
    RT_PK_BLOCK,         /* workgroup size of the LDS plan: 512 or 1024                           */
    RT_PK_N_ACTIVE,      /* tiles the launch samples                                              */
    RT_PK_SAMPLES, RT_PK_SFLAGS, RT_PK_WBUF, RT_PK_TILE_LIST,   /* 1/0: staged colours, sparse flags,
                            the per-wave slots of ordered launches, a tile mask                   */
    RT_PK_N_NODES, RT_PK_N_LNODE_F4, RT_PK_LDS_NODE_F4, RT_PK_LDS_END_F4,   /* link nodes, float4 of
                            their array, float4 of nodes in LDS, float4 end of everything staged  */
    RT_PK_N_F2INNER, RT_PK_N_F2LEAVES,   /* the near-first walk's tree (A/B)                      */
    RT_PK_FASTDIV, RT_PK_BOX_ALL_CMP, RT_PK_BOX_INTERIOR, RT_PK_SPH_PAIRS, RT_PK_LEAF_PF,
    RT_PK_MEDIA_SPH, RT_PK_N_MEDIA, RT_PK_N_SPH_LDS, RT_PK_N_BOX_LDS,
    /* float4 offsets of the tables in LDS, -1 = not staged */
    RT_PK_PERLIN_LDS, RT_PK_MEDIA_LDS, RT_PK_SPH_LDS, RT_PK_BOX_CMP_LDS, RT_PK_SPH_MAT_LDS, RT_PK_BOX_MAT_LDS,
    RT_PK_TEX_LDS,
    RT_PK_PRETEST,       /* 1/0: the box bounds pre-test is on                                    */
    RT_PK_N_CHUNKS, RT_PK_SPINE_LEN, RT_PK_WALK_FRAC,   /* reported only                          */
    RT_PK_N
};
enum {
    RT_PKO_OK = 0,       /* 0: the launch is refused                                              */
    RT_PKO_SHAPE, RT_PKO_STATS, RT_PKO_POOL, RT_PKO_BLOCK, RT_PKO_OPT, RT_PKO_LDS_BYTES,
    RT_PKO_ACC_LDS, RT_PKO_LEAF_PF,   /* the arguments as the plan leaves them, and the offsets:  */
    RT_PKO_PERLIN_LDS, RT_PKO_MEDIA_LDS, RT_PKO_SPH_LDS, RT_PKO_BOX_CMP_LDS, RT_PKO_SPH_MAT_LDS,
    RT_PKO_BOX_MAT_LDS, RT_PKO_TEX_LDS,
    RT_PKO_N
};
int rt_debug_plan_kernel(const int* in, int n_in, int ab, int* out, int n_out, int* info, int* table, int table_cap,
                         int* n_table);

/* Host-only: what rt_render would assemble for a scene and launch first, with no context and no
 * device: the uploads' host halves, validation, the walk's trees, the scene's kernel arguments, the
 * unit split and the frame counts, by the functions rt_render itself runs (csrc/rt_args.h).
 * In: the six bindings as for rt_upload_buffer (all six count as uploaded), textures as for
 * rt_upload_texture (tex_w[slot] = 0: none), the camera UBO, rt_set_params' values, the image size
 * and partition, n_options (option, value) pairs as for rt_debug_set_option (ab = 1: the A/B
 * library's options >= 100 too, RT_OPTION_KERNEL_VARIANT among them), rt_set_bvh_mode's mode,
 * rt_set_moments' switch, a tile mask as its n_mask ascending tile indices (n_mask < 0: no mask), the
 * frame counts before the call (prev_frames for every tile, or prev_tile_frames, one per tile of the
 * rank's stripe), rt_render's first_frame and n_frames, and the two numbers rt_render asks the device
 * for: its resident waves and its free bytes.
 * Out: pk, the RT_PK_* inputs of the first launch (feed them to rt_debug_plan_kernel); launched, 0
 * when the call launches nothing (an empty mask, no frame, no row) and pk is all 0; the
 * rt_debug_last_launch fields rt_render fills itself; rt_debug_first_leaf's words (by the kernel
 * rt_debug_plan_kernel chooses for pk) and the prologue's argument words; plan_split's and the
 * first launch's plan_chunks' results; the frame counts after the call (frames_all; n_tile_frames
 * counts written to tile_frames when the tiles differ, else 0; RT_ERR_LIMIT if tile_cap is short).
 * Optional (NULL: not wanted): links / links_cap gets the walk's link array (links_f4 float4), args /
 * args_cap the first launch's rt_kernel_args block (args_bytes; csrc/rt_device.h) with every pointer
 * and the rand factors zeroed.  Returns what the upload, rt_render or option call it mirrors would. */
typedef struct rt_debug_scene_in {
    const void* buf[6];
    size_t buf_bytes[6];
    int tex_format[8], tex_w[8], tex_h[8];
    const void* tex[8];
    const float* camera;   /* 28 floats */
    int max_depth;
    float background[3], sqrt_spp, recip_sqrt_spp;
    int width, height, rank, world, stripe_rows;
    const int* options;
    int n_options;
    int ab, bvh_mode, moments;
    const int* mask;
    int n_mask;
    int prev_frames;
    const int* prev_tile_frames;
    int first_frame, n_frames;
    long long waves;
    size_t free_bytes;
} rt_debug_scene_in;
typedef struct rt_debug_scene_out {
    int pk[RT_PK_N];
    int launched;
    int bvh_mode, vnodes, collapsed, rebuilt;
    int first_leaf[4];
    unsigned int first_leaf_args[3], spine_start;
    int per_launch, chunks_wanted, staged;
    int n_chunks, chunk_frames, tail_chunks, stage;
    int frames_all, n_tile_frames;
    int* tile_frames;
    int tile_cap;
    void* links;
    size_t links_cap;
    int links_f4;
    void* args;
    size_t args_cap, args_bytes;
} rt_debug_scene_out;
int rt_debug_plan_scene(const rt_debug_scene_in* in, rt_debug_scene_out* out);

/* The BVH the link walk of ctx uses, in the reference's node format (rt_bvh_node): the
 * uploaded one, or in RT_BVH_SAH mode the tree rt_set_bvh_mode builds (validated as by
 * rt_render).  out may be NULL to query *nbytes; returns RT_ERR_LIMIT if out_cap is short.
 * Tests feed it to the CPU oracle: the kernel on the SAH tree is bit-exact against the
 * oracle walking the same tree. */
int rt_debug_walk_bvh(struct rt_ctx* ctx, void* out, size_t out_cap, size_t* nbytes);

/* Context-free form of the RT_BVH_SAH build (no device needed): the SAH tree over the prims
 * of `bvh` (the reference's nodes), from the uploaded record bytes of the other bindings.
 * order: 0 the larger child (surface area) first, 1 the smaller first, 2 the child nearer
 * to eye[3] first (rt_set_bvh_mode's, with the camera position); prim_cost: the SAH cost of a
 * prim test in node steps (rt_set_bvh_mode's: 1). */
int rt_debug_build_sah_bvh(const void* spheres, size_t sph_bytes, const void* quads, size_t quad_bytes,
                           const void* media, size_t med_bytes, const void* boxes, size_t box_bytes,
                           const void* bvh, size_t bvh_bytes, int order, const float eye[3],
                           float prim_cost, void* out, size_t out_cap, size_t* nbytes);

#ifdef __cplusplus
}
#endif

#endif
