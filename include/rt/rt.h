/*
 * rt.h — drop-in C ABI of the MI355X path tracer (librtamd.so).
 *
 * It replaces the OpenGL binding contract that the reference's Java host drives
 * (SURVEY §8b).  Each entry point names the reference call it stands in for.
 * All calls return 0 (RT_OK) or a negative RT_ERR_* code; the message of the
 * last failure on a context is available from rt_last_error().  A context is
 * used by one host thread at a time (the reference's GL-context rule); callers
 * own every host buffer they pass (the library copies what it keeps).
 */
#ifndef RT_H
#define RT_H

#include <stddef.h>
#include <stdint.h>

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,  /* bad pointer/size/enum, record size mismatch       */
    RT_ERR_DEVICE = -2,       /* HIP runtime failure                               */
    RT_ERR_STATE = -3,        /* call order (e.g. render before resize)            */
    RT_ERR_LIMIT = -4,        /* an implicit reference limit exceeded (SURVEY App.C)*/
    RT_ERR_NOMEM = -5,
    RT_ERR_TIMEOUT = -6       /* rt_comm_init / rt_gather_image: a peer did not complete in
                                 time (rt_comm_set_timeout); the communicator was aborted   */
};

/* SSBO binding points (compute.glsl:127-153, RaytraceModel.java:81-113) */
enum {
    RT_BIND_SPHERES = 0, RT_BIND_BVH = 1, RT_BIND_QUADS = 2,
    RT_BIND_MEDIA = 3, RT_BIND_BOXES = 4, RT_BIND_LIGHTS = 5
};


#define RT_MAX_TEXTURES 8        /* uniform sampler2D textures[8], compute.glsl:23 */
#define RT_MAX_RECORDS 65535     /* 16-bit indices in packed ids (App. C)          */
#define RT_MAX_BVH_DEPTH 64      /* int stack[64], compute.glsl:229                */
#define RT_MAX_IMAGE_DIM 65536   /* image width / height (pixel coordinates feed rand()) */
#define RT_MAX_RAND_FACTOR 1024.0f /* |u_rand_factor| (see rt_render)                */

typedef struct rt_ctx rt_ctx;

/* Create a context rendering on n_devices HIP devices (device_ids may be NULL
 * for 0..n-1; explicit ids may repeat, n <= 64).  Rows are split in
 * interleaved stripes over the device slots and gathered on device 0 by
 * rt_read_image (RCCL, see rt_comm_*); the result equals a 1-device render bit
 * for bit.
 * Replaces: Window.initGLFW/initShaderPrograms (Window.java:90-193). */
int rt_create(int n_devices, const int* device_ids, rt_ctx** out);
int rt_destroy(rt_ctx* ctx);
/* Message of the last failure on ctx; with ctx == NULL, of the last failed
 * rt_create on the calling thread. */
const char* rt_last_error(rt_ctx* ctx);
int rt_abi_version(void);

/* Upload one SSBO's exact std430 bytes (rt_types.h records; lights = int count
 * followed by count packed ints).  nbytes must be a multiple of the record size.
 * Replaces: RaytraceModel.put{Spheres,BVHNodes,Quads,ConstantMediums,Boxes,
 * Lights}ToProgram -> BufferObject.uploadData (RaytraceModel.java:138-246). */
int rt_upload_buffer(rt_ctx* ctx, int binding, const void* bytes, size_t nbytes);

/* Upload texture slot 0..7; rows tightly packed, row 0 first (glTexImage2D).
 * Sampling follows GL_LINEAR + CLAMP_TO_EDGE (Texture.java:74-77).
 * Replaces: Texture.putData (Texture.java:122-133). */
int rt_upload_texture(rt_ctx* ctx, int slot, int format, int w, int h, const void* texels);

/* The 28-float std140 camera block (rt_camera_ubo).
 * Replaces: Camera.putToShaderProgram UBO upload (Camera.java:121-139). */
int rt_set_camera(rt_ctx* ctx, const float ubo[28]);

/* Uniforms max_depth, background, sqrt_spp, recip_sqrt_spp.
 * Replaces: GuiRenderer.maxDepthUpdate, Camera.putToShaderProgram("background"),
 * RaytraceExecutor.setSamplePerPixel (RaytraceExecutor.java:50-56). */
int rt_set_params(rt_ctx* ctx, int max_depth, const float background[3],
                  float sqrt_spp, float recip_sqrt_spp);

/* (Re)allocate the RGBA32F accumulation image, zero-filled; 1 <= w, h <= RT_MAX_IMAGE_DIM.
 * Replaces: Texture.resize on the framebuffer callback (Window.java:116-129). */
int rt_resize(rt_ctx* ctx, int w, int h);

/* Run n_frames progressive frames.  Equal to n_frames x { frame_count =
 * first_frame+i; u_rand_factor = rand_factors[i]; glDispatchCompute;
 * glMemoryBarrier }.  Asynchronous on the context's stream(s).  Each rand
 * factor must be finite with |value| <= RT_MAX_RAND_FACTOR (the reference
 * passes (float)Math.random() in [0, 1); beyond, rand()'s +0.001 steps vanish).
 * Replaces: RaytraceExecutor.raytrace (RaytraceExecutor.java:100-142). */
int rt_render(rt_ctx* ctx, int first_frame, int n_frames, const float* rand_factors);

/* Wait for all queued renders. */
int rt_sync(rt_ctx* ctx);

/* Copy the accumulation image (W*H*4 floats, row 0 = top) to the host.
 * Replaces: glGetTexImage in Texture.saveAsPNG (Texture.java:93). */
int rt_read_image(rt_ctx* ctx, float* rgba);

/* Overwrite the accumulation image (resume a checkpointed accumulation). */
int rt_write_image(rt_ctx* ctx, const float* rgba);

/* Device time of the last rt_render call (max over devices), after completion.
 * Replaces: QueryTimer GL_TIME_ELAPSED (QueryTimer.java:24-50). */
int rt_last_render_ns(rt_ctx* ctx, uint64_t* ns);

/* Non-blocking: returns 1 with *ns (max over devices) once the last rt_render
 * call has finished on the device, 0 while it still runs (*ns untouched).
 * Replaces: the polling of finished QueryTimer results that feeds
 * lastDispatchTime on every raytrace() (RaytraceExecutor.java:106-115). */
int rt_render_done(rt_ctx* ctx, uint64_t* ns);

/* ---- MI355X-native extensions (no reference counterpart) ---------------- */

/* Multi-process partition (one process per GPU): this context renders only the
 * rows r with (r / stripe_rows) % world == rank.  Its image then holds
 * local_rows = rt_local_rows(...) rows, stripe-compacted; gather with
 * torch.distributed (RCCL) and rt_deinterleave_rows().  Must precede rt_resize. */
int rt_set_partition(rt_ctx* ctx, int rank, int world, int stripe_rows);
int rt_local_rows(int height, int rank, int world, int stripe_rows);
int rt_padded_local_rows(int height, int world, int stripe_rows);

/* Bind a caller-owned device buffer (>= W*local_rows*16 bytes, on the context's
 * single device) as the accumulation image instead of an internal one; pass
 * NULL to go back to the internal image.  Must follow rt_resize. */
int rt_bind_device_image(rt_ctx* ctx, void* device_ptr, size_t nbytes);

/* Use a caller-provided hipStream_t (e.g. torch's current stream); NULL = own. */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);

/* ---- RCCL over xGMI behind the ABI (the partition's one exchange).
 * A context over several devices (rt_create(n > 1)) gathers in rt_read_image: each
 * device's stripe block to device 0 over RCCL (ncclCommInitAll; one ncclSend /
 * ncclRecv pair per device) when the device ids are distinct, else by peer copies,
 * then a de-interleave kernel on device 0 and one copy to the host.
 * One process per GPU: rank 0 makes a communicator id (RT_COMM_ID_BYTES bytes) that
 * the host hands to every rank by its own means (the reference has no transport);
 * each rank, after rt_set_partition(rank, world, ...), calls rt_comm_init; then
 * rt_gather_image sends every rank's stripe block to rank 0 over RCCL, where it is
 * de-interleaved on the device and copied out (rgba: W*H*4 floats on rank 0, NULL
 * elsewhere).  librccl.so is loaded on first use. */
#define RT_COMM_ID_BYTES 128
enum { RT_GATHER_HOST = 0, RT_GATHER_PEER = 1, RT_GATHER_RCCL = 2 };
int rt_comm_unique_id(void* id_out);
int rt_comm_init(rt_ctx* ctx, const void* id, int rank, int world);
int rt_gather_image(rt_ctx* ctx, float* rgba);
/* Deadline of rt_comm_init and rt_gather_image on this context, in ms (default 120000;
 * 0 = wait forever).  The communicator is made non-blocking (ncclConfig_t.blocking = 0)
 * where the library allows it, and every wait polls against the deadline: a rank that
 * never joins or never posts its Send / Recv makes the call return RT_ERR_TIMEOUT, with
 * the communicator aborted (its queued work freed), instead of holding the host. */
int rt_comm_set_timeout(rt_ctx* ctx, int timeout_ms);
/* Abort the context's communicator(s) (ncclCommAbort; ncclCommDestroy where absent) and
 * free their queued work.  A later gather needs rt_comm_init again. */
int rt_comm_abort(rt_ctx* ctx);
/* How the last gather ran: RT_GATHER_*, or -1 before any. */
int rt_gather_path(rt_ctx* ctx);

/* Host helper: scatter gathered stripe blocks [world][padded_rows][W][4] into a
 * full W x H image (row 0 = top). */
int rt_deinterleave_rows(const float* gathered, int width, int height, int world,
                         int stripe_rows, float* rgba_out);

/* ---- Non-parity fast mode -------------------------------
 * RT_BVH_REFERENCE (default): the walk runs on the uploaded BVH -- the reference's median
 * split (BVHNode.java:13-56) -- and every image is bit-identical to the reference semantics.
 * RT_BVH_SAH: the context rebuilds the BVH from the uploaded BVH's prims with a binned-SAH
 * builder (leaves of at most two prims; each medium keeps its reference leaf, so its test
 * multiplicity and hence its density are the reference's) and walks that.  Same kernel, same
 * leaf tests; far fewer node visits and prim tests.  NOT bit-exact against the reference
 * BVH: a medium's rand() draws fall at another point of the visit sequence, so images agree
 * statistically (tests/test_gpu_fast_bvh.py).  Takes effect at the next rt_render. */
enum { RT_BVH_REFERENCE = 0, RT_BVH_SAH = 1 };
int rt_set_bvh_mode(rt_ctx* ctx, int mode);

/* ---- Per-pixel sample moments and a noise-target render loop -----------------
 * With moments on, every launch stages its per-frame colours (a one-frame launch too) and
 * the fold that applies the running mean also keeps, per pixel, the sum of squared
 * deviations of the frames' colours from their mean (Welford's update, in f32):
 *   M2.ch += (c.ch - mean_before.ch) * (c.ch - mean_after.ch)   for ch in x, y, z, and
 *   M2.w likewise for the channel sum y = (c.x + c.y) + c.z;  frame 1 sets M2 = 0.
 * The running mean is computed by the same operations as without moments: the image is
 * unchanged bit for bit, and the render kernels are the same.  M2 / (n - 1) is the sample
 * variance over the n frames, M2 / (n (n - 1)) the estimated variance of the mean.  Frames
 * are stratified (each frame takes one cell of the sqrt_spp grid), so the variance between
 * frames overstates the error of the mean: the estimate is conservative.
 *
 * State: the moments cover frames 1 .. n.  rt_render from first_frame 1 restarts them, from
 * n + 1 extends them; any other first_frame, rt_write_image, rt_bind_device_image and
 * rt_resize (which reallocates them zero-filled) make them invalid until the next render
 * from frame 1 or rt_write_moments.  Single-device contexts only (RT_ERR_STATE otherwise);
 * under rt_set_partition every figure is the rank's own rows'. */
typedef struct rt_tile_sum   { float m2y, y; uint32_t bad, pixels; } rt_tile_sum;
typedef struct rt_noise_stats{ double sum_m2y, sum_y; uint64_t pixels, bad; int frames, converged; double noise; } rt_noise_stats;

/* Moments on (1) or off (0, frees the buffer); takes effect at the next rt_render.  Off, the
 * launch plan, kernels and buffers are exactly those of a context that never had them. */
int rt_set_moments(rt_ctx* ctx, int on);
/* M2 as W*local_rows*4 floats in the image's layout; RT_ERR_STATE while invalid. */
int rt_read_moments(rt_ctx* ctx, float* m2_rgba);
/* Resume from a checkpoint (pairs with rt_write_image, which comes first): M2 of frames
 * 1 .. n_frames, n_frames >= 1. */
int rt_write_moments(rt_ctx* ctx, const float* m2_rgba, int n_frames);
/* One record per 8x8 tile of the local image, tiles row-major, ceil(W/8) per row: the f32
 * sums of M2.w and of y = (mean.x + mean.y) + mean.z over the tile's pixels, reduced in a fixed
 * order (lane ty*8+tx, x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1), so they depend on image
 * and moments alone.  A pixel whose y or M2.w is not finite is bad: it adds +0 to both sums and
 * 1 to `bad`.  out may be NULL to query *n_tiles; RT_ERR_LIMIT if cap is short. */
int rt_read_tile_sums(rt_ctx* ctx, rt_tile_sum* out, int cap, int* n_tiles);
/* Host only: the tiles summed in order in double; with P = pixels - bad,
 *   noise = sqrt(max(0, sum_m2y / (frames (frames - 1))) * P) / sum_y,
 * the estimated RMS error of the mean relative to the mean y (0 when sum_y and the numerator
 * are 0, +inf when only sum_y is); frames >= 2, converged = 0. */
int rt_noise_from_tile_sums(const rt_tile_sum* tiles, int n_tiles, int frames, rt_noise_stats* out);
/* rt_sync, the tile sums, rt_noise_from_tile_sums over the frames held (at least 2).  Ranks of
 * a partition add sum_m2y, sum_y, pixels and bad across ranks and apply the formula. */
int rt_noise(rt_ctx* ctx, rt_noise_stats* out);
/* Render frames first_frame, first_frame + 1, ... in batches of batch_frames (the last may be
 * shorter), at most max_frames of them; frame f takes rt_frame_rand_factor(seed, f - 1).  After
 * every batch rt_noise; stops at the first batch boundary with noise <= target_noise
 * (last->converged = 1), else after max_frames (0).  *frames_done = frames rendered by this
 * call.  Not pipelined: frames_done and the image depend on the inputs alone. */
int rt_render_until(rt_ctx* ctx, int first_frame, int max_frames, int batch_frames, uint64_t seed,
                    float target_noise, int* frames_done, rt_noise_stats* last);

/* ---- Adaptive sampling: tile masks, per-tile frame counts, a per-tile stopping rule -----------
 * A sample's bits depend on its pixel, its frame and the scene alone, so a tile whose sampling
 * stopped after frame n holds, pixel for pixel and in its moments, the bits of a plain n-frame
 * render.  Single-device contexts without rt_set_partition (RT_ERR_STATE otherwise).
 *
 * active: one byte per 8x8 tile of the image, tiles row-major, ceil(W/8) per row (the tiles of
 * rt_read_tile_sums); NULL = all tiles again.  While set, rt_render samples only the pixels of
 * tiles whose byte is non-zero; every other pixel's image and moments words are not written.
 * n_tiles must match the image (RT_ERR_INVALID_ARG); rt_resize clears the mask.  With no byte
 * set rt_render launches nothing and returns RT_OK. */
int rt_set_active_tiles(rt_ctx* ctx, const uint8_t* active, int n_tiles);
/* One frame count per tile: the frames 1 .. n the tile holds, 0 = invalid.  For each tile a
 * launch samples, first_frame == 1 sets its count to n_frames, first_frame == count + 1 adds
 * n_frames, anything else sets 0; the other tiles keep theirs.  rt_write_image,
 * rt_bind_device_image and rt_resize set every count to 0, rt_write_moments(n) to n.  The
 * moments are valid when every count is >= 1.  frames may be NULL to query *n_tiles;
 * RT_ERR_LIMIT if cap is short. */
int rt_read_tile_frames(rt_ctx* ctx, int32_t* frames, int cap, int* n_tiles);
/* Resume a checkpoint whose tiles stopped at different frames: after rt_write_image and
 * rt_write_moments, the counts (each >= 0). */
int rt_write_tile_frames(rt_ctx* ctx, const int32_t* frames, int n_tiles);
/* Host only.  rt_noise_from_tile_sums for tiles with their own frame counts; in double, the
 * tiles in order, with P = pixels - bad over all tiles:
 *   noise = sqrt(max(0, sum_t m2y_t / (n_t (n_t - 1))) * P) / sum_y,   every n_t >= 2;
 * out->frames = max n_t, out->sum_m2y the plain sum.  rt_noise uses it when the counts differ. */
int rt_noise_from_tile_sums_frames(const rt_tile_sum* tiles, const int32_t* frames, int n_tiles,
                                   rt_noise_stats* out);
/* Host only, pure.  frames = F, the frames every active tile holds.  In double, tiles in index
 * order, P_t = pixels_t - bad_t:
 *   ybar = sum_t y_t / sum_t P_t over ALL tiles (0 when no good pixel);
 *   lim  = (double)target * ybar;
 *   v_t  = (double)m2y_t / ((double)F * (F - 1)) / P_t;
 * an active tile stays active unless F >= min_frames and (P_t == 0 or v_t <= lim * lim).  An
 * inactive tile stays inactive (active_in NULL: all active).  If every tile satisfies
 * v_t <= lim * lim, the rt_noise figure is <= target.  min_frames >= 2 guards a dark tile
 * against stopping before any path has found the light: with all its samples zero so far its
 * variance estimate is 0, which passes any limit.  n_active may be NULL. */
int rt_adaptive_select(const rt_tile_sum* tiles, const uint8_t* active_in, int n_tiles, int frames,
                       int min_frames, float target, uint8_t* active_out, int* n_active);
/* rt_render_until with the rule above between batches: frames first_frame, first_frame + 1, ...
 * in batches of batch_frames with rt_frame_rand_factor(seed, f - 1); after each batch rt_sync,
 * the tile sums, rt_adaptive_select, and the next batch renders the tiles still active.  Stops
 * when none is (last->converged = 1) or after max_frames (0).  A stopped tile never restarts:
 * its count (rt_read_tile_frames) is the frame at which it stopped.  last = rt_noise's figures
 * at the end; *frames_done = the frames of the longest-sampled tiles rendered by this call.
 * first_frame is 1, or the largest count + 1 with valid counts (RT_ERR_STATE otherwise); tiles
 * with a smaller count are already stopped.  Needs rt_set_moments(ctx, 1); no caller mask may
 * be set (RT_ERR_STATE) and none is left set.  Not pipelined. */
int rt_render_adaptive(rt_ctx* ctx, int first_frame, int max_frames, int batch_frames, int min_frames,
                       uint64_t seed, float target_noise, int* frames_done, rt_noise_stats* last);

/* ---- Variance-guided a-trous preview filter over the sample moments --------------------------
 * An edge-avoiding wavelet filter whose edge-stopping comes from the measured variance of each
 * pixel's mean (the moments above), for the first few dozen frames of a render.  It reads the
 * image, the moments and the per-tile frame counts and writes a buffer of its own: image and
 * moments keep their bits, and rendering continues as if it had never been called.
 *
 * Inputs per pixel: the image's rgb, M2.w, and n = the frame count of the pixel's 8x8 tile (>= 2).
 * All arithmetic is f32 without contraction, using only + - * / sqrtf fabsf and rt_glsl.h's g_max
 * (g_max(a, b) = a < b ? b : a), so a float32 restatement matches bit for bit.
 *   y(C)  = (C.x + C.y) + C.z
 *   C_0   = rgb,   V_0 = g_max(0, M2.w / ((float)n * (float)(n - 1)))   (variance of the mean of y)
 * A pixel whose y or M2.w is not finite is bad: it passes through unchanged at every level and is
 * never used as a tap.  For level i = 0 .. levels-1 with step s = 2^i, at every good pixel p:
 *   1. Vb(p): over the taps (dy, dx) in {-1,0,1}^2 at spacing 1, row-major (dy outer), that lie in
 *      the image and are good, with u = k3[dy] * k3[dx], k3 = (1, 2, 1):
 *        acc = acc + u * V_i(q);  ws = ws + u;   Vb(p) = acc / ws   (acc, ws start at +0).
 *   2. Taps (dy, dx) in {-2..2}^2, row-major (dy outer), q = p + s * (dx, dy); the centre and taps
 *      outside the image or bad are skipped.  With h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *        d  = fabsf(y(p) - y(q)) / (k * sqrtf(Vb(p) + Vb(q)) + 1e-30f)
 *        w  = (h[dy] * h[dx]) * g_max(0, 1 - d)
 *        sw = sw + w;   sc = sc + w * (C_i(q).c - C_i(p).c) for c in x, y, z;
 *        sv = sv + (w * w) * V_i(q)                               (all sums start at +0).
 *   3. den = h0 + sw with h0 = 9/64;   C_{i+1}(p).c = C_i(p).c + sc / den;
 *      V_{i+1}(p) = ((h0 * h0) * V_i(p) + sv) / (den * den).
 * With no neighbour accepted C_{i+1}(p) is C_i(p) exactly; at zero variance the filter is the
 * identity (unless two pixels' y are equal to the bit).  Output: rgb = C_levels, w = 1.
 * csrc/rt_denoise_math.h holds these operations once, for the kernels and for rt_denoise_host.
 *
 * levels is 1 .. RT_DENOISE_MAX_LEVELS, k > 0 and finite; params NULL = the defaults levels 3,
 * k 3.  reserved must be 0 (room for guide-buffer terms without another ABI change).
 * Single-device contexts without rt_set_partition. */
#define RT_DENOISE_MAX_LEVELS 5
typedef struct rt_denoise_params { int levels; float k; int reserved[6]; /* must be 0 */ } rt_denoise_params;

/* Queue the filter on the context's stream behind the queued renders.  The result stays in a
 * buffer of the context until the next rt_denoise, rt_resize, rt_set_moments(ctx, 0) or rt_destroy.
 * RT_ERR_INVALID_ARG: bad params or non-zero reserved.  RT_ERR_STATE: no image, moments off or
 * invalid, a tile count < 2, a multi-device context or one under rt_set_partition. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params);

/* rt_sync, then the filtered image as W*H*4 floats; RT_ERR_STATE with no result held. */
int rt_read_denoised(rt_ctx* ctx, float* rgba);

/* Host only, no device: the same header's arithmetic over caller arrays.
 * image / m2: W*H*4 floats.  tile_frames: one count per 8x8 tile, row-major, each >= 2;
 * n_tiles = ceil(W/8) * ceil(H/8) (RT_ERR_INVALID_ARG otherwise). */
int rt_denoise_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles,
                    int width, int height, const rt_denoise_params* params, float* rgba_out);

/* ---- First-hit feature buffers, and their use as guides of the preview filter -------------------
 * rt_render_features traces one deterministic ray per pixel (x, y) and keeps what it hits first:
 *   coord = (up_left + pixel_delta_u * (float)x) + pixel_delta_v * (float)y   (rt_render's pixel base),
 *   o = camera_pos, d = coord - o, time 0, ray_t = (0.001, RT_INFINITY):
 * the pixel's centre ray through a pinhole at camera_pos -- no jitter, no defocus disk, no rand() draw;
 * the buffers depend on the scene and the camera alone.  The closest hit is the one rt_render's first
 * walk finds for that ray with the constant media left out: the walk runs over the current BVH
 * (rt_set_bvh_mode), tests the leaves in walk order with the render's own leaf tests, each accepted
 * hit shrinking ray_t.max (ties resolve as in the render), and skips every leaf slot of type
 * RT_MODEL_CONSTANT_MEDIUM (a medium's hit draws rand()); a primitive that is only a medium's boundary
 * is in no leaf and is not hit.  Two float4 buffers in the image's layout (row 0 = top):
 *   normal_depth = (N.x, N.y, N.z, t): N the shading normal as the render forms it at p = o + d * t
 *     (sphere: (p - center) / radius; quad or box face: the record's normal; negated when
 *     dot(d, N) >= 0), t the accepted hit's t in units of |d|;
 *   albedo_id = (A.r, A.g, A.b, id): A the attenuation the first bounce multiplies in, the material's
 *     texture at p with this hit's uv at time 0 -- for RT_MAT_DIFFUSE_LIGHT the emission on a
 *     front-face hit and (0, 0, 0) on a back-face hit; id holds the bits of a uint32:
 *     prim type | box face << 4 | prim index << 16.
 * A miss stores N = 0, t = -1, A = the background colour (rt_set_params), id = RT_FEATURE_MISS.
 *
 * The buffers (32 bytes per pixel, allocated by the first rt_render_features; a context that never
 * calls it allocates and runs nothing new) hold the result until rt_upload_buffer, rt_upload_texture,
 * rt_set_camera, rt_set_bvh_mode (stale: RT_ERR_STATE from the readers until the next
 * rt_render_features), rt_resize (freed) or rt_destroy.  rt_set_params does not make them stale: a
 * miss keeps the background of the pass.  Image, moments and frame counts are never touched.
 * Single-device contexts without rt_set_partition (RT_ERR_STATE otherwise). */
#define RT_FEATURE_MISS 0xFFFFFFFFu
/* Queue the pass on the context's stream.  RT_ERR_STATE without BVH, camera or rt_resize. */
int rt_render_features(rt_ctx* ctx);
/* rt_sync, then W*H*4 floats each; either pointer may be NULL.  RT_ERR_STATE while none is held. */
int rt_read_features(rt_ctx* ctx, float* normal_depth, float* albedo_id);

/* The guided filter: rt_denoise's filter with one more factor g on each tap's weight, from the
 * feature buffers; the same rules (f32, no contraction, only + - * / sqrtf fabsf g_max).  A pixel is
 * guide-good when its N, t and A are all finite; hit(p) means id(p) != RT_FEATURE_MISS.  For a tap q
 * of pixel p (both good in rt_denoise's sense):
 *   g = 1                  if p or q is not guide-good
 *   g = 0                  else if hit(p) != hit(q)
 *   g = (gn * gz) * ga     otherwise, where a term whose k is exactly 0 is exactly 1, and
 *     gn = 1 for two misses, else g_max(0, 1 - kn * (1 - ((N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z)))
 *     gz = 1 for two misses, else g_max(0, 1 - kz * (fabsf(t_p - t_q) / (g_max(t_p, t_q) + 1e-30f)))
 *     ga = g_max(0, 1 - ka * ((fabsf(A_p.x-A_q.x) + fabsf(A_p.y-A_q.y)) + fabsf(A_p.z-A_q.z)))
 *   w = ((h[dy] * h[dx]) * g_max(0, 1 - d)) * g
 * and everything else as in rt_denoise (Vb, the sums, den, the variance update, skipped taps, bad
 * pixels).  The guides are the same at every level.  With kn = kz = ka = 0 no guide applies (g = 1 on
 * every tap, the hit / miss rule included) and the result is rt_denoise's bit for bit.
 * Each k is finite and >= 0, reserved 0 (RT_ERR_INVALID_ARG otherwise); NULL = the defaults below,
 * the setting that tools/denoise_quality.py's grid found best on scene 0 among those no worse than
 * the unguided filter on scenes 8, 6 and 2 (profiles/denoise_guided_quality.json). */
#define RT_GUIDE_DEFAULT_KN 0.5f
#define RT_GUIDE_DEFAULT_KZ 1.0f
#define RT_GUIDE_DEFAULT_KA 1.0f
typedef struct rt_guide_params { float kn, kz, ka; int reserved[5]; /* must be 0 */ } rt_guide_params;
/* rt_denoise with the guides: its preconditions, plus feature buffers held (RT_ERR_STATE naming
 * rt_render_features otherwise).  The result is read with rt_read_denoised. */
int rt_denoise_guided(rt_ctx* ctx, const rt_denoise_params* params, const rt_guide_params* guides);
/* Host only: rt_denoise_host with the guides; normal_depth / albedo_id: W*H*4 floats each. */
int rt_denoise_guided_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles,
                           const float* normal_depth, const float* albedo_id, int width, int height,
                           const rt_denoise_params* params, const rt_guide_params* guides, float* rgba_out);

/* ---- Temporal reprojection: the accumulated image carried into the new view after a camera move ----
 * rt_set_camera restarts the running mean at frame 1.  rt_history_capture keeps what the old view had
 * learned -- per pixel (r, g, b, n), n the frames behind that mean, with the first-hit buffers and the
 * camera they were made with -- and rt_reproject, after the move, gathers it into the new view wherever
 * the new view's first hit is a surface the old view saw, and blends it with the new view's own few
 * frames by their counts.  It writes a buffer of its own, (r, g, b, n_out) per pixel: image, moments, tile
 * counts, features and the denoised buffer keep their bits, and a context that never calls these
 * allocates and runs nothing new.  Single-device contexts without rt_set_partition (RT_ERR_STATE).
 *
 * The history view's matrix.  With the history camera's c0 = pixel_delta_u, c1 = pixel_delta_v,
 * c2 = up_left - camera_pos, all in double (a x b = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x), a . b = (a.x*b.x + a.y*b.y) + a.z*b.z, no contraction):
 *   det = c0 . (c1 x c2);   rows of M: (c1 x c2) / det, (c2 x c0) / det, (c0 x c1) / det,
 * each entry rounded to f32 once.  det 0 or not finite: RT_ERR_INVALID_ARG.  M takes a point's offset
 * from the history camera to (a, b, c) with a / c, b / c its pixel coordinates in the history view.
 *
 * The definition.  All arithmetic below is f32 without contraction, using only + - * / fabsf floorf,
 * rt_glsl.h's g_max / g_min (g_min(a, b) = b < a ? b : a) and comparisons, so a float32 restatement matches
 * bit for bit.  pixel_base(cam, fx, fy).c = (up_left.c + pixel_delta_u.c * fx) + pixel_delta_v.c * fy
 * (rt_render_features' coord); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  finite(v): fabsf(v) <= FLT_MAX.
 * For the current pixel p = (x, y) of a W x H image: C = the image's rgb; n_c = (float) of its 8x8 tile's
 * frame count, taken as 0 when a component of C is not finite; (N, t) and (A, id) its first-hit words;
 * o, o_h the current and the history camera_pos.
 *   1. If p is a miss (id == RT_FEATURE_MISS) or not guide-good (rt_denoise_guided: N, t, A all finite),
 *      there is no reprojection.
 *   2. d = pixel_base(cam, (float)x, (float)y) - o;   P.c = o.c + d.c * t.
 *   3. w = P - o_h;   a = (M00*w.x + M01*w.y) + M02*w.z,  b and c likewise from rows 1 and 2.
 *      Reject unless c > 0.   fx = a / c, fy = b / c.   Reject unless fx > -1 && fx < (float)W &&
 *      fy > -1 && fy < (float)H (a NaN fails).   x0 = floorf(fx), ax = fx - x0;  y0, ay likewise.
 *   4. Four taps q = (x0 + i, y0 + j), j outer over {0, 1}, i inner over {0, 1}, each with weight
 *      u = (i ? ax : 1 - ax) * (j ? ay : 1 - ay).  A tap is accepted when q is inside the image, the
 *      history's n_h(q) > 0, q's history features are guide-good and a hit, its id word equals p's (the
 *      same primitive and box face), (N.x*Nh.x + N.y*Nh.y) + N.z*Nh.z >= cos_min, and, unless kz == 0,
 *        d_q = pixel_base(cam_h, (float)q.x, (float)q.y) - o_h,   t_exp = dot(w, d_q) / dot(d_q, d_q),
 *        fabsf(t_exp - t_h(q)) <= kz * t_exp.
 *      A skipped tap is read at the clamped position and leaves the sums untouched.  The sums start at
 *      +0:   sw = sw + u;   sc.c = sc.c + u * H(q).c  for c in r, g, b;   sn = sn + u * n_h(q).
 *   5. Reject unless sw > 0.   Hc.c = sc.c / sw;   n_hist = g_min(sn / sw, max_history).
 *   6. Output: rejected or not reprojected: (C, n_c);  else if n_c == 0: (Hc, n_hist);  else
 *      n_out = n_c + n_hist,  alpha = n_hist / n_out,  out.c = C.c + alpha * (Hc.c - C.c),  (out, n_out).
 * csrc/rt_reproject_math.h holds these operations once, for the kernel and for rt_reproject_host.
 * The primitives are convex, so a ray meets one at most once from outside: equal ids at p and q mean
 * the history sample lies on the surface p sees, and the id test is the disocclusion test.
 *
 * cos_min is in [-1, 1], kz >= 0 and finite (0 switches the depth test off), max_history > 0 and
 * finite, reserved 0 (RT_ERR_INVALID_ARG otherwise); NULL = the defaults below, the best setting of
 * tools/reproject_quality.py's grid on scene 6 after a sideways move (among equal ratios the strictest;
 * profiles/reproject_quality.json).  max_history bounds how long a view-dependent surface (metal, glass)
 * keeps showing what the old view saw in it: history is shaded for the old camera. */
#define RT_REPROJECT_DEFAULT_COS_MIN 0.9f
#define RT_REPROJECT_DEFAULT_KZ 0.1f
#define RT_REPROJECT_DEFAULT_MAX_HISTORY 64.0f
enum { RT_HISTORY_FROM_IMAGE = 0, RT_HISTORY_FROM_REPROJECTED = 1 };
typedef struct rt_reproject_params { float cos_min, kz, max_history; int reserved[5]; /* must be 0 */ } rt_reproject_params;

/* Keep the history: device-to-device copies on the context's stream into buffers the context owns
 * (48 bytes per pixel, allocated by the first call), and the current camera block with its M.
 * RT_HISTORY_FROM_IMAGE: (r, g, b, n) from the image, n = (float) of the pixel's tile frame count, 0 where
 * a component of rgb is not finite; needs an image, rt_set_moments(ctx, 1) with tile counts that are not
 * all 0 (a render from frame 1; a single tile whose count is 0 gives n = 0) and feature buffers held and
 * not stale (rt_render_features), RT_ERR_STATE naming what is lacking.  RT_HISTORY_FROM_REPROJECTED: the last
 * rt_reproject result's (r, g, b, n_out) with the current feature buffers -- history that survives a camera
 * that keeps moving with a frame or two per pose; RT_ERR_STATE if no result is held or the features
 * are stale.  RT_ERR_INVALID_ARG: another source, or a camera whose det is 0 or not finite.
 * The history is held until rt_resize, rt_destroy, or rt_upload_buffer / rt_upload_texture (the ids
 * no longer mean the same surfaces); it survives rt_set_camera, rt_set_params, rt_set_bvh_mode and
 * later renders. */
int rt_history_capture(rt_ctx* ctx, int source);
/* Queue the gather (one kernel) on the context's stream behind the queued renders.  Needs, RT_ERR_STATE
 * naming what is lacking otherwise: history held (rt_history_capture), the image's size equal to the
 * history's, rt_set_moments(ctx, 1), and feature buffers held and current for the current camera
 * (rt_render_features).  A tile whose count is 0 has n_c = 0.  The result is held until the next
 * rt_reproject, rt_resize or rt_destroy. */
int rt_reproject(rt_ctx* ctx, const rt_reproject_params* params);
/* rt_sync, then the result as W*H*4 floats (r, g, b, n_out); RT_ERR_STATE with no result held. */
int rt_read_reprojected(rt_ctx* ctx, float* rgbn);
/* Host only, no device: the same header's arithmetic over caller arrays.  history_rgbn, history_nd,
 * history_ai, image, normal_depth, albedo_id: W*H*4 floats each; the two 28-float camera blocks;
 * tile_frames: one count >= 0 per 8x8 tile of the current image, row-major, n_tiles = ceil(W/8) * ceil(H/8)
 * (RT_ERR_INVALID_ARG otherwise, and for bad params or a singular history camera). */
int rt_reproject_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                      const float history_camera[28], const float* image, const int32_t* tile_frames, int n_tiles,
                      const float* normal_depth, const float* albedo_id, const float camera[28], int width, int height,
                      const rt_reproject_params* params, float* rgbn_out);

/* ---- Sample variance carried through reprojection, and the preview filter over the moved view ------
 * After a move rt_reproject's result is an n-frame picture where the old view saw the surface and a 1- or
 * 2-frame picture elsewhere (disoccluded strips, the background, rejected taps).  With
 * rt_set_history_variance(ctx, 1) a per-sample variance s2 of y = (r + g) + b travels with the history
 * and with the result, and rt_denoise_reprojected runs rt_denoise's levels over the result.  A negative
 * s2 means "unknown"; every "known" test is written s2 >= 0, so a NaN is unknown.  Carrying the variance
 * of one sample, not of the mean, makes its blend a colour channel's: for out = (n_c C + n_h Hc) / n_out
 * the variance of out is (n_c s2_c + n_h s2_h) / n_out^2, so s2_out is the count-weighted mean of s2_c and
 * s2_h and the variance of the mean is s2_out / n_out.  All arithmetic is f32 without contraction, every
 * step one operation in the order written, with only + - * / fabsf sqrtf floorf g_max g_min and
 * comparisons.
 *
 *   history_s2(C, M2.w, count): n = (float)count, 0 where a component of C is not finite;
 *     n >= 2 and finite(M2.w): g_max(0, M2.w / (n - 1.0f));   otherwise -1.
 *   rt_history_capture keeps, beside (r, g, b, n), history_s2 of the image (RT_HISTORY_FROM_IMAGE) or a
 *   copy of the result's s2 (RT_HISTORY_FROM_REPROJECTED).
 *   rt_reproject, in step 4 with `use` the tap's acceptance and s = s2_h(q) read at the same clamped
 *   position:   kn = use && s >= 0;   ss = kn ? ss + u * s : ss;   sws = kn ? sws + u : sws   (both start
 *   at +0), and after the taps s2_hist = sws > 0 ? ss / sws : -1.   With s2_c = history_s2(C, M2.w(p),
 *   count), the result's s2 is: s2_c wherever step 6 gives (C, n_c);  s2_hist where n_c == 0;  otherwise
 *   s2_hist if !(s2_c >= 0), else s2_c if !(s2_hist >= 0), else s2_c + alpha * (s2_hist - s2_c) with step
 *   6's alpha.  The (r, g, b, n_out) word is rt_reproject's, bit for bit.
 *
 * Off is the default: history, kernels, buffers and launches are as described above and nothing new is
 * allocated.  Changing the value drops the history and the result (RT_ERR_STATE from their readers until
 * the next rt_history_capture / rt_reproject).  On, the history and the result hold 4 more bytes per pixel. */
int rt_set_history_variance(rt_ctx* ctx, int on);
/* rt_sync, then the result's s2 as W*H floats; RT_ERR_STATE when no result with variance is held. */
int rt_read_reprojected_variance(rt_ctx* ctx, float* s2);

/* rt_denoise_guided's levels over the reprojected view.  Level 0 at pixel p with R = (r, g, b, n) the
 * result word, s2 its variance and id the id word of the albedo_id buffer:
 *   bad (V = -1, passes through unchanged, never a tap): !(finite(y(R)) && n > 0);
 *   s2 >= 0 && finite(s2):  V_0 = s2 / n;
 *   otherwise the spatial estimate (the fallback for a pixel with no usable sample variance): taps
 *   (dy, dx) in {-2..2}^2 at spacing 1, row-major (dy outer), the centre included; a tap is accepted when it
 *   lies in the image, is not bad and its id word equals p's (two misses are equal); a skipped tap is read
 *   at the clamped position and leaves the sums untouched.  Pass 1:  cnt = cnt + 1.0f;  sy = sy + y(q);
 *   then m = sy / cnt.  Pass 2 over the same taps:  e = y(q) - m;  sd = sd + e * e.
 *   V_0 = +0 if cnt < 2, else (sd / (cnt - 1.0f)) / n.
 * C_0 = R's rgb; levels 0 .. levels-1 then run exactly as in rt_denoise / rt_denoise_guided over the current
 * feature buffers.  params and guides mean what they mean in rt_denoise_guided: NULL = the defaults, all-zero
 * strengths = the unguided filter.  There is no minimum frame count.  The spatial estimate understates the
 * variance at the border between fresh and well-sampled pixels (the well-sampled neighbours of one id pull
 * the spread down), which errs towards less blur.  The result is read with rt_read_denoised and held under
 * rt_denoise's rules; image, moments, counts, features, history and the reprojected result keep their bits.
 * RT_ERR_STATE naming what is lacking: no reprojected result with variance held, feature buffers not
 * current, feature buffers rendered again since that rt_reproject, a multi-device context or one under
 * rt_set_partition. */
int rt_denoise_reprojected(rt_ctx* ctx, const rt_denoise_params* params, const rt_guide_params* guides);

/* Host only, no device: history_s2 per pixel -> s2_out (W*H floats); image / m2 W*H*4 floats, tile_frames
 * one count >= 0 per 8x8 tile (RT_ERR_INVALID_ARG otherwise, as rt_reproject_host). */
int rt_history_variance_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles,
                             int width, int height, float* s2_out);
/* rt_reproject_host with the variance: history_s2 W*H floats, m2 the current view's W*H*4 moments;
 * rgbn_out is rt_reproject_host's bit for bit, s2_out W*H floats. */
int rt_reproject_variance_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                               const float* history_s2, const float history_camera[28], const float* image,
                               const float* m2, const int32_t* tile_frames, int n_tiles, const float* normal_depth,
                               const float* albedo_id, const float camera[28], int width, int height,
                               const rt_reproject_params* params, float* rgbn_out, float* s2_out);
/* rt_denoise_reprojected over caller arrays: rgbn, normal_depth, albedo_id W*H*4 floats, s2 W*H floats. */
int rt_denoise_reprojected_host(const float* rgbn, const float* s2, const float* normal_depth, const float* albedo_id,
                                int width, int height, const rt_denoise_params* params, const rt_guide_params* guides,
                                float* rgba_out);

/* ---- Misses reprojected by direction --------------------------------------------------------------------
 * rt_reproject's step 1 leaves a pixel whose centre ray hits nothing with its own one or two frames.  The
 * first-hit pass leaves the constant media out, so such a pixel is the background seen through whatever fog
 * the scene has: often the noisiest part of the picture.  With rt_set_reproject_misses(ctx, 1) a miss is
 * reprojected too, as the point at infinity along its ray.  The arithmetic is the definition's: f32, no
 * contraction, the same operation set.  For a pixel p that is guide-good and a miss (id == RT_FEATURE_MISS):
 *   2m. d as in step 2;  w = d.  No P is formed and t is not read.
 *   3.  Unchanged, applied to that w: a, b, c from M; reject unless c > 0; fx = a / c, fy = b / c; the same
 *       window test, floor and weights.
 *   4m. A tap q is accepted when it is inside the image, n_h(q) > 0, q's history features are guide-good and
 *       a miss, and the bits of its albedo word's x, y, z (the background the miss was rendered under) equal
 *       those of p's.  There is no cos_min and no kz test.  The sums, and rt_set_history_variance's, are step 4's.
 *   5, 6. Unchanged, the variance blend included.
 * A miss has no surface: what p sees along d is what the old view saw along the same direction, so the
 * background's bits are the miss's id test -- they reject history taken under another rt_set_params background
 * -- and "q is a miss" is its disocclusion test.  A hit pixel's word and s2 are bit for bit what they are with
 * the switch off: it never accepts a miss tap (its id differs), and a miss never accepts a hit tap.  What the
 * history holds beyond the background itself is radiance gathered for the old camera position (fog in-scatter:
 * the "known lag" of a view-dependent surface, bounded by max_history); the defocus disk is ignored, as in the
 * first-hit pass; at a silhouette a miss tap's history may hold some object colour from the frames' jitter.
 *
 * Off is the default: rt_reproject launches the kernels it launches without this call and gives the same
 * bits.  Changing the value drops the held result (RT_ERR_STATE from rt_present, rt_reach_tiles,
 * rt_denoise_reprojected, rt_read_reprojected and RT_HISTORY_FROM_REPROJECTED until the next rt_reproject) and
 * keeps the history, which is the same under both values.  It allocates nothing.  rt_render_moved's and
 * rt_render_moved_refined's rt_reproject steps obey it. */
int rt_set_reproject_misses(rt_ctx* ctx, int on);
/* Host only, no device: rt_reproject_host (history_s2, m2 and s2_out all NULL) or rt_reproject_variance_host
 * (all three given; any other mix is RT_ERR_INVALID_ARG) with the misses reprojected by direction. */
int rt_reproject_misses_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                             const float* history_s2, const float history_camera[28], const float* image,
                             const float* m2, const int32_t* tile_frames, int n_tiles, const float* normal_depth,
                             const float* albedo_id, const float camera[28], int width, int height,
                             const rt_reproject_params* params, float* rgbn_out, float* s2_out);

/* ---- The presented frame: compose, expose and tonemap on the device ----------------------------------
 * The display path of the reference (Texture.saveAsPNG: float -> unorm8 -> gamma table, what
 * rts_tonemap_rgb8 does on the host) as one kernel over a buffer the context holds, so a preview leaves the
 * device as 4 bytes per pixel.  RT_PRESENT_MOVED also composes the picture recommended after a camera move:
 * the filtered buffer where the reprojected view's count did not grow, the reprojected view elsewhere.
 * It writes buffers of its own: image, moments, counts, features, history, the reprojected result and the
 * denoised buffer keep their bits, and a context that never calls these allocates and runs nothing new.
 * Single-device contexts without rt_set_partition (RT_ERR_STATE).
 *
 * The definition.  All arithmetic is f32 without contraction: one multiplication per channel, rintf (round
 * half to even) and comparisons, so a float32 restatement matches bit for bit.  For the pixel p of a W x H
 * image: cnt = the frame count of p's 8x8 tile, n_t = (float)cnt; R = the reprojected word (r, g, b, n_out);
 * D = the denoised buffer (rt_read_denoised's).
 *   1. Colour.  RT_PRESENT_IMAGE, RT_PRESENT_DENOISED, RT_PRESENT_REPROJECTED: c = that buffer's rgb, w = 1.
 *      RT_PRESENT_MOVED: fresh = !(R.w > n_t) (a NaN count is fresh);  c = fresh ? D.rgb : R.rgb;
 *      w = fresh ? 1 : 0.  (A bad pixel passes through the filter unchanged, so D is R there.)
 *   2. Exposure.  e.c = c.c * exposure for c in r, g, b.  (1.0f keeps every finite value's bits and a NaN a NaN.)
 *   3. Code.  code(f) = 0 if !(f > 0);  255 if f >= 1;  otherwise (int)rintf(f * 255.0f).
 *   4. Packing.  byte(f) = lut[code(f)], lut the 256-entry gamma table of Texture.saveAsPNG
 *      (lut[b] = (byte)((float)pow(b / 255.0, 1 / 2.2) * 255.0f), built on the host, never on the device);
 *      the pixel's word is byte(e.r) | byte(e.g) << 8 | byte(e.b) << 16 | 0xFFu << 24: in memory r, g, b, 255.
 *   5. Float copy.  With keep_float, (e.r, e.g, e.b, w) is written as well.
 * csrc/rt_present_math.h holds these operations once, for the kernel and for rt_present_host;
 * host/rt_gamma_lut.h holds the table once, for them and for rts_tonemap_rgb8, whose bytes the r, g, b of
 * RT_PRESENT_IMAGE at exposure 1 equal.
 *
 * source is one of the four values, exposure > 0 and finite, reserved 0 (RT_ERR_INVALID_ARG otherwise);
 * NULL = RT_PRESENT_IMAGE, exposure 1, no float copy. */
enum { RT_PRESENT_IMAGE = 0, RT_PRESENT_DENOISED = 1, RT_PRESENT_REPROJECTED = 2, RT_PRESENT_MOVED = 3 };
typedef struct rt_present_params { int source; float exposure; int keep_float; int reserved[5]; /* must be 0 */ } rt_present_params;

/* Queue the kernel on the context's stream behind what is queued.  RT_ERR_STATE naming what is lacking:
 * no image (RT_PRESENT_IMAGE); no filtered image held (RT_PRESENT_DENOISED); no reprojected result held
 * (RT_PRESENT_REPROJECTED, RT_PRESENT_MOVED); for RT_PRESENT_MOVED also rt_set_moments off (the tile counts),
 * or a denoised buffer that rt_denoise_reprojected did not write from the result now held (none, one that
 * rt_denoise / rt_denoise_guided wrote since, or a result that rt_reproject replaced since).  The counts are
 * the current ones, as rt_reproject reads them.  The frame (4 bytes per pixel, with keep_float 16 more; both
 * allocated by the first call that needs them, with 256 bytes for the table) is held until the next
 * rt_present, rt_resize or rt_destroy. */
int rt_present(rt_ctx* ctx, const rt_present_params* params);
/* rt_sync, then the frame as W*H*4 bytes (r, g, b, 255); RT_ERR_STATE with no frame held. */
int rt_read_presented(rt_ctx* ctx, uint8_t* rgba8);
/* rt_sync, then the float copy as W*H*4 floats (e.r, e.g, e.b, w); RT_ERR_STATE unless the frame held was
 * made with keep_float. */
int rt_read_presented_float(rt_ctx* ctx, float* rgbw);
/* As rt_bind_device_image, for the frame: later rt_present calls write it into caller-owned device memory of
 * at least W*H*4 bytes, 4-byte aligned (RT_ERR_INVALID_ARG otherwise), on the context's stream (rt_set_stream:
 * a torch uint8 tensor of shape (H, W, 4) receives the frame on torch's current stream).  NULL returns to the
 * internal buffer.  Either way no frame is held until the next rt_present; rt_resize lets the buffer go. */
int rt_bind_device_present(rt_ctx* ctx, void* device_ptr, size_t nbytes);
/* Host only, no device: the same header's arithmetic over caller arrays.  image, denoised, reprojected: W*H*4
 * floats each, needed as the source reads them (RT_PRESENT_MOVED: reprojected, denoised and tile_frames, one
 * count >= 0 per 8x8 tile, row-major, n_tiles = ceil(W/8) * ceil(H/8)); the others may be NULL.  rgba8_out:
 * W*H*4 bytes; rgbw_out: W*H*4 floats, written and needed with keep_float alone.  RT_ERR_INVALID_ARG for
 * anything else, and for bad params. */
int rt_present_host(const float* image, const float* denoised, const float* reprojected, const int32_t* tile_frames,
                    int n_tiles, int width, int height, const rt_present_params* params, uint8_t* rgba8_out,
                    float* rgbw_out);

/* One call per pose of a moving camera.  It is this sequence of the calls above and nothing else, queued with
 * no rt_sync between the steps, each step's refusal returned unchanged:
 *   1. rt_history_capture: RT_HISTORY_FROM_REPROJECTED if a result is held for the pose being left (made from
 *      the feature buffers now held, and those current), else RT_HISTORY_FROM_IMAGE, which needs what that
 *      call needs: current features and tile counts that are not all 0;
 *   2. rt_set_camera(camera);   3. rt_render(1, n_frames, rand_factors);   4. rt_render_features;
 *   5. rt_reproject(reproject);
 *   6. rt_denoise_reprojected(denoise, guides), under rt_set_history_variance(ctx, 1) alone;
 *   7. rt_present(present); a NULL present is exposure 1, no float copy and RT_PRESENT_MOVED under
 *      rt_set_history_variance(ctx, 1), RT_PRESENT_REPROJECTED without it.  RT_PRESENT_MOVED without the
 *      variance is rt_present's RT_ERR_STATE: no rt_denoise_reprojected wrote the denoised buffer. */
int rt_render_moved(rt_ctx* ctx, const float camera[28], int n_frames, const float* rand_factors,
                    const rt_reproject_params* reproject, const rt_denoise_params* denoise,
                    const rt_guide_params* guides, const rt_present_params* present);

/* ---- After a move: extra frames on the tiles the history does not reach ------------------------------
 * Where the old view saw the surface a pixel of the reprojected view holds n_hist + n frames, and one more
 * adds next to nothing; a disoccluded strip, a rejected tap or the leading edge holds the pose's own n,
 * usually 1.  rt_reach_tiles reduces the reprojected result's count n_out to one record per 8x8 tile on the
 * device, rt_refine_select chooses tiles from the records on the host, and rt_render_moved_refined spends
 * extra frames on the chosen tiles inside the one call per pose, reading back 16 bytes per tile.  The records
 * are a buffer of their own (allocated by the first rt_reach_tiles; a context that never calls these
 * allocates and runs nothing new): image, moments, counts, features, history, the reprojected result, the
 * denoised buffer and the presented frame keep their bits.  Single-device contexts without
 * rt_set_partition (RT_ERR_STATE).
 *
 * The record.  One per 8x8 tile of the image, tiles row-major, ceil(W/8) per row (the tiles of
 * rt_read_tile_sums), made from the held rt_reproject result R = (r, g, b, n_out) and a threshold min_count.
 * All arithmetic is f32 without contraction, using only +, comparisons, fabsf and rt_glsl.h's g_min
 * (g_min(a, b) = b < a ? b : a), so a float32 restatement matches bit for bit.  Lane ty*8+tx holds the pixel
 * (tile_x*8+tx, tile_y*8+ty); `in` is true when that pixel lies in the image.  With n = R.w:
 *   good  = in && n > 0 && fabsf(n) <= FLT_MAX        (a NaN is not good);
 *   short = in && !(n >= min_count)                   (a NaN and a count of 0 are short);
 *   v_min = good ? n : +inf;   v_sum = good ? n : +0;
 *   for off = 32, 16, 8, 4, 2, 1 (every lane at once, x[lane ^ off] its partner's value before the step):
 *     v_sum = v_sum + v_sum[lane ^ off];   v_min = g_min(v_min, v_min[lane ^ off]);
 *   n_min = lane 0's v_min (+inf when the tile has no good pixel);   n_sum = lane 0's v_sum;
 *   short_px = the number of short lanes;   pixels = the number of lanes that are in.
 * csrc/rt_refine_math.h holds these operations once, for the kernel and for rt_tile_reach_host. */
typedef struct rt_tile_reach { float n_min, n_sum; uint32_t short_px, pixels; } rt_tile_reach;  /* 16 bytes */
/* min_count: 0 = automatic, (float)(n_frames + extra_frames), "short of what the refinement would give it";
 * otherwise > 0 and finite.  extra_frames >= 0 (0: no refinement).  min_pixels 1 .. 64, 0 means 1.
 * max_tiles 0 (no cap) or positive.  reserved 0.  RT_ERR_INVALID_ARG otherwise. */
typedef struct rt_refine_params { float min_count; int extra_frames, min_pixels, max_tiles; int reserved[4]; /* must be 0 */ } rt_refine_params;

/* Queue the kernel on the context's stream behind what is queued.  The record buffer is n_tiles * 16 bytes,
 * allocated by the first call.  RT_ERR_INVALID_ARG unless min_count > 0 and finite.  RT_ERR_STATE naming what
 * is lacking: no reprojected result held (rt_reproject first), a multi-device context or one under
 * rt_set_partition.  The records belong to the result they were made from: they are held until the next
 * rt_reach_tiles, rt_reproject, rt_resize or rt_destroy. */
int rt_reach_tiles(rt_ctx* ctx, float min_count);
/* rt_sync, then the records.  out may be NULL to query *n_tiles; RT_ERR_LIMIT if cap is short;
 * RT_ERR_STATE with no records held. */
int rt_read_tile_reach(rt_ctx* ctx, rt_tile_reach* out, int cap, int* n_tiles);
/* Host only, no device: the same header's arithmetic over a caller array.  rgbn: W*H*4 floats (r, g, b, n_out),
 * as rt_read_reprojected gives them; n_tiles = ceil(W/8) * ceil(H/8) and min_count > 0 and finite
 * (RT_ERR_INVALID_ARG otherwise). */
int rt_tile_reach_host(const float* rgbn, int width, int height, float min_count, rt_tile_reach* out, int n_tiles);
/* Host only, pure.  A tile is a candidate when short_px >= min_pixels, min_pixels in 1 .. 64.  max_tiles 0: every
 * candidate is active.  max_tiles > 0: t is the smallest value in min_pixels .. 65 for which at most max_tiles
 * tiles have short_px >= t, and exactly those tiles are active.  Tiles with equal short_px stay or go together
 * -- a tile's index never decides -- so fewer than max_tiles may be active, and none when more than max_tiles
 * tiles share the largest count.  In particular, after a move that leaves every tile entirely fresh (all 64)
 * a cap below the tile count selects none: when the whole view is new there is nothing to favour, and the
 * pose's own n_frames are all it gets.  RT_ERR_INVALID_ARG: min_pixels outside 1 .. 64, max_tiles < 0, a
 * short_px over 64, NULL tiles or active_out with n_tiles > 0.  n_active may be NULL. */
int rt_refine_select(const rt_tile_reach* tiles, int n_tiles, int min_pixels, int max_tiles, uint8_t* active_out,
                     int* n_active);
/* rt_render_moved with extra frames where the history does not reach.  With refine NULL or extra_frames 0 it is
 * rt_render_moved exactly.  Otherwise it is this sequence of the public calls and nothing else, each step's
 * refusal returned unchanged:
 *   rt_render_moved's steps 1 - 5 (capture, camera, rt_render(1, n_frames, rand_factors), features, reproject);
 *   a. rt_reach_tiles(mc), mc = refine->min_count if that is > 0, else (float)(n_frames + extra_frames);
 *   b. rt_read_tile_reach -- the call's one rt_sync;
 *   c. rt_refine_select(min_pixels, max_tiles);
 *   d. if any tile is active: rt_set_active_tiles(mask) (NULL when every tile is active),
 *      rt_render(n_frames + 1, extra_frames, rand_factors + n_frames), rt_set_active_tiles(NULL, 0), and
 *      rt_reproject(reproject) again over the same history (rt_render leaves the feature buffers current);
 *   rt_render_moved's steps 6 and 7 (rt_denoise_reprojected, rt_present), over the second result.
 * A refined tile holds, in image and moments, the bits of a plain (n_frames + extra_frames)-frame render and
 * its count says so; rt_present's fresh test reads that count, so a refined pixel the history does not reach
 * still takes the filtered buffer.  rand_factors holds n_frames + extra_frames values.  *tiles_refined
 * (may be NULL) receives the number of tiles refined.  RT_ERR_STATE if a caller mask is set on entry (as
 * rt_render_adaptive); no mask is left set, also when a step refuses.  RT_ERR_INVALID_ARG for bad refine
 * params (rt_refine_params above). */
int rt_render_moved_refined(rt_ctx* ctx, const float camera[28], int n_frames, const float* rand_factors,
                            const rt_refine_params* refine, const rt_reproject_params* reproject,
                            const rt_denoise_params* denoise, const rt_guide_params* guides,
                            const rt_present_params* present, int* tiles_refined);

/* ---- After a move: render until the moved view meets a noise target, tile by tile -----------------------
 * The count criterion above sends frames to every fresh pixel alike.  With rt_set_history_variance(ctx, 1) the
 * reprojected result carries a per-sample variance s2 of y, so the variance of a pixel's mean, s2 / n_out, is
 * known wherever two or more samples stand behind the pixel.  rt_noise_tiles reduces it to one record per 8x8
 * tile on the device, rt_refine_noise_select applies rt_adaptive_select's rule to the records on the host, and
 * rt_render_moved_to_noise renders masked batches until every tile meets the target or a round cap, reading
 * back 16 bytes per tile and round.  The records are a buffer of their own (allocated by the first
 * rt_noise_tiles; a context that never calls these allocates and runs nothing new): image, moments, counts,
 * features, history, the reprojected result and its s2, the denoised buffer, the presented frame and the reach
 * records keep their bits.  Single-device contexts without rt_set_partition (RT_ERR_STATE).
 *
 * The record.  One per 8x8 tile of the image, tiles row-major, ceil(W/8) per row (the tiles of
 * rt_read_tile_sums), made from the held rt_reproject result R = (r, g, b, n), its variance word s2
 * (rt_read_reprojected_variance's) and a threshold min_count.  All arithmetic is f32 without contraction, using
 * only +, /, comparisons and fabsf, so a float32 restatement matches bit for bit.  Lane ty*8+tx holds the pixel
 * (tile_x*8+tx, tile_y*8+ty); `in` is true when that pixel lies in the image; finite(x) is fabsf(x) <= FLT_MAX.
 *   y     = (R.r + R.g) + R.b;
 *   good  = in && finite(y) && n > 0 && finite(n)     (the complement of rt_denoise_reprojected's "bad", plus a
 *                                                      finite count);
 *   known = good && s2 >= 0 && finite(s2)             (rt_reproject writes -1 where no variance is known);
 *   thin  = good && (!known || !(n >= min_count));
 *   v     = known ? s2 / n : +0                       (the variance of the pixel's mean);
 *   yv    = good ? y : +0;
 *   for off = 32, 16, 8, 4, 2, 1 (every lane at once, x[lane ^ off] its partner's value before the step):
 *     v = v + v[lane ^ off];   yv = yv + yv[lane ^ off];
 *   v_sum = lane 0's v;   y_sum = lane 0's yv;
 *   known_px = the number of known lanes;   thin_px = the number of thin lanes;
 *   bad_px = the number of lanes with in && !good;   pixels = the number of lanes that are in.
 * csrc/rt_refine_math.h holds these operations once, for the kernel and for rt_tile_noise_host. */
typedef struct rt_tile_noise { float v_sum, y_sum; uint16_t known_px, thin_px, bad_px, pixels; } rt_tile_noise; /* 16 bytes */
/* rt_refine_noise_select's figures over all tiles, and rt_render_moved_to_noise's rounds and outcome. */
typedef struct rt_moved_noise_stats { double sum_v, sum_y; uint64_t known, thin, bad, pixels; int rounds, converged; double noise; } rt_moved_noise_stats;
/* target_noise >= 0 and finite.  min_count: 0 = automatic, 2, the fewest frames from which the moments give an
 * estimate; otherwise > 0 and finite.  batch_frames >= 1: the frames an active tile gets per round.
 * max_rounds >= 0: the cap (0: a noise figure and no extra frames).  reserved 0.  RT_ERR_INVALID_ARG otherwise. */
typedef struct rt_noise_refine_params { float target_noise, min_count; int batch_frames, max_rounds; int reserved[4]; /* must be 0 */ } rt_noise_refine_params;

/* Queue the kernel on the context's stream behind what is queued.  The record buffer is n_tiles * 16 bytes,
 * allocated by the first call.  RT_ERR_INVALID_ARG unless min_count > 0 and finite.  RT_ERR_STATE naming what
 * is lacking: no reprojected result held (rt_reproject first), a result without variance
 * (rt_set_history_variance(ctx, 1) first), a multi-device context, one under rt_set_partition, no image.  The
 * records belong to the result they were made from: they are held until the next rt_noise_tiles, rt_reproject,
 * rt_resize or rt_destroy, or until rt_set_reproject_misses or rt_set_history_variance change value.  Reach
 * records and noise records are held side by side. */
int rt_noise_tiles(rt_ctx* ctx, float min_count);
/* rt_sync, then the records.  out may be NULL to query *n_tiles; RT_ERR_LIMIT if cap is short;
 * RT_ERR_STATE with no records held. */
int rt_read_tile_noise(rt_ctx* ctx, rt_tile_noise* out, int cap, int* n_tiles);
/* Host only, no device: the same header's arithmetic over caller arrays.  rgbn: W*H*4 floats (r, g, b, n), as
 * rt_read_reprojected gives them; s2: W*H floats, as rt_read_reprojected_variance gives them;
 * n_tiles = ceil(W/8) * ceil(H/8) and min_count > 0 and finite (RT_ERR_INVALID_ARG otherwise). */
int rt_tile_noise_host(const float* rgbn, const float* s2, int width, int height, float min_count, rt_tile_noise* out,
                       int n_tiles);
/* Host only, pure; rt_adaptive_select's rule over the noise records.  In double, tiles in index order, with
 * G_t = pixels_t - bad_px_t (the good pixels) and K_t = known_px_t:
 *   ybar = sum_t y_sum_t / sum_t G_t over ALL tiles (0 when no pixel is good);
 *   lim  = (double)target * ybar;
 *   v_t  = (double)v_sum_t / K_t;
 * a tile is active when active_in[t] is set (active_in NULL: all are), G_t > 0, and thin_px_t >= 1 or
 * (K_t > 0 and v_t > lim * lim).  An inactive tile stays inactive.  Thin pixels force activity for the reason
 * rt_adaptive_select has min_frames: a dark pixel whose samples are all zero so far has a variance estimate of
 * 0, which passes any limit, and a 1-frame fresh pixel has no estimate at all -- neither may stop its tile.
 * stats (may be NULL), with K = sum_t K_t: sum_v, sum_y, known, thin, bad, pixels are the plain sums over all
 * tiles; noise = sqrt(sum_v / K) / ybar, 0 when sum_v is 0 and K > 0, +inf when K is 0 or ybar alone is 0;
 * rounds and converged are left 0.  target >= 0 and finite.  RT_ERR_INVALID_ARG otherwise, and for NULL tiles
 * or active_out with n_tiles > 0, any count over 64, known_px + bad_px > pixels.  n_active may be NULL. */
int rt_refine_noise_select(const rt_tile_noise* tiles, const uint8_t* active_in, int n_tiles, float target,
                           uint8_t* active_out, int* n_active, rt_moved_noise_stats* stats);
/* rt_render_moved, then masked batches until every tile meets target_noise or max_rounds is reached.  With
 * refine NULL it is rt_render_moved exactly.  Otherwise it is this sequence of the public calls and nothing
 * else, each step's refusal returned unchanged:
 *   rt_render_moved's steps 1 - 5 (capture, camera, rt_render(1, n_frames, rand_factors), features, reproject);
 *   active = all tiles, r = 0, then:
 *   a. rt_noise_tiles(mc), mc = refine->min_count if that is > 0, else 2;
 *   b. rt_read_tile_noise -- the round's one rt_sync;
 *   c. rt_refine_noise_select(records, active, target_noise) -> active, n_active, stats;
 *   d. n_active == 0: converged = 1, stop;   r == max_rounds: converged = 0, stop;
 *   e. rt_set_active_tiles(mask) (NULL when every tile is active),
 *      rt_render(n_frames + r * batch_frames + 1, batch_frames, rand_factors + n_frames + r * batch_frames),
 *      rt_set_active_tiles(NULL, 0), rt_reproject(reproject) again over the same history;  r = r + 1;  back to a;
 *   rt_render_moved's steps 6 and 7 (rt_denoise_reprojected, rt_present), over the last result.
 * The active set only shrinks, so every active tile holds n_frames + r * batch_frames frames and each masked
 * launch continues its tiles' counts.  A tile that stopped after j rounds holds, in image and moments, the bits
 * of a plain (n_frames + j * batch_frames)-frame render, and its count says so: the tiles end with different
 * numbers of extra frames.  A pixel whose moments are not finite stays thin, so its tile runs to the round cap;
 * the cap is what bounds that tile.  rand_factors holds n_frames + batch_frames * max_rounds values.
 * Outputs (each may be NULL): *rounds_done = r; *tiles_refined = the tiles rendered in the first round;
 * *tile_frames_spent = the sum over the rounds of n_active * batch_frames; *last = the final stats, with rounds
 * and converged filled.  RT_ERR_STATE if a caller mask is set on entry (as rt_render_adaptive) or
 * rt_set_history_variance is off; no mask is left set, also when a step refuses.  RT_ERR_INVALID_ARG for bad
 * refine params (rt_noise_refine_params above) and when n_frames + batch_frames * max_rounds overflows. */
int rt_render_moved_to_noise(rt_ctx* ctx, const float camera[28], int n_frames, const float* rand_factors,
                             const rt_noise_refine_params* refine, const rt_reproject_params* reproject,
                             const rt_denoise_params* denoise, const rt_guide_params* guides,
                             const rt_present_params* present, int* rounds_done, int* tiles_refined,
                             int64_t* tile_frames_spent, rt_moved_noise_stats* last);

/* Per-frame u_rand_factor for frame index f (0-based) of a seeded render:
 * top 24 bits of splitmix64(seed, f) / 2^24, in [0,1).  Stands in for the
 * reference's (float)Math.random() per frame (RaytraceExecutor.java:124). */
float rt_frame_rand_factor(uint64_t seed, uint64_t frame_index);

#ifdef __cplusplus
}
#endif

#endif /* RT_H */
