/*
 * rt_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference's per-pixel kernel (compute.glsl +
 * utils/{hitting,scatter,pdf,random,texture,math,interval}.glsl) used as the parity checker for the HIP path and as the timed
 * CPU baseline in bench.py.  Only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load liboracle.so.  The product library
 * (librtamd.so) never links or calls it.
 *
 * Parity status: the reference (Java + OpenGL GLSL) cannot run anywhere in this
 * pipeline (no JDK, no GL, Windows-only natives), and it ships no
 * tests or golden vectors.  The oracle is therefore pinned only by (a) the
 * get_sphere_uv known-answer table in texture.glsl:100-102, (b) the std430
 * layout comments of RaytraceModel.java:139-219 vs compute.glsl structs, and
 * (c) statistical agreement with the reference gallery render of scene 6, and
 * (d) per operation (the oracle_eval_op entry points below) a float64 restatement of the shader
 * text within derived rounding bounds (tests/ref64.py, tests/test_ops_ref64.py), and (e) likewise the
 * operations that choose a path's next direction and weight (oracle_eval_shade_op: rand as a float32
 * composition, transform_onb, rand_unit_vec, the medium's tail, light pdf and direction, the camera ray and
 * the shading step; tests/ref64_shade.py, tests/test_shade_ref64.py), draw counts included;
 * and (f) the closest-hit walk that joins them (RT_SOP_TRACE below: trace_through_bvh itself; tests/ref64_trace.py,
 * tests/test_trace_ref64.py) and the path loop replayed over those entry points (tests/path_replay.py);
 * everything else is "parity unpinned" against the reference itself.
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oracle_scene_desc {
    const void* buf[6];          /* SSBO bytes, rt.h RT_BIND_* order */
    size_t nbytes[6];
    int tex_format[8];           /* rt.h RT_TEX_*, 0 = unbound */
    int tex_w[8], tex_h[8];
    const void* tex[8];
    float camera[28];            /* std140 Camera block */
    int max_depth;
    float background[3];
    float sqrt_spp, recip_sqrt_spp;
} oracle_scene_desc;

/* Logical record traffic of the reference kernel. */
typedef struct oracle_counters {
    uint64_t samples;
    uint64_t bounces;            /* ray_color loop iterations            */
    uint64_t node_visits;        /* bvh_nodes[...] loads (32 B)          */
    uint64_t sphere_tests, quad_tests, box_tests, medium_tests;
    uint64_t rand_calls;
    uint64_t framebuffer_bytes;  /* 32 per sample                        */
    uint64_t node_bytes;
    uint64_t prim_bytes;         /* primitive records read by hit tests  */
    uint64_t material_bytes;     /* set_material_properties re-reads     */
    uint64_t texel_bytes;
    uint64_t light_bytes;
} oracle_counters;

/* Render n_frames frames (frame_count = first_frame + i, u_rand_factor =
 * rand_factors[i]) into the full-size W x H RGBA32F image `rgba` (row 0 = top),
 * touching only rows r with (r / stripe_rows) % world == rank.
 * nthreads = 0 -> all hardware threads.  counters may be NULL. */
int oracle_render(const oracle_scene_desc* d, int width, int height, float* rgba,
                  int first_frame, int n_frames, const float* rand_factors,
                  int rank, int world, int stripe_rows, int nthreads,
                  oracle_counters* counters);

/* Pin oracle_render's threads: worker i to CPU cpus[i % n] (n = 0: unpinned, the
 * default).  Used by bench.py's CPU baseline only. */
void oracle_set_thread_cpus(const int* cpus, int n);

/* Analysis hook: per-trace BVH node sequences for a pixel window
 * (records [pixel, frame, bounce, n, node...]); returns int32 count. */
long oracle_trace_log(const oracle_scene_desc* d, int width, int height, int x0, int x1, int y0, int y1,
                      int first_frame, int n_frames, const float* rand_factors, int32_t* out, long cap);

/* Known-answer hooks. */
void oracle_get_sphere_uv(float x, float y, float z, float* u, float* v);
/* n successive rand() values for an invocation at (px,py) with u_rand_factor f */
void oracle_rand_sequence(float px, float py, float f, int n, float* out);
/* GLSL built-ins as defined in include/rt/rt_glsl.h: fn 0 sin, 1 cos, 2 log,
 * 3 acos, 4 atan2(x, y2), 5 fract, 6 sqrt */
void oracle_eval_builtin(int fn, const float* x, const float* y2, float* out, int n);
/* Perlin noise_turb / perlin_noise_color for a 6x256 R32F table */
float oracle_perlin_turb(const float* table, float px, float py, float pz, int depth);
/* ray-primitive KATs: return 1 on hit and fill t / p / normal / front */
int oracle_hit_sphere(const void* sphere48, float time, const float o[3], const float dir[3],
                      float tmin, float tmax, float* t, float p[3], float n[3], int* front);
int oracle_hit_quad(const void* quad80, const float o[3], const float dir[3],
                    float tmin, float tmax, float* t, float p[3], float n[3], int* front);
int oracle_hit_aabb(const float box6[6], const float o[3], const float dir[3], float tmin, float tmax);
/* hit_box (hitting.glsl:135-146) on 6 rt_quad: t, the side whose hit the record holds, hit_record.uv */
int oracle_hit_box(const void* box480, const float o[3], const float dir[3], float tmin, float tmax, float* t,
                   int* face, float uv[2]);
/* hit_constant_medium's two boundary hits (hitting.glsl:163-169) on a sphere boundary, before any rand():
 * returns 1 when both hit and fills rec1.t, rec2.t */
int oracle_medium_boundary_hits(const void* sphere48, float time, const float o[3], const float dir[3], float* t1,
                                float* t2);
/* texture2D with GL_LINEAR + CLAMP_TO_EDGE on a texture of rt_types.h format RT_TEX_* */
void oracle_texture_bilinear(int format, int w, int h, const void* texels, float u, float v, float rgb[3]);
/* checkerboard()'s parity (texture.glsl:10-11): 0 even (the first colour), 1 odd */
int oracle_checker_parity(float scale, float px, float py, float pz);
/* The per-operation hooks over n rows in rt_debug_eval_op's layout (include/rt/rt_debug.h: its op
 * numbers, rows of 12 floats, 8 output words per row, recs as the uploads carry them; op 7 runs
 * texture_color on slot 0).  Returns 0, or -1 for an unknown op or a Perlin table of another shape. */
int oracle_eval_op(int op, const void* recs, const float* rows, int n, int tex_format, int tex_w, int tex_h,
                   const void* tex, uint32_t* out);
/* The operations that decide where a path goes next and what it carries, over n rows in
 * rt_debug_eval_shade_op's layout (include/rt/rt_debug.h: its op numbers RT_SOP_*, rows of 20 floats, 12
 * output words per row) on scene d: rand, transform_onb, rand_unit_vec, the tail of hit_constant_medium
 * after its two boundary hits (medium_tail), lights_pdf_value, lights_random, main()'s time = rand() with
 * get_ray(), and the body of ray_color's loop after a trace that hit (shade_step, on the hit record and
 * material globals that hit leaves), and ray_color's walk (trace_through_bvh, below).  ray_color and
 * hit_constant_medium call the same medium_tail and shade_step.  Returns 0, or -1 for an unknown op or a shade row that names no record of the scene. */
int oracle_eval_shade_op(const oracle_scene_desc* d, int op, const float* rows, int n, uint32_t* out);
/* RT_SOP_TRACE (op 8) runs the trace_through_bvh that ray_color runs, over ray_t = [0.001, RT_INFINITY], on the
 * row's o, d, time, px, py, rf and the uv source it had before the walk (row words 15..18).  Out words:
 *   0 hit   1 t   2 tif (type | box face << 4 | index << 16; t and tif 0 on a miss)
 *   3..6 the uv source after the walk (kind_idx, a, b, c) as rt_debug.h's UvSrc carries hit_record.uv: the
 *        walk's last accepted sphere hit (1 << 16 | index, its rec.p) or quad / box side hit (2 << 16,
 *        alpha, beta, c as it was), the input's when the walk accepted neither
 *   7 rf after   8 nodes visited (popped)   9 leaf slots tested (hit_model calls)
 *   10 the visited node indices' hash, in visit order: h = ORACLE_VISIT_HASH_INIT, then per node
 *      h = ORACLE_VISIT_HASH_STEP(h, index) (FNV-1a over 32-bit words, modulo 2^32) */
#define ORACLE_VISIT_HASH_INIT 2166136261u
#define ORACLE_VISIT_HASH_STEP(h, node) ((((uint32_t)(h)) ^ ((uint32_t)(node))) * 16777619u)

#ifdef __cplusplus
}
#endif

#endif
