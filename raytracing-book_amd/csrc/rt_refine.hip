// rt_refine.hip — where a moved view's history does not reach (rt.h rt_reach_tiles / rt_read_tile_reach) and the
// one call per pose that spends extra frames there (rt_render_moved_refined).  Nothing here touches the render
// kernels, the image, the moments, the counts, the features, the history, the reprojected result, the filter's
// buffers or the presented frame: the records are a buffer of their own, allocated by the first rt_reach_tiles.
//
// reach_kernel: tile_sums_kernel's shape.  One wave per 8x8 tile (row-major tiles), lane ty * 8 + tx its pixel,
// four tiles per 256-thread workgroup, lanes outside the image idle but present in the shuffles; no LDS, no
// atomics.  A lane loads the one dword it needs, the count n_out in the .w of its pixel's reprojected word
// (written as a float4 load with .w taken, the compiler emits the same global_load_dword: DESIGN.md §4).  A xor butterfly
// (32, 16, 8, 4, 2, 1) leaves the tile's sum and minimum in every lane, two ballots count the short pixels
// and the pixels, and lane 0 stores the record as one 16-byte store.  The arithmetic is rt_refine_math.h's,
// shared with rt_tile_reach_host, which the records equal bit for bit.
//
// The noise records (rt.h rt_noise_tiles / rt_read_tile_noise) and the pose rendered to a noise target
// (rt_render_moved_to_noise) follow the same plan: noise_tiles_kernel below, a buffer of its own allocated by the
// first rt_noise_tiles, the arithmetic shared with rt_tile_noise_host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "rt/rt.h"
#include "rt_ctx.h"
#include "rt_refine.h"
#include "rt_refine_math.h"

namespace {

static_assert(sizeof(rt_tile_reach) == 16, "a reach record is one 16-byte store");

constexpr int kTilesPerBlock = 4;   // 256 threads: four waves, one 8x8 tile each

// rgbn: the reprojected result as floats, four per pixel
__global__ void __launch_bounds__(256) reach_kernel(const float* __restrict__ rgbn, int W, int H, int n_tiles,
                                                    float min_count, rt_tile_reach* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * kTilesPerBlock + ((int)threadIdx.x >> 6);   // wave-uniform
    if (tile >= n_tiles) return;
    const int tiles_x = (W + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 8 + (lane >> 3);
    const bool in = x < W && y < H;
    float n = 0.0f;
    if (in) n = rgbn[((size_t)y * W + x) * 4 + 3];
    const rf_lane l = rf_lane_of(in, n, min_count);
    float v_min = l.v_min, v_sum = l.v_sum;
    const unsigned long long in_mask = __ballot(in), short_mask = __ballot(l.is_short);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v_sum = rf_sum_step(v_sum, __shfl_xor(v_sum, off, 64));
        v_min = rf_min_step(v_min, __shfl_xor(v_min, off, 64));
    }
    if (lane == 0) {
        float4 rec;
        rec.x = v_min;
        rec.y = v_sum;
        rec.z = __uint_as_float((uint32_t)__popcll(short_mask));
        rec.w = __uint_as_float((uint32_t)__popcll(in_mask));
        *reinterpret_cast<float4*>(out + tile) = rec;
    }
}

static_assert(sizeof(rt_tile_noise) == 16, "a noise record is one 16-byte store");

// noise_tiles_kernel: reach_kernel's shape -- one wave per 8x8 tile, four tiles per 256-thread workgroup, lanes
// outside the image idle but present in the shuffles; no LDS, no atomics.  A lane loads its pixel's whole
// reprojected word (one 16-byte load: a wave touches eight 128-byte row segments) and its s2 (one dword: eight
// 32-byte segments).  Two f32 butterflies in the fixed order, four ballots for the counts, and lane 0 stores the
// record as one 16-byte store, the four 16-bit counts packed into two dwords.
__global__ void __launch_bounds__(256) noise_tiles_kernel(const float4* __restrict__ rgbn, const float* __restrict__ s2,
                                                          int W, int H, int n_tiles, float min_count,
                                                          rt_tile_noise* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * kTilesPerBlock + ((int)threadIdx.x >> 6);   // wave-uniform
    if (tile >= n_tiles) return;
    const int tiles_x = (W + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 8 + (lane >> 3);
    const bool in = x < W && y < H;
    float4 R = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float s = 0.0f;
    if (in) {
        const size_t p = (size_t)y * W + x;
        R = rgbn[p];
        s = s2[p];
    }
    const rf_noise_lane l = rf_noise_lane_of(in, R.x, R.y, R.z, R.w, s, min_count);
    float v = l.v, yv = l.yv;
    const unsigned long long in_mask = __ballot(in), known_mask = __ballot(l.known), thin_mask = __ballot(l.thin),
                             bad_mask = __ballot(l.bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v = rf_sum_step(v, __shfl_xor(v, off, 64));
        yv = rf_sum_step(yv, __shfl_xor(yv, off, 64));
    }
    if (lane == 0) {
        float4 rec;
        rec.x = v;
        rec.y = yv;
        rec.z = __uint_as_float((uint32_t)__popcll(known_mask) | ((uint32_t)__popcll(thin_mask) << 16));   // known_px, thin_px
        rec.w = __uint_as_float((uint32_t)__popcll(bad_mask) | ((uint32_t)__popcll(in_mask) << 16));       // bad_px, pixels
        *reinterpret_cast<float4*>(out + tile) = rec;
    }
}

}  // namespace

namespace rt_impl {

void refine_free(rt_ctx* c) {
    for (Device& d : c->devs) {
        dev_free(d.rf_tiles);
        dev_free(d.nz_tiles);
    }
    c->rf_rp_gen = 0;
    c->nz_rp_gen = 0;
}

}  // namespace rt_impl

using namespace rt_impl;

namespace {

// what both calls need of the context; `what` names the call in the message
int refine_ready(rt_ctx* c, const char* what) {
    const std::string w(what);
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, w + " needs a 1-device context");
    if (c->proc_world > 1) return set_err(c, RT_ERR_STATE, w + ": not under rt_set_partition");
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, w + ": no image (rt_resize first)");
    return RT_OK;
}

int tiles_of(const rt_ctx* c) { return ((c->width + 7) / 8) * ((c->devs[0].local_rows + 7) / 8); }

// records held, and made from the reprojected result now held
bool reach_held(const rt_ctx* c) {
    return c->devs.size() == 1 && c->rp_valid && c->rf_rp_gen != 0 && c->rf_rp_gen == c->rp_gen && c->devs[0].rf_tiles.ptr;
}

bool noise_held(const rt_ctx* c) {
    return c->devs.size() == 1 && c->rp_valid && c->nz_rp_gen != 0 && c->nz_rp_gen == c->rp_gen && c->devs[0].nz_tiles.ptr;
}

}  // namespace

extern "C" {

int rt_reach_tiles(rt_ctx* c, float min_count) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!rf_min_count_ok(min_count)) return set_err(c, RT_ERR_INVALID_ARG, "rt_reach_tiles: min_count > 0 and finite");
    int r = refine_ready(c, "rt_reach_tiles");
    if (r) return r;
    Device& d = c->devs[0];
    if (!c->rp_valid || !d.rp_out.ptr)
        return set_err(c, RT_ERR_STATE, "rt_reach_tiles: no reprojected result held (rt_reproject first)");
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows, nt = tiles_of(c);
    c->rf_rp_gen = 0;
    if ((r = ensure(c, d, d.rf_tiles, (size_t)nt * sizeof(rt_tile_reach)))) return r;
    hipLaunchKernelGGL(reach_kernel, dim3((unsigned)((nt + kTilesPerBlock - 1) / kTilesPerBlock)), dim3(256), 0, d.stream,
                       (const float*)d.rp_out.ptr, W, H, nt, min_count, (rt_tile_reach*)d.rf_tiles.ptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string("rt_reach_tiles launch failed: ") + hipGetErrorString(e));
    c->rf_rp_gen = c->rp_gen;
    return RT_OK;
}

int rt_read_tile_reach(rt_ctx* c, rt_tile_reach* out, int cap, int* n_tiles) {
    if (!c || !n_tiles) return RT_ERR_INVALID_ARG;
    int r = refine_ready(c, "rt_read_tile_reach");
    if (r) return r;
    if (!reach_held(c))
        return set_err(c, RT_ERR_STATE,
                       "rt_read_tile_reach: no reach records held for the reprojected result (rt_reach_tiles first)");
    const int nt = tiles_of(c);
    *n_tiles = nt;
    if (!out) return RT_OK;
    if (cap < nt) return set_err(c, RT_ERR_LIMIT, "rt_read_tile_reach: out is too small");
    if ((r = rt_sync(c))) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, out, d.rf_tiles.ptr, (size_t)nt * sizeof(rt_tile_reach));
}

int rt_render_moved_refined(rt_ctx* c, const float camera[28], int n_frames, const float* rand_factors,
                            const rt_refine_params* refine, const rt_reproject_params* reproject,
                            const rt_denoise_params* denoise, const rt_guide_params* guides,
                            const rt_present_params* present, int* tiles_refined) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (tiles_refined) *tiles_refined = 0;
    rt_rf_resolved prm;
    if (refine_resolve(refine, &prm))
        return set_err(c, RT_ERR_INVALID_ARG,
                       "rt_render_moved_refined: extra_frames >= 0, min_pixels 0 .. 64, max_tiles >= 0, min_count >= 0 and "
                       "finite, reserved 0");
    if (prm.extra_frames == 0) return rt_render_moved(c, camera, n_frames, rand_factors, reproject, denoise, guides, present);
    int r = refine_ready(c, "rt_render_moved_refined");
    if (r) return r;
    if (c->mask_set)
        return set_err(c, RT_ERR_STATE, "rt_render_moved_refined: a tile mask is set (rt_set_active_tiles(ctx, NULL, 0))");
    if (n_frames > INT32_MAX - prm.extra_frames)
        return set_err(c, RT_ERR_INVALID_ARG, "rt_render_moved_refined: n_frames + extra_frames overflows");
    if ((r = moved_to_reprojected(c, camera, n_frames, rand_factors, reproject))) return r;
    // "short of what the refinement would give it", unless the caller names a count
    const float mc = prm.min_count > 0.0f ? prm.min_count : (float)(n_frames + prm.extra_frames);
    if ((r = rt_reach_tiles(c, mc))) return r;
    const int nt = tiles_of(c);
    std::vector<rt_tile_reach> reach((size_t)nt);
    std::vector<uint8_t> active((size_t)nt, 0);
    int m = 0, n_active = 0;
    if ((r = rt_read_tile_reach(c, reach.data(), nt, &m))) return r;   // the call's one rt_sync
    if ((r = rt_refine_select(reach.data(), nt, prm.min_pixels, prm.max_tiles, active.data(), &n_active)))
        return set_err(c, r, "rt_render_moved_refined: rt_refine_select refused the records");
    if (n_active > 0) {
        // (every tile active: the plain launch, the same bits)
        r = n_active == nt ? rt_set_active_tiles(c, nullptr, 0) : rt_set_active_tiles(c, active.data(), nt);
        if (!r) r = rt_render(c, n_frames + 1, prm.extra_frames, rand_factors + n_frames);
        const int r2 = rt_set_active_tiles(c, nullptr, 0);   // no mask is left set
        if (r) return r;
        if (r2) return r2;
        if ((r = rt_reproject(c, reproject))) return r;   // over the same history; rp_gen moves on
    }
    if (tiles_refined) *tiles_refined = n_active;
    return moved_filter_present(c, denoise, guides, present);
}

int rt_noise_tiles(rt_ctx* c, float min_count) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!rf_min_count_ok(min_count)) return set_err(c, RT_ERR_INVALID_ARG, "rt_noise_tiles: min_count > 0 and finite");
    int r = refine_ready(c, "rt_noise_tiles");
    if (r) return r;
    Device& d = c->devs[0];
    if (!c->rp_valid || !d.rp_out.ptr)
        return set_err(c, RT_ERR_STATE, "rt_noise_tiles: no reprojected result held (rt_reproject first)");
    if (!c->hist_var || !d.rp_s2.ptr)
        return set_err(c, RT_ERR_STATE,
                       "rt_noise_tiles: the reprojected result carries no variance (rt_set_history_variance(ctx, 1) first)");
    HIPCHK(c, hipSetDevice(d.id));
    const int W = c->width, H = d.local_rows, nt = tiles_of(c);
    c->nz_rp_gen = 0;
    if ((r = ensure(c, d, d.nz_tiles, (size_t)nt * sizeof(rt_tile_noise)))) return r;
    hipLaunchKernelGGL(noise_tiles_kernel, dim3((unsigned)((nt + kTilesPerBlock - 1) / kTilesPerBlock)), dim3(256), 0, d.stream,
                       (const float4*)d.rp_out.ptr, (const float*)d.rp_s2.ptr, W, H, nt, min_count, (rt_tile_noise*)d.nz_tiles.ptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RT_ERR_DEVICE, std::string("rt_noise_tiles launch failed: ") + hipGetErrorString(e));
    c->nz_rp_gen = c->rp_gen;
    return RT_OK;
}

int rt_read_tile_noise(rt_ctx* c, rt_tile_noise* out, int cap, int* n_tiles) {
    if (!c || !n_tiles) return RT_ERR_INVALID_ARG;
    int r = refine_ready(c, "rt_read_tile_noise");
    if (r) return r;
    if (!noise_held(c))
        return set_err(c, RT_ERR_STATE,
                       "rt_read_tile_noise: no noise records held for the reprojected result (rt_noise_tiles first)");
    const int nt = tiles_of(c);
    *n_tiles = nt;
    if (!out) return RT_OK;
    if (cap < nt) return set_err(c, RT_ERR_LIMIT, "rt_read_tile_noise: out is too small");
    if ((r = rt_sync(c))) return r;
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    return d2h(c, d, out, d.nz_tiles.ptr, (size_t)nt * sizeof(rt_tile_noise));
}

int rt_render_moved_to_noise(rt_ctx* c, const float camera[28], int n_frames, const float* rand_factors,
                             const rt_noise_refine_params* refine, const rt_reproject_params* reproject,
                             const rt_denoise_params* denoise, const rt_guide_params* guides,
                             const rt_present_params* present, int* rounds_done, int* tiles_refined,
                             int64_t* tile_frames_spent, rt_moved_noise_stats* last) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (rounds_done) *rounds_done = 0;
    if (tiles_refined) *tiles_refined = 0;
    if (tile_frames_spent) *tile_frames_spent = 0;
    if (last) std::memset(last, 0, sizeof(*last));
    if (!refine) return rt_render_moved(c, camera, n_frames, rand_factors, reproject, denoise, guides, present);
    rt_nz_resolved prm;
    if (noise_refine_resolve(refine, &prm))
        return set_err(c, RT_ERR_INVALID_ARG,
                       "rt_render_moved_to_noise: target_noise >= 0 and finite, min_count >= 0 and finite, batch_frames >= 1, "
                       "max_rounds >= 0, reserved 0");
    int r = refine_ready(c, "rt_render_moved_to_noise");
    if (r) return r;
    if (c->mask_set)
        return set_err(c, RT_ERR_STATE, "rt_render_moved_to_noise: a tile mask is set (rt_set_active_tiles(ctx, NULL, 0))");
    if (!c->hist_var)
        return set_err(c, RT_ERR_STATE, "rt_render_moved_to_noise: the variance is not carried (rt_set_history_variance(ctx, 1) first)");
    if ((int64_t)n_frames + (int64_t)prm.batch_frames * prm.max_rounds > (int64_t)INT32_MAX)
        return set_err(c, RT_ERR_INVALID_ARG, "rt_render_moved_to_noise: n_frames + batch_frames * max_rounds overflows");
    if ((r = moved_to_reprojected(c, camera, n_frames, rand_factors, reproject))) return r;
    const int nt = tiles_of(c);
    std::vector<rt_tile_noise> recs((size_t)nt);
    std::vector<uint8_t> active((size_t)nt, 1), next((size_t)nt, 0);
    rt_moved_noise_stats stats;
    std::memset(&stats, 0, sizeof(stats));
    int rounds = 0, first_round = 0, converged = 0;
    int64_t spent = 0;
    for (;;) {
        int m = 0, n_active = 0;
        if ((r = rt_noise_tiles(c, prm.min_count))) return r;
        if ((r = rt_read_tile_noise(c, recs.data(), nt, &m))) return r;   // the round's one rt_sync
        if ((r = rt_refine_noise_select(recs.data(), active.data(), nt, prm.target_noise, next.data(), &n_active, &stats)))
            return set_err(c, r, "rt_render_moved_to_noise: rt_refine_noise_select refused the records");
        active.swap(next);   // the set only shrinks
        if (n_active == 0) {
            converged = 1;
            break;
        }
        if (rounds == prm.max_rounds) break;
        const int done = n_frames + rounds * prm.batch_frames;   // the frames every active tile holds
        // (every tile active: the plain launch, the same bits)
        r = n_active == nt ? rt_set_active_tiles(c, nullptr, 0) : rt_set_active_tiles(c, active.data(), nt);
        if (!r) r = rt_render(c, done + 1, prm.batch_frames, rand_factors + done);
        const int r2 = rt_set_active_tiles(c, nullptr, 0);   // no mask is left set
        if (r) return r;
        if (r2) return r2;
        if ((r = rt_reproject(c, reproject))) return r;   // over the same history; rp_gen moves on
        if (rounds == 0) first_round = n_active;
        spent += (int64_t)n_active * prm.batch_frames;
        rounds++;
    }
    stats.rounds = rounds;
    stats.converged = converged;
    if (rounds_done) *rounds_done = rounds;
    if (tiles_refined) *tiles_refined = first_round;
    if (tile_frames_spent) *tile_frames_spent = spent;
    if (last) *last = stats;
    return moved_filter_present(c, denoise, guides, present);
}

}  // extern "C"
