// rt_moments.hip — per-pixel sample moments beside the running mean, and their per-tile sums
// (rt.h rt_set_moments / rt_noise).  Nothing here touches the render kernels: a staged launch's
// colours are folded by fold_moments_kernel instead of rt_kernel.hip's fold_kernel, with the
// same operations on the mean (so the same image bits) plus a Welford update of the second
// moment (fold_tiles_kernel: either fold over the active tiles of a masked launch); tile_sums_kernel reduces image and moments to one record per 8x8 tile in a fixed
// order, so the host's noise figure depends on the inputs alone.  All arithmetic is f32 without
// contraction (-ffp-contract=off), and tests/test_gpu_moments.py restates it in numpy bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt/rt.h"
#include "rt_device.h"

namespace {

// One frame of a pixel: the running mean exactly as fold_kernel computes it, then
// M2 += (c - old) * (c - new) per channel and for the channel sum y = (x + y) + z in .w;
// frame 1 starts the moments at zero.
__device__ __forceinline__ void moment_step(float4& mean, float4& m2, const float4 c, const int fc) {
    const float n1 = (float)(fc - 1), n = (float)fc;
    float4 nw;
    nw.x = (mean.x * n1 + c.x) / n;
    nw.y = (mean.y * n1 + c.y) / n;
    nw.z = (mean.z * n1 + c.z) / n;
    nw.w = 1.0f;
    if (fc == 1) {
        m2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        m2.x = m2.x + (c.x - mean.x) * (c.x - nw.x);
        m2.y = m2.y + (c.y - mean.y) * (c.y - nw.y);
        m2.z = m2.z + (c.z - mean.z) * (c.z - nw.z);
        const float ys = (c.x + c.y) + c.z;
        const float yo = (mean.x + mean.y) + mean.z;
        const float yn = (nw.x + nw.y) + nw.z;
        m2.w = m2.w + (ys - yo) * (ys - yn);
    }
    mean = nw;
}

// fold_kernel's sibling: one thread per pixel, the launch's frames in frame order.  Sparse
// staging (sflags): a clear flag is the colour (+0, +0, +0); eight frames' flags, then the set
// ones' colours, are loaded before their eight folds, as fold_kernel does.
__global__ void __launch_bounds__(256) fold_moments_kernel(float4* __restrict__ image, float4* __restrict__ moments,
                                                           const float4* __restrict__ samples,
                                                           const uint8_t* __restrict__ sflags, size_t n_pixels,
                                                           int first_frame, int n_frames) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pixels) return;
    float4 mean = image[pix];
    float4 m2 = moments[pix];
    const float4* s = samples + pix;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sflags) {
        const uint8_t* fl = sflags + pix;
        int f = 0;
        for (; f + 8 <= n_frames; f += 8) {
            uint32_t fb[8];
            float4 cur[8];
#pragma unroll
            for (int k = 0; k < 8; k++) fb[k] = fl[(size_t)(f + k) * n_pixels];
#pragma unroll
            for (int k = 0; k < 8; k++) cur[k] = fb[k] ? s[(size_t)(f + k) * n_pixels] : z4;
#pragma unroll
            for (int k = 0; k < 8; k++) moment_step(mean, m2, cur[k], first_frame + f + k);
        }
        for (; f < n_frames; f++) {
            const float4 cur = fl[(size_t)f * n_pixels] ? s[(size_t)f * n_pixels] : z4;
            moment_step(mean, m2, cur, first_frame + f);
        }
    } else {
        for (int f = 0; f < n_frames; f++) moment_step(mean, m2, s[(size_t)f * n_pixels], first_frame + f);
    }
    image[pix] = mean;
    moments[pix] = m2;
}

// One frame of the running mean alone: fold_kernel's operations (moment_step's on the mean).
__device__ __forceinline__ void mean_step(float4& mean, const float4 c, const int fc) {
    const float n1 = (float)(fc - 1), n = (float)fc;
    mean.x = (mean.x * n1 + c.x) / n;
    mean.y = (mean.y * n1 + c.y) / n;
    mean.z = (mean.z * n1 + c.z) / n;
    mean.w = 1.0f;
}

// The folds of a launch under a tile mask (rt_set_active_tiles): one wave per active tile, lane
// ty * 8 + tx its pixel, lanes outside the image idle; a pixel of any other tile is neither read
// nor written.  Per pixel and in frame order the operations are fold_moments_kernel's (MOM) or
// fold_kernel's, with the sparse flags read the same way, so an active pixel's image and M2
// bits are those of the plain folds.
template <bool MOM>
__global__ void __launch_bounds__(256) fold_tiles_kernel(float4* __restrict__ image, float4* __restrict__ moments,
                                                         const float4* __restrict__ samples,
                                                         const uint8_t* __restrict__ sflags, size_t n_pixels,
                                                         int first_frame, int n_frames,
                                                         const int* __restrict__ tile_list, int n_active, int width,
                                                         int local_rows) {
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);   // wave-uniform
    if (k >= n_active) return;
    const int tile = tile_list[k];
    const int tiles_x = (width + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x >= width || y >= local_rows) return;
    const size_t pix = (size_t)y * width + x;
    float4 mean = image[pix];
    float4 m2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (MOM) m2 = moments[pix];
    const float4* s = samples + pix;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sflags) {
        const uint8_t* fl = sflags + pix;
        int f = 0;
        for (; f + 8 <= n_frames; f += 8) {
            uint32_t fb[8];
            float4 cur[8];
#pragma unroll
            for (int j = 0; j < 8; j++) fb[j] = fl[(size_t)(f + j) * n_pixels];
#pragma unroll
            for (int j = 0; j < 8; j++) cur[j] = fb[j] ? s[(size_t)(f + j) * n_pixels] : z4;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (MOM) moment_step(mean, m2, cur[j], first_frame + f + j);
                else mean_step(mean, cur[j], first_frame + f + j);
            }
        }
        for (; f < n_frames; f++) {
            const float4 cur = fl[(size_t)f * n_pixels] ? s[(size_t)f * n_pixels] : z4;
            if (MOM) moment_step(mean, m2, cur, first_frame + f);
            else mean_step(mean, cur, first_frame + f);
        }
    } else {
        for (int f = 0; f < n_frames; f++) {
            const float4 cur = s[(size_t)f * n_pixels];
            if (MOM) moment_step(mean, m2, cur, first_frame + f);
            else mean_step(mean, cur, first_frame + f);
        }
    }
    image[pix] = mean;
    if (MOM) moments[pix] = m2;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= __FLT_MAX__; }

// One wave per 8x8 tile (row-major tiles, the render kernels' unit_geo tiles): lane ty * 8 + tx
// holds its pixel's M2.w and y = (mean.x + mean.y) + mean.z, or +0 for both when it lies outside
// the image or either is not finite (a bad pixel); a xor butterfly (32, 16, 8, 4, 2, 1) leaves
// the same sums in every lane, and lane 0 stores the tile's record.
__global__ void __launch_bounds__(256) tile_sums_kernel(const float4* __restrict__ image,
                                                        const float4* __restrict__ moments, int width, int local_rows,
                                                        int n_tiles, rt_tile_sum* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);   // wave-uniform
    if (tile >= n_tiles) return;
    const int tiles_x = (width + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 8 + (lane >> 3);
    const bool in = x < width && y < local_rows;
    float sm = 0.0f, sy = 0.0f;
    bool bad = false;
    if (in) {
        const size_t pix = (size_t)y * width + x;
        const float4 mean = image[pix];
        const float m2y = moments[pix].w;
        const float lum = (mean.x + mean.y) + mean.z;
        bad = !(finite_f(lum) && finite_f(m2y));
        if (!bad) {
            sm = m2y;
            sy = lum;
        }
    }
    const unsigned long long in_mask = __ballot(in), bad_mask = __ballot(bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sm = sm + __shfl_xor(sm, off, 64);
        sy = sy + __shfl_xor(sy, off, 64);
    }
    if (lane == 0) {
        float4 rec;
        rec.x = sm;
        rec.y = sy;
        rec.z = __uint_as_float((uint32_t)__popcll(bad_mask));
        rec.w = __uint_as_float((uint32_t)__popcll(in_mask));
        *reinterpret_cast<float4*>(out + tile) = rec;
    }
}

static_assert(sizeof(rt_tile_sum) == 16, "a tile record is one 16-byte store");

}  // namespace

int rt_launch_fold_moments(const rt_kernel_args& a, void* moments, void* stream) {
    if (!a.samples || !moments || a.n_pixels == 0 || a.n_frames <= 0) return -1;
    const unsigned blocks = (unsigned)((a.n_pixels + 255) / 256);
    hipLaunchKernelGGL(fold_moments_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(a.image), (float4*)moments, (const float4*)a.samples,
                       (const uint8_t*)a.sflags, a.n_pixels, a.first_frame, a.n_frames);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_fold_tiles(const rt_kernel_args& a, void* moments, void* stream) {
    if (!a.samples || !a.tile_list || a.n_active <= 0 || a.n_pixels == 0 || a.n_frames <= 0) return -1;
    const dim3 grid((unsigned)((a.n_active + 3) / 4)), block(256);
    if (moments)
        hipLaunchKernelGGL(fold_tiles_kernel<true>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<float4*>(a.image),
                           (float4*)moments, (const float4*)a.samples, (const uint8_t*)a.sflags, a.n_pixels,
                           a.first_frame, a.n_frames, a.tile_list, a.n_active, a.width, a.local_rows);
    else
        hipLaunchKernelGGL(fold_tiles_kernel<false>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<float4*>(a.image),
                           (float4*)nullptr, (const float4*)a.samples, (const uint8_t*)a.sflags, a.n_pixels,
                           a.first_frame, a.n_frames, a.tile_list, a.n_active, a.width, a.local_rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_tile_sums(const void* image, const void* moments, int width, int local_rows, void* out, void* stream) {
    if (width <= 0 || local_rows <= 0) return 0;
    const int n_tiles = ((width + 7) / 8) * ((local_rows + 7) / 8);
    hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)image, (const float4*)moments, width, local_rows, n_tiles, (rt_tile_sum*)out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
