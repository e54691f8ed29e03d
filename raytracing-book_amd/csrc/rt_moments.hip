// rt_moments.hip — the folds of a staged launch's colours into the running mean, the per-pixel
// sample moments beside it and their per-tile sums (rt.h rt_set_moments / rt_noise).  Nothing here
// touches the render kernels.  One body folds a pixel (fold_pixel): the mean by mean_step
// (rt_fold_step.h, which the render kernels' ordered and in-place folds call too, so every path
// gives the same image bits) and, with MOM, a Welford update of the second moment (moment_step).
// Two thin kernels call it: one thread per pixel, or one wave per active tile of a masked launch.
// tile_sums_kernel reduces image and moments to one record per 8x8 tile in a fixed order, so the
// host's noise figure depends on the inputs alone.  All arithmetic is f32 without contraction
// (-ffp-contract=off), and tests/test_gpu_moments.py restates it in numpy bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt/rt.h"
#include "rt_device.h"
#include "rt_fold_step.h"

namespace {

// One frame of a pixel: the running mean by mean_step, then M2 += (c - old) * (c - new) per
// channel and for the channel sum y = (x + y) + z in .w; frame 1 starts the moments at zero.
__device__ __forceinline__ void moment_step(float4& mean, float4& m2, const float4 c, const int fc) {
    float4 nw = mean;
    mean_step(nw, c, fc);
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

// What a fold reads and writes: the image and (MOM) the moments [n_pixels] float4, the launch's
// colours [n_frames][n_pixels] and, with sparse staging, their flags (else nullptr).
struct FoldArgs {
    float4* image;
    float4* moments;
    const float4* samples;
    const uint8_t* sflags;
    size_t n_pixels;
    int first_frame, n_frames;
};

// Pixel pix: the launch's frames folded in frame order into its mean and (MOM) its M2.  Sparse
// staging: a clear flag is the colour (+0, +0, +0), never stored; eight frames at a time, their
// flags, then the set ones' colours, are loaded before the eight steps, then the tail one by one.
template <bool MOM>
__device__ __forceinline__ void fold_pixel(const FoldArgs& A, const size_t pix) {
    float4 mean = A.image[pix];
    float4 m2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (MOM) m2 = A.moments[pix];
    const float4* s = A.samples + pix;
    const size_t np = A.n_pixels;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto step = [&](const float4 c, const int f) {
        if (MOM) moment_step(mean, m2, c, A.first_frame + f);
        else mean_step(mean, c, A.first_frame + f);
    };
    if (A.sflags) {
        const uint8_t* fl = A.sflags + pix;
        int f = 0;
        for (; f + 8 <= A.n_frames; f += 8) {
            uint32_t fb[8];
            float4 cur[8];
#pragma unroll
            for (int k = 0; k < 8; k++) fb[k] = fl[(size_t)(f + k) * np];
#pragma unroll
            for (int k = 0; k < 8; k++) cur[k] = fb[k] ? s[(size_t)(f + k) * np] : z4;
#pragma unroll
            for (int k = 0; k < 8; k++) step(cur[k], f + k);
        }
        for (; f < A.n_frames; f++) step(fl[(size_t)f * np] ? s[(size_t)f * np] : z4, f);
    } else {
        for (int f = 0; f < A.n_frames; f++) step(s[(size_t)f * np], f);
    }
    A.image[pix] = mean;
    if (MOM) A.moments[pix] = m2;
}

// One thread per pixel of the image.
template <bool MOM>
__global__ void __launch_bounds__(256) fold_pixels_kernel(const FoldArgs A) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix < A.n_pixels) fold_pixel<MOM>(A, pix);
}

// A launch under a tile mask (rt_set_active_tiles): one wave per active tile, lane ty * 8 + tx its
// pixel, lanes outside the image idle; a pixel of any other tile is neither read nor written.
template <bool MOM>
__global__ void __launch_bounds__(256) fold_tiles_kernel(const FoldArgs A, const int* __restrict__ tile_list,
                                                         int n_active, int width, int local_rows) {
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);   // wave-uniform
    if (k >= n_active) return;
    const int tile = tile_list[k];
    const int tiles_x = (width + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x < width && y < local_rows) fold_pixel<MOM>(A, (size_t)y * width + x);
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

static FoldArgs fold_args(const rt_kernel_args& a, void* moments) {
    return {reinterpret_cast<float4*>(a.image), (float4*)moments, a.samples, a.sflags, a.n_pixels, a.first_frame,
            a.n_frames};
}

int rt_launch_fold_moments(const rt_kernel_args& a, void* moments, void* stream) {
    if (!a.samples || a.n_pixels == 0 || a.n_frames <= 0) return -1;
    const dim3 grid((unsigned)((a.n_pixels + 255) / 256)), block(256);
    if (moments) hipLaunchKernelGGL(fold_pixels_kernel<true>, grid, block, 0, (hipStream_t)stream, fold_args(a, moments));
    else hipLaunchKernelGGL(fold_pixels_kernel<false>, grid, block, 0, (hipStream_t)stream, fold_args(a, nullptr));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_fold_tiles(const rt_kernel_args& a, void* moments, void* stream) {
    if (!a.samples || !a.tile_list || a.n_active <= 0 || a.n_pixels == 0 || a.n_frames <= 0) return -1;
    const dim3 grid((unsigned)((a.n_active + 3) / 4)), block(256);
    if (moments)
        hipLaunchKernelGGL(fold_tiles_kernel<true>, grid, block, 0, (hipStream_t)stream, fold_args(a, moments),
                           a.tile_list, a.n_active, a.width, a.local_rows);
    else
        hipLaunchKernelGGL(fold_tiles_kernel<false>, grid, block, 0, (hipStream_t)stream, fold_args(a, nullptr),
                           a.tile_list, a.n_active, a.width, a.local_rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_tile_sums(const void* image, const void* moments, int width, int local_rows, void* out, void* stream) {
    if (width <= 0 || local_rows <= 0) return 0;
    const int n_tiles = ((width + 7) / 8) * ((local_rows + 7) / 8);
    hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)image, (const float4*)moments, width, local_rows, n_tiles, (rt_tile_sum*)out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
