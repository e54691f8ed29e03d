// rt_fold_step.h — one frame of the running mean (compute.glsl:355): (prev * (n-1) + cur) / n
// per channel in f32 without contraction, w = 1.  The staged folds (rt_moments.hip) and the A/B
// kernels' ordered and in-place folds (rt_kernel_variants.hip) call it; render_stream's ordered
// fold (rt_kernel.hip) keeps the same operations written out, see there.  The same operations in
// the same order on every path, so the same image bits.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ void mean_step(float4& mean, const float4& c, const int fc) {
    const float n1 = (float)(fc - 1), n = (float)fc;
    mean.x = (mean.x * n1 + c.x) / n;
    mean.y = (mean.y * n1 + c.y) / n;
    mean.z = (mean.z * n1 + c.z) / n;
    mean.w = 1.0f;
}
