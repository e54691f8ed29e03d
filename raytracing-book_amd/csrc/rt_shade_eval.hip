// rt_shade_eval.hip -- rt_debug_eval_shade_op's device half (rt_debug.h): one lane per input row calls
// the sampling, light, camera or shading function the render kernels call (rt_kernel_common.h) on the
// scene of a context and stores what it returned and what it left in rf.  A translation unit of its
// own, like rt_ops_eval.hip: the render kernels' code objects (rt_kernel.hip) do not see it.
// The argument block has every LDS offset at -1 (the host half sets them), so no function here reads
// the dynamic LDS and the launch has none.  Rows are processed in whole waves, in input order.
#include "rt/rt_debug.h"
#include "rt_kernel_common.h"
#include "rt_plain_walk.h"

namespace {

// Row i: RT_SOP_ROW_F floats in (rt_debug.h lists them), RT_SOP_OUT_W words out.
__global__ void __launch_bounds__(256) eval_shade_op_kernel(const KP* __restrict__ Pp, int op, int form,
                                                            const float* __restrict__ rows,
                                                            uint32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;   // n is a multiple of 64: whole waves leave
    const KP& P = *Pp;
    const float* r = rows + (size_t)i * RT_SOP_ROW_F;
    const v3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
    const float time = r[8], px = r[9], py = r[10];
    float rf = r[11];
    uint32_t* w = out + (size_t)i * RT_SOP_OUT_W;
    auto put3 = [&](int k, v3 v) {
        w[k] = __float_as_uint(v.x);
        w[k + 1] = __float_as_uint(v.y);
        w[k + 2] = __float_as_uint(v.z);
    };
    if (op == RT_SOP_RAND) {
        for (int k = 0; k < 6; k++) w[k] = __float_as_uint(rnd(rf, px, py));
        w[6] = __float_as_uint(rf);
    } else if (op == RT_SOP_ONB) {
        put3(0, transform_onb(o, d));
    } else if (op == RT_SOP_UNIT_VEC) {
        put3(0, rand_unit_vec(rf, px, py));
        w[3] = __float_as_uint(rf);
    } else if (op == RT_SOP_MEDIUM_TAIL) {
        float t = 0.0f;
        const bool hit = medium_tail(r[0], r[1], r[2], r[3], r[4], r[5], rf, px, py, t);
        w[0] = hit;
        w[1] = __float_as_uint(hit ? t : 0.0f);
        w[2] = __float_as_uint(rf);
    } else if (op == RT_SOP_LIGHT_PDF) {
        w[0] = __float_as_uint(lights_pdf_value(P, o, d, time));
    } else if (op == RT_SOP_LIGHT_DIR) {
        put3(0, lights_random(P, o, rf, px, py));
        w[3] = __float_as_uint(rf);
    } else if (op == RT_SOP_CAMERA_RAY) {
        Path S;
        start_path(P, S, __float_as_int(r[19]), rf, px, py, pixel_base(P.cam, px, py));
        w[0] = __float_as_uint(S.time);
        put3(1, S.o);
        put3(4, S.d);
        w[7] = __float_as_uint(S.rf);
    } else if (op == RT_SOP_SHADE) {
        Path S;
        S.o = o;
        S.d = d;
        S.acc = mk3(r[12], r[13], r[14]);
        S.time = time;
        S.rf = rf;
        S.uvs.kind_idx = __float_as_int(r[15]);
        S.uvs.a = r[16];
        S.uvs.b = r[17];
        S.uvs.c = r[18];
        S.depth = 0;
        Hit h;
        h.t = r[6];
        h.tif = __float_as_int(r[7]);
        h.uv_kind_idx = 0;
        h.uv_a = h.uv_b = 0.0f;
        v3 result = mk3s(0.0f);
        const bool ended = form == 1 ? shade<false, false, false, true>(P, S, h, px, py, result)
                                     : shade<false, false, false, false>(P, S, h, px, py, result);
        w[0] = ended;
        if (ended) {
            put3(1, result);
        } else {
            put3(1, S.o);
            put3(4, S.d);
            put3(7, S.acc);
        }
        w[10] = __float_as_uint(S.rf);
    }
}

// RT_SOP_TRACE: the plain closest-hit walk from the root with media on, then the uv hand-over, as
// render_stream's HIT block and after_trace() do them after a walk (h.t = tmax, walk_uv).  Words 8..10
// (the oracle's visit counts and hash) stay 0: the link walk's nodes differ by design.
template <bool FD>
__global__ void __launch_bounds__(256) eval_trace_op_kernel(const KP* __restrict__ Pp, const float4* __restrict__ links,
                                                            int n_nodes, const float* __restrict__ rows,
                                                            uint32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;   // n is a multiple of 64: whole waves leave
    const KP& P = *Pp;
    const float* r = rows + (size_t)i * RT_SOP_ROW_F;
    const v3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
    const float time = r[8], px = r[9], py = r[10];
    float rf = r[11];
    UvSrc uvs = {__float_as_int(r[15]), r[16], r[17], r[18]};
    Hit h;
    bool has;
    float tmax;
    plain_walk<FD, true>(P, links, n_nodes, o, d, time, rf, px, py, h, has, tmax);
    walk_uv(h, o, d, uvs);
    uint32_t* w = out + (size_t)i * RT_SOP_OUT_W;
    w[0] = has;
    w[1] = __float_as_uint(has ? tmax : 0.0f);
    w[2] = has ? (uint32_t)h.tif : 0u;
    w[3] = (uint32_t)uvs.kind_idx;
    w[4] = __float_as_uint(uvs.a);
    w[5] = __float_as_uint(uvs.b);
    w[6] = __float_as_uint(uvs.c);
    w[7] = __float_as_uint(rf);
}

}  // namespace

int rt_launch_eval_trace_op(const rt_kernel_args* dargs, int form, const void* dlinks, int n_nodes, const float* drows,
                            void* dout, int n, void* stream) {
    if (n <= 0) return 0;
    if (n % 64) return -1;
    if (form == 1)
        hipLaunchKernelGGL(eval_trace_op_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dargs,
                           (const float4*)dlinks, n_nodes, drows, (uint32_t*)dout, n);
    else
        hipLaunchKernelGGL(eval_trace_op_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dargs,
                           (const float4*)dlinks, n_nodes, drows, (uint32_t*)dout, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_eval_shade_op(const rt_kernel_args* dargs, int op, int form, const float* drows, void* dout, int n,
                            void* stream) {
    if (n <= 0) return 0;
    if (n % 64) return -1;
    hipLaunchKernelGGL(eval_shade_op_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dargs, op, form,
                       drows, (uint32_t*)dout, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
