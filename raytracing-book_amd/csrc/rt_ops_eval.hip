// rt_ops_eval.hip -- rt_debug_eval_op's device half (rt_debug.h): one lane per input row calls the
// device function the render kernels call (rt_kernel_common.h) and stores what it returned.  A
// translation unit of its own: the render kernels' code objects (rt_kernel.hip) do not see it.
// Rows are processed in whole waves, in input order (the host pads the batch to a multiple of 64
// with copies of its last row), so the wave-wide ballots that choose a division form see the 64
// rows the test put together.
#include "rt/rt_debug.h"
#include "rt_kernel_common.h"

namespace {

// Row i: RT_OPS_ROW_F floats in (o, d, tmin, tmax, time, an int word, 2 unused), RT_OPS_OUT_W words out.
__global__ void __launch_bounds__(256) eval_op_kernel(const KP* __restrict__ Pp, int op, int form,
                                                      const float4* __restrict__ recs, const float* __restrict__ rows,
                                                      uint32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    // the packed Perlin table staged as the render kernels stage it: 256 float4 from offset 0
    if (op == RT_OP_PERLIN && form == 1) {
        for (int k = threadIdx.x; k < 256; k += 256) rt_dyn_lds[k] = ldg(recs + k);
        __syncthreads();
    }
    if (i >= n) return;   // n is a multiple of 64: whole waves leave
    const KP& P = *Pp;
    const float* r = rows + (size_t)i * RT_OPS_ROW_F;
    const v3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
    const float tmin = r[6], tmax = r[7], time = r[8];
    const int word = __float_as_int(r[9]);
    uint32_t* w = out + (size_t)i * RT_OPS_OUT_W;
    float t = 0.0f, al = 0.0f, be = 0.0f;
    int face = 0;
    bool hit = false;
    const float a = g_dot(d, d);
    if (op == RT_OP_SPHERE) {
        // form 0 '/', 1 the shared reciprocal (leaf_prims_t's call), 2 / 3 the same through sphere_t's loads
        const bool fd = (form & 1) != 0;
        if (form < 2)
            hit = sphere_t_ab(ldg(recs + 3 * i), ldg(recs + 3 * i + 1), time, o, d, a, tmin, tmax, t, fd,
                              fd ? rcp_nr(a) : 0.0f);
        else
            hit = sphere_t(recs + 3 * i, time, o, d, a, tmin, tmax, t, fd, fd ? rcp_nr(a) : 0.0f);
        w[0] = hit;
        w[1] = __float_as_uint(t);
    } else if (op == RT_OP_MEDIUM_SPHERE) {
        float t1 = 0.0f, t2 = 0.0f;
        hit = sphere_bounds(ldg(recs + 3 * i), ldg(recs + 3 * i + 1), o, d, a, time, t1, t2, form == 1);
        w[0] = hit;
        w[1] = __float_as_uint(t1);
        w[2] = __float_as_uint(t2);
    } else if (op == RT_OP_QUAD) {
        hit = quad_test(recs + RT_DFACE_F4 * i, o, d, tmin, tmax, t, al, be, form == 1);
        w[0] = hit;
        w[1] = __float_as_uint(t);
        w[2] = __float_as_uint(al);
        w[3] = __float_as_uint(be);
    } else if (op == RT_OP_BOX) {
        // form 0 / 1 box_test plain / fd on the box's dboxes record; 2 / 3 box_test_compact plain / fd and
        // 4 box_test_compact_q on its 48-byte record (recs: RT_DBOX_F4 + RT_BOXC_F4 float4 per row)
        const float4* fb = recs + (size_t)(RT_DBOX_F4 + RT_BOXC_F4) * i;
        const float4 c0 = ldg(fb + RT_DBOX_F4), c1 = ldg(fb + RT_DBOX_F4 + 1), c2 = ldg(fb + RT_DBOX_F4 + 2);
        if (form < 2)
            hit = box_test(fb, o, d, tmin, tmax, t, face, al, be, form == 1);
        else if (form < 4)
            hit = box_test_compact(c0, c1, c2, o, d, tmin, tmax, t, face, al, be, form == 3);
        else
            hit = box_test_compact_q(c0, c1, c2, o, d, tmin, tmax, t, face, al, be);
        w[0] = hit;
        w[1] = __float_as_uint(t);
        w[2] = (uint32_t)face;
        w[3] = __float_as_uint(al);
        w[4] = __float_as_uint(be);
    } else if (op == RT_OP_NODE) {
        // form 0 aabb_fast, 1 aabb_pk, 2 the exact per-axis slab of link_walk<EXACT>; inv as render_stream's
        const float* b = reinterpret_cast<const float*>(recs) + 6 * (size_t)i;
        const float4 n0 = make_float4(b[0], b[1], b[2], b[3]), n1 = make_float4(b[4], b[5], 0.0f, 0.0f);
        const v3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        if (form == 0) {
            hit = aabb_fast(n0, n1, o, inv, tmin, tmax);
        } else if (form == 1) {
            hit = aabb_pk(n0, n1, o, inv, tmin, tmax);
        } else {
            float lo = tmin, hi = tmax;
            slab(n0.x, n0.y, o.x, inv.x, lo, hi);
            slab(n0.z, n0.w, o.y, inv.y, lo, hi);
            slab(n1.x, n1.y, o.z, inv.z, lo, hi);
            hit = !(hi <= lo);
        }
        w[0] = hit;
    } else if (op == RT_OP_PERLIN) {
        // form 0 the texture in global memory (recs: 6 x 256 floats), 1 the packed table in LDS
        const float acc = form == 1 ? perlin_turb_lds(0, o.x, o.y, o.z)
                                    : perlin_turb_global(reinterpret_cast<const float*>(recs), 6, 256, o.x, o.y, o.z);
        w[0] = __float_as_uint(fabsf(acc));   // noise_turb's abs (texture_color applies it)
    } else if (op == RT_OP_SPHERE_UV) {
        const v2 uv = sphere_uv(o);
        w[0] = __float_as_uint(uv.x);
        w[1] = __float_as_uint(uv.y);
    } else if (op == RT_OP_TEXTURE) {
        // texture_color's checker and image branches on P.tex (global memory, no LDS tables): p = o,
        // the texture id in the int word, uv = (d.x, d.y) as a quad hit's (alpha, beta)
        UvSrc uvs;
        uvs.kind_idx = 2 << 16;
        uvs.a = d.x;
        uvs.b = d.y;
        uvs.c = 0.0f;
        const v3 c = texture_color<false, false>(P, o, word, uvs, time);
        w[0] = __float_as_uint(c.x);
        w[1] = __float_as_uint(c.y);
        w[2] = __float_as_uint(c.z);
    }
}

}  // namespace

int rt_launch_eval_op(const rt_kernel_args* dargs, int op, int form, const void* drecs, const float* drows, void* dout,
                      int n, void* stream) {
    if (n <= 0) return 0;
    if (n % 64) return -1;
    const size_t lds = (op == RT_OP_PERLIN && form == 1) ? 256 * sizeof(float4) : 0;
    hipLaunchKernelGGL(eval_op_kernel, dim3((n + 255) / 256), dim3(256), lds, (hipStream_t)stream, dargs, op, form,
                       (const float4*)drecs, drows, (uint32_t*)dout, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
