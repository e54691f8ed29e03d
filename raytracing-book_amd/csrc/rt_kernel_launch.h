// rt_kernel_launch.h -- what the two render translation units (rt_kernel.hip, rt_kernel_variants.hip)
// need beyond the restated shader of rt_kernel_common.h: the ordered-chunk hand-off, the LDS staging,
// the stats twins' leaf census and the persistent launcher.  The off-path units (rt_features.hip,
// rt_ops_eval.hip, rt_shade_eval.hip) do not include it.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "rt_fold_step.h"
#include "rt_kernel_common.h"
#include "rt_plan.h"

namespace {

// The leaf census (stats twin with P.census): one record per wave leaf round -- when it started,
// how long it took, which wave, how many lanes were walking, and per prim type how many lanes
// hold a slot-0 / slot-1 test -- so tools/leaf_census.py can count what a workgroup-wide queue
// per prim type could have pooled.  Called by the lanes at a leaf (the first one writes).
__device__ __forceinline__ void census_leaf(const KP& P, int gwave, uint32_t types, unsigned long long t0,
                                            unsigned long long t1, int walking, unsigned long long* st) {
    const uint32_t a = types & 7u, b = (types >> 4) & 0xFu;
    uint32_t s0 = 0, s1 = 0;
#pragma unroll
    for (int k = 1; k <= 4; k++) {
        s0 |= (uint32_t)__popcll(__ballot(a == (uint32_t)k)) << (8 * (k - 1));
        s1 |= (uint32_t)__popcll(__ballot(b == (uint32_t)k)) << (8 * (k - 1));
    }
    if (first_active_lane()) {
        const unsigned long long i = atomicAdd(&st[ST_CEN_N], 1ull);
        if (gwave < P.census_waves && i < (unsigned long long)P.census_cap) {
            unsigned* r = P.census + P.census_waves + ((size_t)gwave * P.census_cap + i) * RT_CENSUS_WORDS;
            r[0] = (unsigned)t0;
            r[1] = (unsigned)(t1 - t0);
            r[2] = (unsigned)blockIdx.x | ((unsigned)(threadIdx.x >> 6) << 16) | ((unsigned)walking << 24);
            r[3] = s0;
            r[4] = s1;
        }
    }
}

// Ordered chunks (a launch over few tiles per resident wave, e.g. the stripe set
// of one of N GPUs): the work unit is one 8x8 tile x one chunk of the launch's
// frames, unit = chunk * n_tiles + tile, so chunk k of a tile is dequeued after
// chunk k-1.  The wave that takes chunk k > 0 waits until chunk k-1 of its tile
// is published, then continues that tile's running mean from the image: the
// reference's per-frame formula in frame order, so the same bits as one chunk.
// Publication follows the agent-scope release/acquire recipe of
// cdna_hip_programming.md §6 G16: the producing wave's plain image stores,
// vmcnt(0), release fence, vmcnt(0), then one relaxed agent-scope store of the
// tile's chunk count; the consumer polls that word relaxed (with s_sleep), then
// one acquire fence, then plain loads.  The unit it waits for was dequeued
// earlier by a running wave that waits only on earlier units, so the chain ends
// at chunk 0; the poll is still bounded (RT_CHUNK_WAIT_TICKS of the 100 MHz
// real-time clock, P.chunk_wait_ticks: 30 s by default) and a timeout sets
// P.fault, which rt_sync reports.
typedef __attribute__((address_space(1))) unsigned gu32;   // global (never flat) accesses to shared words
// tile and chunk are wave-uniform (readfirstlane): every lane polls / stores the
// same word with the same value, so there is no lane-divergent control flow here
__device__ __forceinline__ void wait_chunk(const KP& P, int tile, int chunk) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    gu32* w = (gu32*)(P.tile_done + tile);
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) <
           (unsigned)chunk) {
        __builtin_amdgcn_s_sleep(2);
        if (__builtin_amdgcn_s_memrealtime() - t0 >= P.chunk_wait_ticks) {
            __hip_atomic_store((gu32*)P.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void publish_chunk(const KP& P, int tile, int chunk) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store((gu32*)(P.tile_done + tile), (unsigned)(chunk + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The link-format shapes' LDS staging (rt_capi.hip plans it; every workgroup once): the nodes
// (all, or the two-level walk's top levels; LINK = false: the threaded meta-word nodes of the A/B
// variant 30), the leaf records, the packed Perlin table, the media records with their sphere
// boundaries, the spheres' (A, B) halves, the boxes' compact records and the shading tables.
template <bool LINK, int BLOCK>
__device__ __forceinline__ void stage_lds(const KP& P, float4* s_nodes, int tid) {
    // link format: the nodes staged (all, or the two-level walk's top levels), then the leaf
    // records when they are staged too; meta format: the threaded nodes
    const float4* g = LINK ? P.lnodes : reinterpret_cast<const float4*>(P.nodes);
    const int nf4 = LINK ? P.lds_node_f4 : 2 * P.n_nodes;
    for (int k = tid; k < nf4; k += BLOCK) s_nodes[k] = g[k];
    if (LINK && P.leaf_lds >= 0)
        for (int k = tid; k < P.n_lnode_f4 - 2 * P.n_nodes; k += BLOCK)
            s_nodes[P.leaf_lds + k] = g[2 * P.n_nodes + k];
    if (P.perlin_lds >= 0)   // the packed Perlin table after the nodes (host-sized launch)
        for (int k = tid; k < 256; k += BLOCK) s_nodes[P.perlin_lds + k] = ldg(P.perlin_pk + k);
    if (P.media_lds >= 0) {   // per medium: (boundary idx, type, -1/density, phase), sphere A, B
        for (int k = tid; k < 3 * P.n_media; k += BLOCK) {
            const rt_medium& m = P.media[k / 3];
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k % 3 == 0)
                v = make_float4(__int_as_float(m.boundary_idx), __int_as_float(m.boundary_type), m.neg_inv_density,
                                __int_as_float(m.phase_material));
            else if (m.boundary_type == RT_MODEL_SPHERE)
                v = reinterpret_cast<const float4*>(P.spheres + m.boundary_idx)[k % 3 - 1];
            s_nodes[P.media_lds + k] = v;
        }
    }
    if (P.sph_lds >= 0) {   // per sphere its first two float4 (center0 + texture, motion + radius)
        const float4* sp = reinterpret_cast<const float4*>(P.spheres);
        for (int k = tid; k < 2 * P.n_sph_lds; k += BLOCK) s_nodes[P.sph_lds + k] = ldg(sp + (k >> 1) * 3 + (k & 1));
    }
    if (P.box_cmp_lds >= 0)   // the boxes' compact records (box_test_compact)
        for (int k = tid; k < RT_BOXC_F4 * P.n_box_lds; k += BLOCK) s_nodes[P.box_cmp_lds + k] = ldg(P.dboxc + k);
    // the shading tables (P.sph_mat_lds / box_mat_lds / tex_lds, option shade_lds)
    if (P.sph_mat_lds >= 0) {   // per sphere its third float4: emission, material
        const float4* sp = reinterpret_cast<const float4*>(P.spheres);
        for (int k = tid; k < P.n_sph_lds; k += BLOCK) s_nodes[P.sph_mat_lds + k] = ldg(sp + 3 * k + 2);
    }
    if (P.box_mat_lds >= 0) {   // per box quads[0]'s emission and material
        for (int k = tid; k < P.n_box_lds; k += BLOCK) {
            const float4* q0 = reinterpret_cast<const float4*>(P.boxes + k);
            const float4 e = ldg(q0 + 4), m = ldg(q0 + 1);
            s_nodes[P.box_mat_lds + k] = make_float4(e.x, e.y, e.z, m.w);
        }
    }
    if (P.tex_lds >= 0) {   // per slot (w, h, is_float, texel offset), then the small slots' texels
        if (tid < 8) {
            const rt_dtex& T = P.tex[tid];
            const int off = T.data ? P.tex_lds_off[tid] : -1;
            s_nodes[P.tex_lds + tid] = make_float4(__int_as_float(T.data ? T.w : 0), __int_as_float(T.h),
                                                   __int_as_float(T.is_float), __int_as_float(off));
        }
        for (int t = 0; t < 8; t++) {
            const rt_dtex& T = P.tex[t];
            if (P.tex_lds_off[t] < 0 || !T.data) continue;
            const int words = T.w * T.h;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(T.data);
            uint32_t* dst = reinterpret_cast<uint32_t*>(s_nodes + P.tex_lds_off[t]);
            for (int k = tid; k < words; k += BLOCK) dst[k] = src[k];
        }
    }
}

template <typename K>
int launch_persistent(K kernel, int block, size_t lds, const rt_kernel_args& a, const rt_kernel_args* d,
                      hipStream_t st) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    per_cu = per_cu > 2 ? 2 : per_cu;   // rt_resident_waves(): the per-wave buffers are sized for it
    if ((long long)cus * per_cu * (block / 64) > (long long)rt_resident_waves()) return -1;
    if (a.wbuf && (long long)cus * per_cu * (block / 64) > (long long)a.wbuf_waves) return -1;
    hipLaunchKernelGGL(kernel, dim3(cus * per_cu), dim3(block), lds, st, d);
    return 0;
}

}  // namespace
