// rt_prep.cpp — host-only scene preparation (rt_prep.h): everything the kernels' inputs are
// derived from before a byte reaches the device.  The bit-exactness arguments of the link
// format, the rebuilt and collapsed trees and the compact box records live here.
#include "rt_prep.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>

namespace rt_impl __attribute__((visibility("hidden"))) {

static int fail(std::string* err, int code, const char* m) {
    if (err) *err = m;
    return code;
}

int local_rows_of(int h, int rank, int world, int stripe) {
    if (h <= 0 || world <= 0 || stripe <= 0) return 0;
    int n = 0;
    int n_stripes = (h + stripe - 1) / stripe;
    for (int s = rank; s < n_stripes; s += world) n += std::min(stripe, h - s * stripe);
    return n;
}

int padded_rows_of(int h, int world, int stripe) {
    int n_stripes = (h + stripe - 1) / stripe;
    return ((n_stripes + world - 1) / world) * stripe;
}

// Re-lay the reference's pre-order BVH (BVHNode.java:13-56) as a threaded
// array in the reference traversal's own visiting order (right child first).
int thread_bvh(const rt_bvh_node* in, int n, std::vector<rt_dnode>& out, std::string* err) {
    out.clear();
    if (n == 0) return RT_OK;
    // Explicit DFS producing right-first pre-order; skip links patched after.
    std::vector<int> order_src;
    // Iterative: emit node, then (if inner) process right subtree whose skip = first node of left subtree,
    // then left subtree whose skip = this node's skip.
    // We compute skip by a second pass: skip(node) = next emitted node after its subtree.
    std::vector<int> subtree_end;   // emitted index one past this node's subtree
    // recursive lambda with explicit stack to avoid deep recursion
    struct Work { int src; int depth; int phase; int emitted; };
    std::vector<Work> st;
    st.push_back({0, 1, 0, -1});
    const size_t kMaxNodes = (size_t)RT_MAX_RECORDS;
    while (!st.empty()) {
        Work& w = st.back();
        if (w.phase == 0) {
            if (w.src < 0 || w.src >= n) return fail(err, RT_ERR_INVALID_ARG, "BVH child index out of range");
            if (w.depth > RT_MAX_BVH_DEPTH) return fail(err, RT_ERR_LIMIT, "BVH deeper than the reference's stack[64]");
            if (order_src.size() >= kMaxNodes) return fail(err, RT_ERR_LIMIT, "threaded BVH exceeds 65535 nodes");
            w.emitted = (int)order_src.size();
            order_src.push_back(w.src);
            subtree_end.push_back(0);
            const rt_bvh_node& nd = in[w.src];
            int lt = nd.left_id & 0xFFFF;
            if (lt != 0) {
                subtree_end[w.emitted] = w.emitted + 1;
                st.pop_back();
                continue;
            }
            w.phase = 1;
            int right = (nd.right_id >> 16) & 0xFFFF;
            int depth = w.depth;
            st.push_back({right, depth + 1, 0, -1});
        } else if (w.phase == 1) {
            w.phase = 2;
            const rt_bvh_node& nd = in[w.src];
            int left = (nd.left_id >> 16) & 0xFFFF;
            int depth = w.depth;
            st.push_back({left, depth + 1, 0, -1});
        } else {
            subtree_end[w.emitted] = (int)order_src.size();
            st.pop_back();
        }
    }
    int m = (int)order_src.size();
    out.resize(m);
    for (int k = 0; k < m; k++) {
        const rt_bvh_node& nd = in[order_src[k]];
        rt_dnode& d = out[k];
        d.xmin = nd.xmin; d.xmax = nd.xmax; d.ymin = nd.ymin; d.ymax = nd.ymax; d.zmin = nd.zmin; d.zmax = nd.zmax;
        int e = subtree_end[k];
        uint32_t skip = (e >= m) ? RT_NODE_END : (uint32_t)e;
        uint32_t lt = (uint32_t)(nd.left_id & 0xFFFF), rt = (uint32_t)(nd.right_id & 0xFFFF);
        if (lt != 0) {
            if (lt > 15 || rt > 15 || rt == 0) return fail(err, RT_ERR_INVALID_ARG, "BVH leaf with bad model type");
            // A singleton leaf lists one prim twice (BVHNode.java:33-34).
            // Re-testing a sphere cannot hit (strict root test against the t it set);
            // a quad/box re-hit at equal t rebuilds the same record (same face: the
            // last interior face of minimal t).  Only a medium's second test matters
            // (its own rand() draw), so for the others slot 2 is marked empty (type 0).
            if (lt == rt && nd.left_id == nd.right_id && lt != RT_MODEL_CONSTANT_MEDIUM) rt = 0;
            d.meta = skip | (lt << 16) | (rt << 20);
            d.prims = (uint32_t)((nd.left_id >> 16) & 0xFFFF) | ((uint32_t)((nd.right_id >> 16) & 0xFFFF) << 16);
        } else {
            d.meta = skip;
            d.prims = 0;
        }
    }
    return RT_OK;
}

// Every inner node's two children (right = k+1, left = skip of k+1) lie inside
// its box.  The reference's builder guarantees it (a node's box is the padded
// join of its children's, AABB.java:15-66); uploaded bytes are checked anyway
// because the speculative walk (rt_kernel.hip, Trace) relies on it.
bool boxes_nest(const std::vector<rt_dnode>& dn) {
    const int m = (int)dn.size();
    auto inside = [](const rt_dnode& c, const rt_dnode& p) {
        return c.xmin >= p.xmin && c.xmax <= p.xmax && c.ymin >= p.ymin && c.ymax <= p.ymax && c.zmin >= p.zmin &&
               c.zmax <= p.zmax;
    };
    for (int k = 0; k < m; k++) {
        if ((dn[k].meta & 0xF0000u) != 0) continue;   // leaf
        if (k + 1 >= m) return false;
        uint32_t l = dn[k + 1].meta & 0xFFFFu;
        if (l == RT_NODE_END || (int)l >= m) return false;
        if (!inside(dn[k + 1], dn[k]) || !inside(dn[l], dn[k])) return false;
    }
    return true;
}

// The threaded BVH in link format (rt_device.h RT_LINK_*; rt_kernel.hip link_walk):
// the same nodes and boxes, placed breadth-first (node k's children in the threaded
// array are its right child k + 1 and its left child skip(k + 1)), each with its
// successor addresses: on a box hit an inner node continues at its right child (the
// reference pushes left then right and pops right first, compute.glsl:259-260), a leaf
// leaves the loop with its ordinal; on a miss both continue at the threaded skip node.
// Leaf j's record follows the nodes: (prim types | the skip node's address << 8,
// prims), in threaded order.  The walk therefore visits the threaded walk's node
// sequence (tests/test_link_nodes.py), and the top levels every ray walks sit at the
// lowest addresses, the part a two-level launch stages in LDS.  Empty when there is
// no BVH or it has more nodes than 16-bit indices address.
std::vector<float4> build_links(const std::vector<rt_dnode>& dn, const std::vector<float>* vbox,
                                int* n_nodes_out, const std::vector<uint8_t>* drop) {
    std::vector<float4> out;
    const size_t n = dn.size();
    if (n_nodes_out) *n_nodes_out = 0;
    if (n == 0 || n > RT_LINK_MAX_NODES) return out;
    auto is_leaf = [&](size_t k) { return (dn[k].meta & 0xF0000u) != 0; };
    // Node collapse (plan_collapse): a link that leads to a left-out inner node leads to its first
    // child (threaded k + 1) instead, repeatedly; the left-out nodes get no place (the kept nodes keep
    // their breadth-first order, so a two-level launch's LDS prefix holds only reachable nodes).
    const bool dropping = drop && drop->size() == n && !(*drop)[0];
    auto kept = [&](uint32_t k) {
        while (dropping && k < n && (*drop)[k] && !is_leaf(k)) k++;
        return k;
    };
    std::vector<uint32_t> pos(n, 0xFFFFFFFFu), order;
    order.reserve(n);
    order.push_back(0);
    for (size_t h = 0; h < order.size(); h++) {
        const uint32_t k = order[h];
        if (pos[k] != 0xFFFFFFFFu || order.size() > n) return std::vector<float4>();
        pos[k] = (uint32_t)h;
        if (is_leaf(k)) continue;
        const uint32_t l = k + 1 < n ? (dn[k + 1].meta & 0xFFFFu) : RT_NODE_END;
        if (k + 1 >= n || l == RT_NODE_END || l >= n) return std::vector<float4>();
        order.push_back(k + 1);
        order.push_back(l);
    }
    if (order.size() != n) return out;
    size_t nk = n;   // the tree's nodes that get a place
    if (dropping) {
        nk = 0;
        for (size_t h = 0; h < n; h++) {
            const uint32_t k = order[h];
            pos[k] = ((*drop)[k] && !is_leaf(k)) ? 0xFFFFFFFFu : (uint32_t)nk++;
        }
    }
    // Box pre-tests as nodes (vbox: 6 floats per box, its bounds grown by the pre-test's margin,
    // rt_kernel.hip leaf_prims_t): a leaf of one or two boxes becomes a chain of one node per box
    // whose hit leads to that box's own leaf record -- the box tested alone, marked pre-tested
    // (RT_LINK_PRETESTED) -- and whose miss (or the record's continuation) leads to the next box's
    // node, after the last one to the leaf's skip node.  The walk meets the boxes in the same
    // order, each node test is the pre-test itself (the same slab function on the same floats
    // under the same ray_t), and a box whose pre-test misses is one the exact test rejects, so
    // every lane tests the same boxes with the same results -- only the pre-test moves from the
    // leaf stage into the walk.  The chain nodes follow the tree's nodes.
    const size_t nbox = vbox ? vbox->size() / 6 : 0;
    std::vector<uint32_t> vfirst(n, 0xFFFFFFFFu);   // leaf k's first chain node (0xFFFFFFFF: not expanded)
    size_t nv = 0;
    for (size_t k = 0; k < n && vbox; k++) {
        if (!is_leaf(k)) continue;
        const uint32_t t0 = (dn[k].meta >> 16) & 0xFu, t1 = (dn[k].meta >> 20) & 0xFu;
        const uint32_t p0 = dn[k].prims & 0xFFFFu, p1 = dn[k].prims >> 16;
        if (t0 != RT_MODEL_BOX || (t1 != RT_MODEL_BOX && t1 != 0) || p0 >= nbox || (t1 && p1 >= nbox)) continue;
        vfirst[k] = (uint32_t)(nk + nv);
        nv += t1 ? 2 : 1;
    }
    const size_t N = nk + nv;
    if (N > RT_LINK_MAX_NODES) return build_links(dn, nullptr, n_nodes_out, drop);
    size_t nl = 0;
    for (size_t k = 0; k < n; k++)
        if (is_leaf(k)) nl += vfirst[k] == 0xFFFFFFFFu ? 1 : (((dn[k].meta >> 20) & 0xFu) ? 2 : 1);
    out.assign(2 * N + (nl + 1) / 2, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    uint2* leaves = reinterpret_cast<uint2*>(out.data() + 2 * N);
    auto f = [](uint32_t u) {
        float x;
        std::memcpy(&x, &u, 4);
        return x;
    };
    auto put = [&](size_t at, float x0, float x1, float y0, float y1, float z0, float z1, uint32_t hit, uint32_t miss) {
        out[2 * at] = make_float4(x0, x1, y0, y1);
        out[2 * at + 1] = make_float4(z0, z1, f(hit), f(miss));
    };
    uint32_t li = 0;
    for (size_t k = 0; k < n; k++) {
        const rt_dnode& d = dn[k];
        if (pos[k] == 0xFFFFFFFFu) continue;   // left out (collapse)
        const uint32_t skip = d.meta & 0xFFFFu;
        const uint32_t skip_at = skip == RT_NODE_END ? RT_LINK_END : 32u * pos[kept(skip)];
        const uint32_t next_end = skip == RT_NODE_END ? RT_LINK_NEXT_END : skip_at;
        uint32_t hit;
        if (is_leaf(k) && vfirst[k] != 0xFFFFFFFFu) {
            const uint32_t v0 = vfirst[k];
            const bool two = ((d.meta >> 20) & 0xFu) != 0;
            hit = 32u * v0;
            for (int j = 0; j < (two ? 2 : 1); j++) {
                const uint32_t b = j ? d.prims >> 16 : d.prims & 0xFFFFu;
                const float* g = vbox->data() + 6 * (size_t)b;
                const bool last = !two || j == 1;
                const uint32_t cont = last ? skip_at : 32u * (v0 + 1);
                put(v0 + j, g[0], g[1], g[2], g[3], g[4], g[5], RT_LINK_LEAF | li, cont);
                leaves[li++] = make_uint2((RT_MODEL_BOX | RT_LINK_PRETESTED) | (last ? next_end : cont) << 8, b);
            }
        } else if (is_leaf(k)) {
            hit = RT_LINK_LEAF | li;
            leaves[li++] = make_uint2(((d.meta >> 16) & 0xFFu) | next_end << 8, d.prims);
        } else {
            hit = 32u * pos[kept((uint32_t)k + 1)];
        }
        put(pos[k], d.xmin, d.xmax, d.ymin, d.ymax, d.zmin, d.zmax, hit, skip_at);
    }
    if (n_nodes_out) *n_nodes_out = (int)N;
    return out;
}

// Small trees (up to RT_SMALL_TREE nodes: the Cornell boxes' 7) keep their nodes: there the camera's
// rays are few of the walks (paths bounce inside the box) and their counts mislead -- scenes 6 / 7
// measured +7.7 / +13.8% with the grid's choice, while scene 0 (511 nodes) -8.8%, scene 8 -5.6%
// (profiles/r05_j_opts_s*.log).
#define RT_SMALL_TREE 64

// Inner-node rebuild (option rebuild): the walk's leaves tested, their order and each test's
// ray_t do not depend on the inner nodes above them, as long as every inner box holds the leaf
// boxes below it.  A leaf node whose box test hits (under the ray_t of its turn) has every
// ancestor's test hit too -- an ancestor is tested earlier, under a ray_t.max at least as large,
// and the slab test is monotone in the box and in ray_t.max (plan_collapse below) -- so it is
// tested in any such tree; one whose test misses has its prims tested in none.  The leaves' own
// boxes and their order (the reference's walk order, the threaded array's) decide everything.  So
// the inner nodes are rebuilt over the reference's leaf sequence: each range of consecutive leaves
// split where the surface-area cost of its two parts, area x leaves, is least, a node's box the
// exact join (min / max) of its leaves' boxes.  The reference's builder splits at the median along
// a random axis (BVHNode.java:13-56); over scene 8's leaf order this tree takes a camera ray
// through 35% fewer node tests (tools/node_collapse_study.py).  Leaves and their records are
// unchanged.  Empty when the uploaded tree's boxes do not nest (the reference's walk
// then prunes leaves at a missed ancestor that the rebuilt tree would reach -- the ABI accepts any
// BVH bytes, so this is checked, as plan_collapse does), when a leaf box is flat or inverted
// (plan_collapse's condition), when the tree has fewer than 3 leaves, or when the host memory
// for the plan cannot be had.
std::vector<rt_dnode> rebuild_inner_impl(const std::vector<rt_dnode>& dn, int mode);
std::vector<rt_dnode> rebuild_inner(const std::vector<rt_dnode>& dn, int mode) {
    if (dn.size() <= RT_SMALL_TREE || dn.size() > RT_LINK_MAX_NODES || !boxes_nest(dn)) return {};
    try {
        return rebuild_inner_impl(dn, mode);
    } catch (const std::bad_alloc&) {   // the walk keeps the uploaded tree
        return {};
    }
}

// The dynamic programme's ranges: up to RT_REBUILD_DP_LEAVES leaves (3 m x m doubles + an m x m
// split table: 28 MB at 1024; scene 8 has 897 leaves), greedy splits above.
#define RT_REBUILD_DP_LEAVES 1024

std::vector<rt_dnode> rebuild_inner_impl(const std::vector<rt_dnode>& dn, int mode) {
    std::vector<rt_dnode> out;
    const size_t n = dn.size();
    std::vector<uint32_t> L;
    for (size_t k = 0; k < n; k++) {
        const rt_dnode& d = dn[k];
        if ((d.meta & 0xF0000u) == 0) continue;
        if (!(d.xmin < d.xmax && d.ymin < d.ymax && d.zmin < d.zmax)) return out;
        L.push_back((uint32_t)k);
    }
    const size_t m = L.size();
    if (m < 3 || 2 * m - 1 > RT_LINK_MAX_NODES) return out;
    auto join = [](rt_dnode& a, const rt_dnode& b) {
        a.xmin = std::min(a.xmin, b.xmin); a.xmax = std::max(a.xmax, b.xmax);
        a.ymin = std::min(a.ymin, b.ymin); a.ymax = std::max(a.ymax, b.ymax);
        a.zmin = std::min(a.zmin, b.zmin); a.zmax = std::max(a.zmax, b.zmax);
    };
    auto area = [](const rt_dnode& b) {
        const double dx = (double)b.xmax - b.xmin, dy = (double)b.ymax - b.ymin, dz = (double)b.zmax - b.zmin;
        return dx * dy + dy * dz + dz * dx;
    };
    out.resize(2 * m - 1);
    std::vector<rt_dnode> pre(m), suf(m);
    // mode 2 (up to RT_REBUILD_DP_LEAVES leaves): the split points of the tree whose inner boxes'
    // areas sum least, by a dynamic programme over the ranges; otherwise each range split greedily
    std::vector<uint32_t> split;
    if (mode == 2 && m <= RT_REBUILD_DP_LEAVES) {
        std::vector<double> A(m * m), C(m * m, 0.0), CT(m * m, 0.0);   // CT[j * m + i] = C[i * m + j]
        for (size_t i = 0; i < m; i++) {
            rt_dnode b = dn[L[i]];
            for (size_t j = i; j < m; j++) {
                if (j > i) join(b, dn[L[j]]);
                A[i * m + j] = area(b);
            }
        }
        split.assign(m * m, 0);
        for (size_t len = 2; len <= m; len++) {
            for (size_t i = 0; i + len <= m; i++) {
                const size_t j = i + len - 1;
                double best = INFINITY;
                uint32_t bk = (uint32_t)i;
                const double* row = &C[i * m];
                const double* col = &CT[j * m + 1];   // col[k] = C[(k + 1) * m + j]
                // Knuth's window: the best split of [i, j] between those of [i, j - 1] and [i + 1, j]
                // (exact when the costs satisfy the quadrangle inequality; any split is exact for the
                // walk, so a window that misses the optimum only costs node tests): O(leaves^2)
                size_t k0 = i, k1 = j - 1;
                if (len > 2) {
                    k0 = std::max<size_t>(i, split[i * m + j - 1]);
                    k1 = std::min<size_t>(j - 1, split[(i + 1) * m + j]);
                    if (k0 > k1) {
                        k0 = i;
                        k1 = j - 1;
                    }
                }
                for (size_t k = k0; k <= k1; k++) {
                    const double c = row[k] + col[k];
                    if (c < best) {
                        best = c;
                        bk = (uint32_t)k;
                    }
                }
                C[i * m + j] = CT[j * m + i] = A[i * m + j] + best;
                split[i * m + j] = bk;
            }
        }
    }
    // pre-order emission: (range, slot); a node's first child follows it, its skip is the slot
    // after its subtree (2 x leaves - 1 slots), RT_NODE_END past the last
    struct Item { uint32_t i, j, at; };
    std::vector<Item> st{{0u, (uint32_t)m, 0u}};
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const uint32_t cnt = it.j - it.i, end = it.at + 2 * cnt - 1;
        const uint32_t skip = end >= 2 * m - 1 ? RT_NODE_END : end;
        if (cnt == 1) {
            rt_dnode d = dn[L[it.i]];
            d.meta = (d.meta & ~0xFFFFu) | skip;
            out[it.at] = d;
            continue;
        }
        for (uint32_t t = 0; t < cnt; t++) {
            pre[t] = dn[L[it.i + t]];
            if (t) join(pre[t], pre[t - 1]);
        }
        for (uint32_t t = cnt; t-- > 0;) {
            suf[t] = dn[L[it.i + t]];
            if (t + 1 < cnt) join(suf[t], suf[t + 1]);
        }
        uint32_t best = 1;
        double best_c = INFINITY;
        if (!split.empty()) {
            best = split[(size_t)it.i * m + (it.j - 1)] - it.i + 1;
            best_c = 0.0;
        }
        for (uint32_t s = 1; s < cnt && split.empty(); s++) {
            const double cst = area(pre[s - 1]) * s + area(suf[s]) * (cnt - s);
            if (cst < best_c) {
                best_c = cst;
                best = s;
            }
        }
        rt_dnode d = pre[cnt - 1];
        d.meta = skip;   // inner: no prim types
        d.prims = 0;
        out[it.at] = d;
        const uint32_t first_at = it.at + 1, second_at = it.at + 1 + (2 * best - 1);
        st.push_back({it.i + best, it.j, second_at});
        st.push_back({it.i, it.i + best, first_at});
    }
    return out;
}

// Node collapse (option collapse): which inner nodes the link walk leaves out.  When every node's
// box holds its children's (boxes_nest) and no box is flat, a walk that skips an inner node's test
// and tests its children where it stood tests the same leaves in the same order under the same
// ray_t: where the reference's test of the node misses, its children's tests miss too -- per axis
// the slab values are monotone in the plane coordinates (rounding is monotone; with a component
// of 1/dir infinite the fast form passes an axis only for o strictly inside the slab, the exact
// form (rt_kernel_common.h slab) only for o inside or on it, both monotone under nesting) and the
// interval test is monotone in ray_t.max, which only shrinks between a node and its later
// children -- and so on down to the leaf nodes, which are always kept.  Only the number of node
// tests changes: leaving node N out saves its V(N) tests and costs each child V(N) - H(N) more,
// where H(N), the tests of N that hit, does not depend on the other choices and V(N) = H of N's
// nearest kept ancestor.  H is counted over a 128 x 72 grid of the camera's rays (pixel centres,
// ray_t [0.001, inf), boxes only: the host traces no prims) and the least-tests choice for those
// counts taken by a dynamic programme over the tree; the root stays (the walk starts there).
// tools/node_collapse_study.py: on scene 8 this grid's choice cuts the node tests of the
// reference's own walks by 11.5% beyond the spine (the best choice for the walks themselves: 16%).
std::vector<uint8_t> plan_from_hits(const std::vector<rt_dnode>& dn, const std::vector<int64_t>& H, int64_t walks);
std::vector<uint8_t> plan_collapse(const std::vector<rt_dnode>& dn, const rt_camera_ubo& cam, int width, int height) {
    const size_t n = dn.size();
    std::vector<uint8_t> drop(n, 0);
    if (n <= RT_SMALL_TREE || n > RT_LINK_MAX_NODES || width <= 0 || height <= 0 || !boxes_nest(dn)) return drop;
    for (const rt_dnode& d : dn)
        if (!(d.xmin < d.xmax && d.ymin < d.ymax && d.zmin < d.zmax)) return drop;
    auto is_leaf = [&](size_t k) { return (dn[k].meta & 0xF0000u) != 0; };
    const int gx = 128, gy = 72;
    std::vector<int64_t> H(n, 0);
    for (int j = 0; j < gy; j++) {
        for (int i = 0; i < gx; i++) {
            const float px = ((float)i + 0.5f) * (float)width / (float)gx;
            const float py = ((float)j + 0.5f) * (float)height / (float)gy;
            float o[3], inv[3];
            for (int k = 0; k < 3; k++) {
                o[k] = cam.camera_pos[k];
                inv[k] = 1.0f / (cam.up_left[k] + cam.pixel_delta_u[k] * px + cam.pixel_delta_v[k] * py - o[k]);
            }
            uint32_t k = 0;
            while (k < n) {
                const rt_dnode& b = dn[k];
                const float lo3[3] = {b.xmin, b.ymin, b.zmin}, hi3[3] = {b.xmax, b.ymax, b.zmax};
                float lo = 0.001f, hi = INFINITY;
                for (int a = 0; a < 3; a++) {
                    const float t0 = (lo3[a] - o[a]) * inv[a], t1 = (hi3[a] - o[a]) * inv[a];
                    lo = std::fmax(lo, std::fmin(t0, t1));
                    hi = std::fmin(hi, std::fmax(t0, t1));
                }
                const uint32_t skip = b.meta & 0xFFFFu;
                if (!(hi <= lo)) {
                    H[k]++;
                    k = is_leaf(k) ? skip : k + 1;
                } else {
                    k = skip;
                }
                if (k == RT_NODE_END) break;
            }
        }
    }
    return plan_from_hits(dn, H, (int64_t)gx * gy);
}

// The collapse's dynamic programme for given hit counts H (per node of dn) over `walks` walks
// begun at the root (plan_collapse's grid, or counts measured on the walks themselves by the stats
// twin, rt_debug_set_collapse_hits).
std::vector<uint8_t> plan_from_hits(const std::vector<rt_dnode>& dn, const std::vector<int64_t>& H, int64_t walks) {
    const size_t n = dn.size();
    std::vector<uint8_t> drop(n, 0);
    if (H.size() != n || n <= RT_SMALL_TREE || n > RT_LINK_MAX_NODES || !boxes_nest(dn)) return drop;
    for (const rt_dnode& d : dn)
        if (!(d.xmin < d.xmax && d.ymin < d.ymax && d.zmin < d.zmax)) return drop;
    auto is_leaf = [&](size_t k) { return (dn[k].meta & 0xF0000u) != 0; };
    // cost(k, v): the fewest tests of k's subtree when k's place is reached v times
    std::map<std::pair<uint32_t, int64_t>, std::pair<int64_t, bool>> memo;
    std::function<std::pair<int64_t, bool>(uint32_t, int64_t)> cost = [&](uint32_t k, int64_t v) {
        if (is_leaf(k)) return std::make_pair(v, false);
        const auto key = std::make_pair(k, v);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        const uint32_t r = k + 1, l = dn[k + 1].meta & 0xFFFFu;
        const int64_t keep = v + cost(r, H[k]).first + cost(l, H[k]).first;
        std::pair<int64_t, bool> best(keep, false);
        if (k != 0) {
            const int64_t out = cost(r, v).first + cost(l, v).first;
            if (out < keep) best = std::make_pair(out, true);
        }
        memo.emplace(key, best);
        return best;
    };
    std::vector<std::pair<uint32_t, int64_t>> st{{0u, walks}};
    while (!st.empty()) {
        const auto [k, v] = st.back();
        st.pop_back();
        if (is_leaf(k)) continue;
        const bool out = cost(k, v).second;
        drop[k] = out ? 1 : 0;
        const uint32_t r = k + 1, l = dn[k + 1].meta & 0xFFFFu;
        st.push_back({r, out ? v : H[k]});
        st.push_back({l, out ? v : H[k]});
    }
    return drop;
}

// The default walk round threshold (option walk_frac 0): a round's node walk stops once this
// many 64ths of its lanes hold a leaf or ended.  Measured per scene (round 4,
// profiles/r04_knobs*_s*.log; the default was 48 for every scene): the 7-node Cornell boxes
// want short rounds (scene 6: 8..16 -6%, scene 7: 8 -8.6%, 16 -2.5%), scene 0's 511 nodes 32..36
// (-1.3%), scene 8's 1793 nodes 48..52 (44: +0.4%); a two-level launch takes 32 (LDS plan below).
// Rounds only regroup which lanes walk and
// test leaves together: every lane's node and prim sequence is unchanged (bit-identical).
int walk_frac_for(int n_nodes) { return n_nodes <= RT_SMALL_TREE ? 8 : n_nodes <= 1024 ? 32 : 48; }

// The default number of one-frame chunks that end a staged launch (option tail_chunks -1): the units
// the grid claims last are then 64 samples, so its waves finish closer together.  Measured (round 6,
// profiles/r06_l_opts_s*.log, r06_m_opts_s*.log): scene 8 (1793 nodes) -0.9% with one (+0.6% with 4,
// +3.5% with 8: a short unit's claim and set-up cost more than the imbalance), scene 0 (511 nodes)
// +0.4%, scene 6 +0.2%; so one above 1024 nodes, none otherwise.  Only the grouping of samples into
// units changes (bit-identical; tests/test_gpu_fullsize.py gates 0 and 7 at 1080p).
int tail_chunks_for(int n_nodes) { return n_nodes > 1024 ? 1 : 0; }

// The spine of the link-format walk (rt_kernel.hip spine_entry): every walk starts at the
// root and, while it hits, goes on to the right child (compute.glsl:259-260), so its first
// steps are the chain root, right child, its right child, ... down to the first leaf.  In
// scenes with one huge object (scene 8's fog boundary, r 5000; scene 0's ground, r 1000)
// the builder's sort puts it in the right-most leaf, and every box on the chain contains
// it: for a ray starting inside all of them they are hits, tested on every walk (11 of
// scene 8's ~41 node steps per walk).  Picks the longest prefix of the chain whose boxes'
// intersection holds the camera and >= 3/4 of the leaf boxes' centres (where later walks
// start), at least 3 nodes; its last node's hit successor is where such a walk starts.
// leaf_chain (the first-leaf prologue, rt_kernel.hip render_stream): a prefix that ends at the chain's
// leaf counts from one node on.  The rebuilt tree (rebuild_inner) splits scene 8's fog leaf off at the
// root, so its chain is two nodes -- too short to pay for the entry test by the node steps it
// saves, but with the prologue the walk also leaves out its first round's parked steps and the generic
// leaf stage for that leaf.  The entry's argument holds for any length.
void plan_spine(const std::vector<float4>& L, int n_nodes, const rt_camera_ubo& cam, bool on, bool leaf_chain,
                rt_kernel_args& a) {
    a.spine_len = 0;
    a.spine_start = 0;
    for (int k = 0; k < 3; k++) a.spine_lo[k] = a.spine_hi[k] = 0.0f;
    if (!on || n_nodes <= 0 || L.size() < 2 * (size_t)n_nodes) return;
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    std::vector<float> cx;   // leaf box centres, x y z
    for (int i = 0; i < n_nodes; i++) {
        if ((bits(L[2 * i + 1].z) & RT_LINK_LEAF) == 0) continue;
        cx.push_back(0.5f * (L[2 * i].x + L[2 * i].y));
        cx.push_back(0.5f * (L[2 * i].z + L[2 * i].w));
        cx.push_back(0.5f * (L[2 * i + 1].x + L[2 * i + 1].y));
    }
    const size_t n_leaf = cx.size() / 3;
    if (n_leaf == 0) return;
    float lo[3] = {-INFINITY, -INFINITY, -INFINITY}, hi[3] = {INFINITY, INFINITY, INFINITY};
    uint32_t at = 0;
    for (int len = 1; len <= n_nodes; len++) {
        const float4 b0 = L[2 * (at / 32)], b1 = L[2 * (at / 32) + 1];
        const float blo[3] = {b0.x, b0.z, b1.x}, bhi[3] = {b0.y, b0.w, b1.y};
        for (int k = 0; k < 3; k++) {
            lo[k] = std::max(lo[k], blo[k]);
            hi[k] = std::min(hi[k], bhi[k]);
        }
        float big = 0.0f;
        bool finite = true;
        for (int k = 0; k < 3; k++) {
            finite = finite && std::isfinite(lo[k]) && std::isfinite(hi[k]);
            big = std::max(big, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
        }
        if (!finite) break;
        const float sh = std::ldexp(big, -18);
        float slo[3], shi[3];
        bool ok = true;
        for (int k = 0; k < 3; k++) {
            slo[k] = lo[k] + sh;
            shi[k] = hi[k] - sh;
            ok = ok && slo[k] < shi[k] && slo[k] < cam.camera_pos[k] && cam.camera_pos[k] < shi[k];
        }
        if (!ok) break;   // the intersection only shrinks along the chain
        size_t in = 0;
        for (size_t j = 0; j < n_leaf; j++)
            in += cx[3 * j] > slo[0] && cx[3 * j] < shi[0] && cx[3 * j + 1] > slo[1] && cx[3 * j + 1] < shi[1] &&
                  cx[3 * j + 2] > slo[2] && cx[3 * j + 2] < shi[2];
        if (4 * in < 3 * n_leaf) break;
        const uint32_t hit = bits(b1.z);
        if (len >= 3 || (leaf_chain && (hit & RT_LINK_LEAF) != 0 && hit != RT_LINK_END)) {
            a.spine_len = len;
            a.spine_start = hit;
            for (int k = 0; k < 3; k++) {
                a.spine_lo[k] = slo[k];
                a.spine_hi[k] = shi[k];
            }
        }
        if (hit & RT_LINK_LEAF) break;   // the chain's leaf: the walk leaves with it
        if (hit / 32 >= (uint32_t)n_nodes) break;
        at = hit;
    }
}

// ---- exact near-first walk (variant 60; rt_kernel.hip trace_fast) -------------
// Built from the reference's threaded BVH (thread_bvh):
//  * a SAH tree over the BVH's solid prims (sphere / quad / box), each item
//    bounded by its REFERENCE LEAF box, so every SAH box contains the leaf
//    boxes below it (joins are exact min/max); binned SAH, <= 2 prims a leaf;
//  * that tree laid out 8 times as a threaded pre-order with the near child
//    first for each ray-direction octant (a negative direction on the split
//    axis visits the upper child first): the stackless walk, ordered;
//  * per solid prim its reference rank (2 * leaf ordinal + slot: the order in
//    which the reference tests prims) and its reference leaf node;
//  * the media slots in the reference order; a slot with solids ranked before
//    it gets a tracker k (the closest such solid is its ray_t.max), and meta
//    bit 24 + k marks the SAH subtrees holding solids ranked before it.
// Eligibility (ok): every quad / box face is axis-aligned, so plane hits are
// exact to a few ulps (the kernel's windows rely on it); <= 4 media slots,
// <= 2 trackers, every index in range.  The caller adds the box nesting and
// the no-image-texture-on-media conditions.
struct FastItem {
    float lo[3], hi[3], c[3];
    int type, idx, rank;
};
struct FastNode {
    float lo[3], hi[3];
    int kid[2];
    int axis, first, count, min_rank;
};

int fast_build_node(std::vector<FastItem>& it, int b, int e, std::vector<FastNode>& T) {
    FastNode nd;
    float clo[3], chi[3];
    for (int k = 0; k < 3; k++) {
        nd.lo[k] = clo[k] = INFINITY;
        nd.hi[k] = chi[k] = -INFINITY;
    }
    nd.kid[0] = nd.kid[1] = -1;
    nd.axis = 0;
    nd.first = b;
    nd.count = e - b;
    nd.min_rank = INT_MAX;
    for (int i = b; i < e; i++) {
        for (int k = 0; k < 3; k++) {
            nd.lo[k] = std::min(nd.lo[k], it[i].lo[k]);
            nd.hi[k] = std::max(nd.hi[k], it[i].hi[k]);
            clo[k] = std::min(clo[k], it[i].c[k]);
            chi[k] = std::max(chi[k], it[i].c[k]);
        }
        nd.min_rank = std::min(nd.min_rank, it[i].rank);
    }
    const int id = (int)T.size();
    T.push_back(nd);
    if (e - b <= 2) return id;
    constexpr int NB = 16;
    auto area = [](const float* lo, const float* hi) {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    auto bin_of = [&](const FastItem& q, int ax) {   // a non-finite centroid (uploaded NaN / inf) to an end bin
        const float f = (q.c[ax] - clo[ax]) / (chi[ax] - clo[ax]) * NB;
        return f >= (float)NB ? NB - 1 : (f >= 0.0f ? (int)f : 0);
    };
    float best = INFINITY;
    int bax = -1, bsplit = 0;
    for (int ax = 0; ax < 3; ax++) {
        if (!(chi[ax] - clo[ax] > 0.0f)) continue;
        int cnt[NB] = {0};
        float blo[NB][3], bhi[NB][3];
        for (int s = 0; s < NB; s++)
            for (int k = 0; k < 3; k++) {
                blo[s][k] = INFINITY;
                bhi[s][k] = -INFINITY;
            }
        for (int i = b; i < e; i++) {
            const int s = bin_of(it[i], ax);
            cnt[s]++;
            for (int k = 0; k < 3; k++) {
                blo[s][k] = std::min(blo[s][k], it[i].lo[k]);
                bhi[s][k] = std::max(bhi[s][k], it[i].hi[k]);
            }
        }
        float lA[NB], llo[3] = {INFINITY, INFINITY, INFINITY}, lhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        int lN[NB], n = 0;
        for (int s = 0; s < NB; s++) {
            n += cnt[s];
            for (int k = 0; k < 3; k++) {
                llo[k] = std::min(llo[k], blo[s][k]);
                lhi[k] = std::max(lhi[k], bhi[s][k]);
            }
            lN[s] = n;
            lA[s] = n ? area(llo, lhi) : 0.0f;
        }
        float rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        int rn = 0;
        for (int s = NB - 1; s >= 1; s--) {   // bins < s left, >= s right
            rn += cnt[s];
            for (int k = 0; k < 3; k++) {
                rlo[k] = std::min(rlo[k], blo[s][k]);
                rhi[k] = std::max(rhi[k], bhi[s][k]);
            }
            const int ln = lN[s - 1];
            if (ln == 0 || rn == 0) continue;
            const float cost = lA[s - 1] * ln + area(rlo, rhi) * rn;
            if (cost < best) {
                best = cost;
                bax = ax;
                bsplit = s;
            }
        }
    }
    int mid = b;
    if (bax >= 0) {
        auto pm = std::partition(it.begin() + b, it.begin() + e,
                                 [&](const FastItem& q) { return bin_of(q, bax) < bsplit; });
        mid = (int)(pm - it.begin());
    }
    if (mid == b || mid == e) {   // coincident centroids: halve the range along the widest axis
        int ax = 0;
        for (int k = 1; k < 3; k++)
            if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
        mid = (b + e) / 2;
        std::nth_element(it.begin() + b, it.begin() + mid, it.begin() + e,
                         [ax](const FastItem& x, const FastItem& y) { return x.c[ax] < y.c[ax]; });
        bax = ax;
    }
    const int l = fast_build_node(it, b, mid, T);
    const int r = fast_build_node(it, mid, e, T);
    T[id].kid[0] = l;
    T[id].kid[1] = r;
    T[id].axis = bax;
    return id;
}

void fast_emit(const std::vector<FastNode>& T, const std::vector<FastItem>& it, int n, int oct, const FastTables& F,
               std::vector<rt_dnode>& out) {
    const int k = (int)out.size();
    out.emplace_back();
    const FastNode& s = T[n];
    rt_dnode d;
    d.xmin = s.lo[0]; d.xmax = s.hi[0];
    d.ymin = s.lo[1]; d.ymax = s.hi[1];
    d.zmin = s.lo[2]; d.zmax = s.hi[2];
    uint32_t bits = 0;
    d.prims = 0;
    for (int t = 0; t < F.fl_n; t++)
        if (s.min_rank < F.fl_rank[t]) bits |= 1u << (24 + t);
    if (s.kid[0] < 0) {
        for (int j = 0; j < s.count; j++) {
            const FastItem& q = it[s.first + j];
            bits |= (uint32_t)q.type << (16 + 4 * j);
            d.prims |= (uint32_t)q.idx << (16 * j);
        }
    } else {
        const int f = (oct >> s.axis) & 1;
        fast_emit(T, it, s.kid[f], oct, F, out);
        fast_emit(T, it, s.kid[1 - f], oct, F, out);
    }
    d.meta = bits | (uint32_t)out.size();   // skip = end of this subtree (END patched by the caller)
    out[k] = d;
}

// Two-child layout of tree T (FastTables::inner2 / leaves2).  Returns false when
// a reference does not fit the 16-bit stack entries.
int fast_ref(const std::vector<FastNode>& T, const std::vector<FastItem>& it, int n, FastTables& F, int depth);
bool fast_two_child(const std::vector<FastNode>& T, const std::vector<FastItem>& it, FastTables& F) {
    F.inner2.clear();
    F.leaves2.clear();
    F.depth = 0;
    fast_ref(T, it, 0, F, 1);
    return F.inner2.size() / 4 < 32768 && F.leaves2.size() <= 32768;
}
int fast_ref(const std::vector<FastNode>& T, const std::vector<FastItem>& it, int n, FastTables& F, int depth) {
    const FastNode& s = T[n];
    F.depth = std::max(F.depth, depth);
    if (s.kid[0] < 0) {
        uint2 lf = make_uint2(0u, 0u);
        for (int j = 0; j < s.count; j++) {
            lf.x |= (uint32_t)it[s.first + j].type << (16 + 4 * j);
            lf.y |= (uint32_t)it[s.first + j].idx << (16 * j);
        }
        F.leaves2.push_back(lf);
        return ~(int)(F.leaves2.size() - 1);
    }
    const int k = (int)(F.inner2.size() / 4);
    F.inner2.resize(F.inner2.size() + 4);
    const int rl = fast_ref(T, it, s.kid[0], F, depth + 1);
    const int rr = fast_ref(T, it, s.kid[1], F, depth + 1);
    const FastNode& L = T[s.kid[0]];
    const FastNode& R = T[s.kid[1]];
    uint32_t bits = 0;
    for (int t = 0; t < F.fl_n; t++) {
        if (L.min_rank < F.fl_rank[t]) bits |= 1u << t;
        if (R.min_rank < F.fl_rank[t]) bits |= 1u << (8 + t);
    }
    float4* o = &F.inner2[4 * (size_t)k];
    o[0] = make_float4(L.lo[0], L.hi[0], L.lo[1], L.hi[1]);
    o[1] = make_float4(L.lo[2], L.hi[2], R.lo[0], R.hi[0]);
    o[2] = make_float4(R.lo[1], R.hi[1], R.lo[2], R.hi[2]);
    float a, b, c;
    std::memcpy(&a, &rl, 4);
    std::memcpy(&b, &rr, 4);
    std::memcpy(&c, &bits, 4);
    o[3] = make_float4(a, b, c, 0.0f);
    return k;
}

FastTables build_fast(const std::vector<rt_dnode>& dn, size_t ns, const rt_quad* quads, size_t nq, const rt_box* boxes,
                      size_t nb) {
    FastTables F;
    auto aligned = [](const rt_quad& q) {
        return (q.normal[0] == 0.0f) + (q.normal[1] == 0.0f) + (q.normal[2] == 0.0f) == 2;
    };
    for (size_t i = 0; i < nq; i++)
        if (!aligned(quads[i])) return F;
    for (size_t i = 0; i < nb; i++)
        for (int f = 0; f < 6; f++)
            if (!aligned(boxes[i].quads[f])) return F;
    F.info.assign(ns + nq + nb, 0xFFFFFFFFu);
    F.base[RT_MODEL_SPHERE] = 0;
    F.base[RT_MODEL_QUAD] = (int)ns;
    F.base[RT_MODEL_BOX] = (int)(ns + nq);
    const size_t count[8] = {0, ns, nq, 0, nb, 0, 0, 0};
    std::vector<FastItem> items;
    int rank = 0;
    bool solid_seen = false;
    for (int k = 0; k < (int)dn.size(); k++) {
        const rt_dnode& nd = dn[k];
        if ((nd.meta & 0xF0000u) == 0) continue;   // inner node
        int prev = 0;
        for (int s = 0; s < 2; s++, rank++) {
            const int ty = (int)((nd.meta >> (16 + 4 * s)) & 0xFu), ix = (int)((nd.prims >> (16 * s)) & 0xFFFFu);
            const bool solid = ty == RT_MODEL_SPHERE || ty == RT_MODEL_QUAD || ty == RT_MODEL_BOX;
            if (solid) {
                if ((size_t)ix >= count[ty] || rank > 0xFFFF) return F;
                uint32_t& w = F.info[F.base[ty] + ix];
                if (w == 0xFFFFFFFFu) {   // a prim listed twice keeps its first (earliest) slot
                    w = ((uint32_t)rank << 16) | (uint32_t)k;
                    FastItem q;
                    q.lo[0] = nd.xmin; q.lo[1] = nd.ymin; q.lo[2] = nd.zmin;
                    q.hi[0] = nd.xmax; q.hi[1] = nd.ymax; q.hi[2] = nd.zmax;
                    for (int a = 0; a < 3; a++) q.c[a] = 0.5f * (q.lo[a] + q.hi[a]);
                    q.type = ty;
                    q.idx = ix;
                    q.rank = rank;
                    items.push_back(q);
                }
                solid_seen = true;
            } else if (ty == RT_MODEL_CONSTANT_MEDIUM) {
                if (F.fm_n == 4) return F;
                int tr = -1;
                if (solid_seen) {
                    if (F.fl_n == 2) return F;
                    tr = F.fl_n++;
                    F.fl_medium[tr] = ix;
                    F.fl_rank[tr] = rank;
                }
                const int j = F.fm_n++;
                F.fm_medium[j] = ix;
                F.fm_leaf[j] = k;
                F.fm_track[j] = tr;
                const bool prev_solid = prev == RT_MODEL_SPHERE || prev == RT_MODEL_QUAD || prev == RT_MODEL_BOX;
                F.fm_flags[j] = (s == 1 && prev == RT_MODEL_CONSTANT_MEDIUM ? 1 : 0) | (s == 1 && prev_solid ? 2 : 0);
            }
            prev = ty;
        }
    }
    if (!items.empty()) {
        std::vector<FastNode> T;
        T.reserve(2 * items.size());
        fast_build_node(items, 0, (int)items.size(), T);
        for (int oct = 0; oct < 8; oct++) {
            std::vector<rt_dnode> out;
            fast_emit(T, items, 0, oct, F, out);
            if (out.size() >= RT_NODE_END) return F;
            for (rt_dnode& d : out)
                if ((d.meta & 0xFFFFu) == out.size()) d.meta = (d.meta & ~0xFFFFu) | RT_NODE_END;
            F.n_per = (int)out.size();
            F.nodes.insert(F.nodes.end(), out.begin(), out.end());
        }
        if (!fast_two_child(T, items, F)) return F;   // the same tree for the stack walk (variant 61)
    }
    F.ok = true;
    return F;
}

// Intersection-only record of one quad face (rt_device.h, RT_DFACE_F4): the
// plane (normal, d) and the 2-D Cramer system of hit_quad (hitting.glsl:90-122)
// with its axis pair and delta precomputed by the same float expressions.
void face_record(const rt_quad& q, float4 out[3]) {
    const float* u = q.u;
    const float* v = q.v;
    float delta;
    int a, b, cs;
    if ((delta = u[0] * v[1] - u[1] * v[0]) != 0.0f) { a = 0; b = 1; cs = 0; }
    else if ((delta = u[0] * v[2] - u[2] * v[0]) != 0.0f) { a = 0; b = 2; cs = 1; }
    else { delta = u[1] * v[2] - u[2] * v[1]; a = 1; b = 2; cs = 2; }
    float csf;
    std::memcpy(&csf, &cs, 4);
    out[0] = make_float4(q.normal[0], q.normal[1], q.normal[2], q.d);
    out[1] = make_float4(q.q[a], q.q[b], u[a], u[b]);
    out[2] = make_float4(v[a], v[b], delta, csf);
}

// The compact record of a box with Box.java's axis-aligned layout (rt_kernel.hip
// box_test_compact, rt_device.h RT_BOXC_F4): its corners mn / mx as its faces' q carry
// them (Box.java:32-37) and its faces' normal components along z, x, y.  The kernel
// rebuilds every value its canonical test reads from these with the operations below;
// the record is kept (out[2].y = 1) only when each rebuilt value equals the one the
// uploaded faces give (face_record, the canonical planes), else the box takes the
// full record path.  Float equality: the sign of a zero is the one freedom, and no
// result depends on it (box_test_compact).
bool compact_box(const rt_quad* Q, float4 out[3]) {
    const float mnx = Q[0].q[0], mny = Q[0].q[1], mxz = Q[0].q[2], mxx = Q[1].q[0], mnz = Q[2].q[2],
                mxy = Q[4].q[1];
    const float sz = Q[0].normal[2], sx = Q[1].normal[0], sy = Q[4].normal[1];
    out[0] = make_float4(mnx, mny, mnz, mxx);
    out[1] = make_float4(mxy, mxz, sz, sx);
    // z: quads[0]'s texture id, w: the sign bits of each face normal's two zero components
    // (bits 2i, 2i+1: components (axis+1)%3, (axis+2)%3 of face i), so the shading can rebuild
    // every face normal's exact bits from the record (rt_kernel.hip boxc_normal)
    uint32_t zmask = 0;
    {
        static const int kAxS[6] = {2, 0, 2, 0, 1, 1};
        for (int i = 0; i < 6; i++)
            for (int j = 1; j <= 2; j++)
                if (std::signbit(Q[i].normal[(kAxS[i] + j) % 3])) zmask |= 1u << (2 * i + j - 1);
    }
    float texf, zmf;
    std::memcpy(&texf, &Q[0].texture_id, 4);
    std::memcpy(&zmf, &zmask, 4);
    out[2] = make_float4(sy, 0.0f, texf, zmf);
    static const int kAx[6] = {2, 0, 2, 0, 1, 1};   // Box.java:32-37 face order: normals along z, x, z, x, y, y
    const float sv[6] = {sz, sx, -sz, -sx, sy, -sy};
    const float qk[6] = {mxz, mxx, mnz, mnx, mxy, mny};
    const float DX = mxx - mnx, DY = mxy - mny, DZ = mxz - mnz;
    auto cs = [](int c) {
        float x;
        std::memcpy(&x, &c, 4);
        return x;
    };
    // box_test_compact's per-face systems (boxc_face)
    const float4 A[6] = {make_float4(mnx, mny, DX, 0.0f), make_float4(mny, mxz, 0.0f, -DZ),
                         make_float4(mxx, mny, -DX, 0.0f), make_float4(mny, mnz, 0.0f, DZ),
                         make_float4(mnx, mxz, DX, 0.0f), make_float4(mnx, mnz, DX, 0.0f)};
    const float4 B[6] = {make_float4(0.0f, DY, DX * DY, cs(0)), make_float4(DY, 0.0f, DZ * DY, cs(2)),
                         make_float4(0.0f, DY, -(DX * DY), cs(0)), make_float4(DY, 0.0f, -(DZ * DY), cs(2)),
                         make_float4(0.0f, -DZ, -(DX * DZ), cs(1)), make_float4(0.0f, DZ, DX * DZ, cs(1))};
    auto same = [](float4 a, float4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; };
    for (int i = 0; i < 6; i++) {
        const rt_quad& q = Q[i];
        const int ax = kAx[i];
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(q.normal[k]) || !std::isfinite(q.q[k]) || !std::isfinite(q.u[k]) || !std::isfinite(q.v[k]))
                return false;
        // the canonical plane: normal (s_i along its axis, zeros elsewhere), d = s_i * q_k
        if (q.normal[ax] != sv[i] || sv[i] == 0.0f || q.normal[(ax + 1) % 3] != 0.0f || q.normal[(ax + 2) % 3] != 0.0f)
            return false;
        if (q.d != sv[i] * qk[i]) return false;
        float4 f[3];
        face_record(q, f);
        uint32_t c0, c1;
        std::memcpy(&c0, &f[2].w, 4);
        std::memcpy(&c1, &B[i].w, 4);
        if (!same(f[1], A[i]) || f[2].x != B[i].x || f[2].y != B[i].y || f[2].z != B[i].z || c0 != c1) return false;
    }
    out[2].y = 1.0f;
    return true;
}

// A box's bounds (dboxes[21..22]): min / max over its faces' corners, rounded to float.
void box_bounds(const rt_quad* Q, float4 out[2]) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < 6; i++)
        for (int k = 0; k < 3; k++)
            for (int cu = 0; cu < 2; cu++)
                for (int cv = 0; cv < 2; cv++) {
                    const double x = (double)Q[i].q[k] + cu * (double)Q[i].u[k] + cv * (double)Q[i].v[k];
                    lo[k] = std::min(lo[k], x);
                    hi[k] = std::max(hi[k], x);
                }
    out[0] = make_float4((float)lo[0], (float)hi[0], (float)lo[1], (float)hi[1]);
    out[1] = make_float4((float)lo[2], (float)hi[2], 0.0f, 0.0f);
}

// A box's 48-byte record (rt_kernel.hip leaf_prims_t): compact (compact_box) or, when its
// faces cannot be rebuilt from one, just its bounds (dboxes[21..22]) for the pre-test.
bool box_record(const rt_quad* Q, const float4 bounds[2], float4 rb[RT_BOXC_F4]) {
    if (compact_box(Q, rb)) return true;
    rb[0] = make_float4(bounds[0].x, bounds[0].z, bounds[1].x, bounds[0].y);
    rb[1] = make_float4(bounds[0].w, bounds[1].y, 0.0f, 0.0f);
    rb[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return false;
}

// The scene side of the shared-reciprocal division regime (rt_kernel.hip rcp_nr /
// div_nr): coordinates within 2^20 (so are the rays' origins and directions: hit
// points, camera rays, scatter and light-sampling directions), a face's delta
// normal within [2^-60, 2^20].
bool fd_coord(float x) { return std::fabs(x) <= 1048576.0f; }
bool fd_face(const float4 f[3]) {
    const float ad = std::fabs(f[2].z);
    return fd_coord(f[0].w) && fd_coord(f[1].x) && fd_coord(f[1].y) && fd_coord(f[1].z) && fd_coord(f[1].w) &&
           fd_coord(f[2].x) && fd_coord(f[2].y) && ad >= 0x1p-60f && ad <= 0x1p20f;
}

// Max |coordinate| a ray origin or hit point can have: every record's reach (sphere
// centre + motion + radius, quad / box corners) and the camera block.
float scene_extent(const rt_sphere* sph, size_t n_sph, const rt_quad* quads, size_t n_quads, const rt_quad* box_faces,
                   size_t n_box_faces, const rt_camera_ubo& cam_ubo) {
    double b = 0.0;
    for (size_t k = 0; k < n_sph; k++) {
        const rt_sphere& sp = sph[k];
        for (int i = 0; i < 3; i++)
            b = std::max(b, std::fabs((double)sp.center1[i]) + std::fabs((double)sp.center_vec[i]) +
                                std::fabs((double)sp.radius));
    }
    const rt_quad* Q[2] = {quads, box_faces};
    const size_t nQ[2] = {n_quads, n_box_faces};
    for (int s = 0; s < 2; s++) {
        for (size_t k = 0; k < nQ[s]; k++) {
            const rt_quad& q = Q[s][k];
            for (int i = 0; i < 3; i++)
                b = std::max(b, std::fabs((double)q.q[i]) + std::fabs((double)q.u[i]) + std::fabs((double)q.v[i]));
        }
    }
    const float* cam = (const float*)&cam_ubo;
    for (int i = 0; i < 28; i++) b = std::max(b, std::fabs((double)cam[i]));
    return b < 1e30 ? (float)b : INFINITY;
}

// The quads' intersection-only records (RT_DFACE_F4 each); true when all are in the fast-division regime.
bool prep_quads(const rt_quad* qs, size_t n_quads, std::vector<float4>& faces) {
    faces.resize(n_quads * RT_DFACE_F4);
    bool fd = true;
    for (size_t k = 0; k < n_quads; k++) {
        face_record(qs[k], &faces[k * RT_DFACE_F4]);
        fd = fd && fd_face(&faces[k * RT_DFACE_F4]);
    }
    return fd;
}

// The boxes' records (a box is 6 consecutive quads): per box the 6 planes first, then the 6 (A, B)
// pairs, then the canonical planes and the bounds (RT_DBOX_F4 float4), and its 48-byte record.
BoxPrep prep_boxes(const rt_quad* qs, size_t n_boxes) {
    BoxPrep P;
    P.faces.resize(n_boxes * RT_DBOX_F4);
    P.boxc.assign(n_boxes * RT_BOXC_F4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t bx = 0; bx < n_boxes; bx++) {
        float4* o = &P.faces[bx * RT_DBOX_F4];
        float sw[12];
        for (int i = 0; i < 6; i++) {
            const rt_quad& Q = qs[bx * 6 + i];
            // the face test solves alpha, beta on the reference's axis pair (face_record);
            // |delta| >= half of |u_a v_b| + |u_b v_a| bounds how far a point it accepts
            // can lie outside the face (a few ulps of the scene's extent)
            const float* u = Q.u;
            const float* v = Q.v;
            int ka = 1, kb = 2;
            if (u[0] * v[1] - u[1] * v[0] != 0.0f) { ka = 0; kb = 1; }
            else if (u[0] * v[2] - u[2] * v[0] != 0.0f) { ka = 0; kb = 2; }
            const double t1 = (double)u[ka] * v[kb], t2 = (double)u[kb] * v[ka];
            if (!(std::fabs(t1 - t2) >= 0.5 * (std::fabs(t1) + std::fabs(t2))) || t1 == t2)
                P.cond = false;
        }
        box_bounds(qs + bx * 6, o + 21);
        for (int i = 0; i < 6; i++) {
            float4 f[3];
            face_record(qs[bx * 6 + i], f);
            P.fd = P.fd && fd_face(f);
            o[i] = f[0];
            o[6 + 2 * i] = f[1];
            o[7 + 2 * i] = f[2];
            // Box.java:32-37 face order: normals along z, x, z, x, y, y
            static const int kAx[6] = {2, 0, 2, 0, 1, 1};
            const float* n = qs[bx * 6 + i].normal;
            const int ax = kAx[i];
            if (n[ax] == 0.0f || n[(ax + 1) % 3] != 0.0f || n[(ax + 2) % 3] != 0.0f) P.canon = false;
            sw[2 * i] = n[ax];
            sw[2 * i + 1] = qs[bx * 6 + i].d;
        }
        o[18] = make_float4(sw[0], sw[1], sw[2], sw[3]);
        o[19] = make_float4(sw[4], sw[5], sw[6], sw[7]);
        o[20] = make_float4(sw[8], sw[9], sw[10], sw[11]);
        P.n_compact += box_record(qs + bx * 6, o + 21, &P.boxc[bx * RT_BOXC_F4]);
        // the canonical test shares one reciprocal per axis: opposite faces' normals negated
        if (sw[4] != -sw[0] || sw[6] != -sw[2] || sw[10] != -sw[8]) P.fd = false;
    }
    return P;
}

// The spheres' side of the fast-division regime.
bool spheres_fd(const rt_sphere* sp, size_t n) {
    bool fd = true;
    const float L = 524288.0f;   // center1 + center_vec * time within 2^20
    for (size_t k = 0; k < n; k++)
        for (int i = 0; i < 3; i++)
            fd = fd && std::fabs(sp[k].center1[i]) <= L && std::fabs(sp[k].center_vec[i]) <= L &&
                 std::fabs(sp[k].radius) <= L;
    return fd;
}

// The packed Perlin table (rt_kernel.hip perlin_noise_pk): 256 float4 (ranvec x y z, perm x |
// perm y << 8 | perm z << 16) from an R32F 6 x 256 texture whose perm columns hold whole
// numbers 0..255; false (and pk empty) for any other texture.
bool perlin_pack(const float* t, int w, int h, std::vector<float4>& pk) {
    pk.clear();
    if (!t || w != 6 || h != 256) return false;
    pk.resize(256);
    for (int r = 0; r < 256; r++) {
        uint32_t packed = 0;
        for (int k = 0; k < 3; k++) {
            const float v = t[r * 6 + 3 + k];
            if (!(v >= 0.0f && v <= 255.0f && v == std::floor(v))) {
                pk.clear();
                return false;
            }
            packed |= (uint32_t)v << (8 * k);
        }
        float pf;
        std::memcpy(&pf, &packed, 4);
        pk[r] = make_float4(t[r * 6], t[r * 6 + 1], t[r * 6 + 2], pf);
    }
    return true;
}

// Per mille of the link-format leaves (build_links) that hold two spheres: the sphere-pair
// kernels' criterion (rt_render: at least 500).
int pair_leaves_permille(const std::vector<float4>& L, int n_nodes) {
    size_t n = 0, pairs = 0;
    const size_t nf4 = 2 * (size_t)n_nodes;
    for (int i = 0; i < n_nodes && L.size() > nf4; i++) {
        uint32_t hs;
        std::memcpy(&hs, &L[2 * (size_t)i + 1].z, 4);
        if (!(hs & RT_LINK_LEAF)) continue;
        const size_t ord = hs & 0x7FFFFFFFu;
        if (nf4 + ord / 2 >= L.size()) continue;
        uint32_t w[4];
        std::memcpy(w, &L[nf4 + ord / 2], 16);
        n++;
        pairs += (w[2 * (ord % 2)] & 0xFFu) == (uint32_t)(RT_MODEL_SPHERE | (RT_MODEL_SPHERE << 4));
    }
    return n ? (int)(1000 * pairs / n) : 0;
}

}  // namespace rt_impl
