// rt_prep.h — host-only scene preparation (rt_prep.cpp): the threaded and link-format BVH, the
// inner-node rebuild, the collapse and spine plans, the near-first walk's tables, the face / box /
// Perlin records and the stripe arithmetic.  Plain C++: no HIP runtime call, no context.  The
// floats computed here are the ones the kernels consume, so the unit is built once, with the host
// flags of the .hip units (no contraction, no fast-math), and linked into both libraries.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rt/rt.h"
#include "rt/rt_types.h"
#include "rt_device.h"

namespace rt_impl __attribute__((visibility("hidden"))) {

// Tables of the exact near-first walk (build_fast; rt_kernel_variants.hip trace_fast).
struct FastTables {
    bool ok = false;
    std::vector<rt_dnode> nodes;   // 8 octant layouts x n_per threaded nodes
    int n_per = 0;
    std::vector<uint32_t> info;    // per solid prim: reference rank << 16 | reference leaf node
    int base[8] = {0};             // info offset by model type
    int fm_n = 0, fm_medium[4] = {0}, fm_leaf[4] = {0}, fm_track[4] = {0}, fm_flags[4] = {0};
    int fl_n = 0, fl_medium[2] = {0}, fl_rank[2] = {0};
    // the same tree as two-child nodes for the stack walk (variant 61): per inner node 4 float4 =
    // left box, right box, (left ref, right ref, tracker bits left | right << 8, 0); a ref >= 0 is an
    // inner node, ~ref a leaf; a leaf is (meta, prims) as in rt_dnode (types and indices, no skip)
    std::vector<float4> inner2;
    std::vector<uint2> leaves2;
    int depth = 0;   // levels of the tree (the stack walk holds at most depth - 1 entries)
};

// What rt_upload_buffer(RT_BIND_BOXES) derives from the boxes' 6 faces each (prep_boxes).
struct BoxPrep {
    std::vector<float4> faces;   // RT_DBOX_F4 per box (Device::dboxes)
    std::vector<float4> boxc;    // RT_BOXC_F4 per box (Device::dboxc)
    int n_compact = 0;           // boxes whose compact record reproduces their faces
    bool canon = true;           // every box has Box.java's axis-aligned face layout
    bool cond = true;            // every face's 2-D Cramer system is well conditioned
    bool fd = true;              // every face is in the fast-division regime
};

// stripes (rt_set_partition)
int local_rows_of(int h, int rank, int world, int stripe);
int padded_rows_of(int h, int world, int stripe);

// BVH layouts; thread_bvh returns RT_OK or an error code with its text in *err (may be NULL)
int thread_bvh(const rt_bvh_node* in, int n, std::vector<rt_dnode>& out, std::string* err);
bool boxes_nest(const std::vector<rt_dnode>& dn);
std::vector<float4> build_links(const std::vector<rt_dnode>& dn, const std::vector<float>* vbox = nullptr,
                                int* n_nodes_out = nullptr, const std::vector<uint8_t>* drop = nullptr);
std::vector<rt_dnode> rebuild_inner(const std::vector<rt_dnode>& dn, int mode = 1);
std::vector<uint8_t> plan_collapse(const std::vector<rt_dnode>& dn, const rt_camera_ubo& cam, int width, int height);
std::vector<uint8_t> plan_from_hits(const std::vector<rt_dnode>& dn, const std::vector<int64_t>& H, int64_t walks);
int walk_frac_for(int n_nodes);
int tail_chunks_for(int n_nodes);
void plan_spine(const std::vector<float4>& L, int n_nodes, const rt_camera_ubo& cam, bool on, bool leaf_chain,
                rt_kernel_args& a);
int pair_leaves_permille(const std::vector<float4>& L, int n_nodes);
FastTables build_fast(const std::vector<rt_dnode>& dn, size_t ns, const rt_quad* quads, size_t nq, const rt_box* boxes,
                      size_t nb);

// records
void face_record(const rt_quad& q, float4 out[3]);
bool compact_box(const rt_quad* Q, float4 out[3]);
void box_bounds(const rt_quad* Q, float4 out[2]);
bool box_record(const rt_quad* Q, const float4 bounds[2], float4 rb[RT_BOXC_F4]);
bool fd_coord(float x);
bool fd_face(const float4 f[3]);
bool prep_quads(const rt_quad* qs, size_t n_quads, std::vector<float4>& faces);   // returns their fd flag
BoxPrep prep_boxes(const rt_quad* qs, size_t n_boxes);
bool spheres_fd(const rt_sphere* sp, size_t n);
bool perlin_pack(const float* t, int w, int h, std::vector<float4>& pk);
float scene_extent(const rt_sphere* sph, size_t n_sph, const rt_quad* quads, size_t n_quads, const rt_quad* box_faces,
                   size_t n_box_faces, const rt_camera_ubo& cam);

}  // namespace rt_impl
