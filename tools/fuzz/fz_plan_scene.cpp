// host fuzz driver: mutated scene records (spheres, quads, media, boxes, BVH, lights), camera, mask and
// options through rt_debug_plan_scene -- the uploads' host halves, validation, the walk's trees, the
// kernel arguments, the unit split and the frame counts, as rt_render runs them
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "rt/rt.h"
#include "rt/rt_debug.h"
#include "rt/rt_types.h"
static std::vector<uint8_t> load(const std::string& p) {
    std::vector<uint8_t> b;
    FILE* f = std::fopen(p.c_str(), "rb");
    if (!f) return b;
    int ch;
    while ((ch = std::fgetc(f)) != EOF) b.push_back((uint8_t)ch);
    std::fclose(f);
    return b;
}
static void mutate(std::vector<uint8_t>& b, std::mt19937& rng, size_t rec) {
    if (b.size() < 4) return;
    const int muts = 1 + rng() % 8;
    for (int m = 0; m < muts; m++) {
        const size_t at = (rng() % (b.size() - 3)) & ~(size_t)3;
        switch (rng() % 4) {
        case 0: b[at] = (uint8_t)rng(); break;
        case 1: { uint32_t v = rng() % 2048; std::memcpy(&b[at], &v, 4); break; }
        case 2: { float v = (float)((int)(rng() % 4000) - 2000) * 0.25f; std::memcpy(&b[at], &v, 4); break; }
        case 3: { const uint32_t s[4] = {0x7fc00000u, 0x7f800000u, 0xff800000u, 0x00000001u};
                  std::memcpy(&b[at], &s[rng() % 4], 4); break; }   // NaN, +-inf, a denormal
        }
    }
    if (rng() % 5 == 0 && b.size() > rec) b.resize((b.size() / rec - 1) * rec);
}
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[1];   // DIR/{sph,bvh,quad,med,box,lights,cam}.bin: the six bindings and the camera UBO
    const char* names[6] = {"sph", "bvh", "quad", "med", "box", "lights"};
    const size_t rec[6] = {sizeof(rt_sphere), sizeof(rt_bvh_node), sizeof(rt_quad), sizeof(rt_medium), sizeof(rt_box), 4};
    std::vector<uint8_t> buf0[6];
    for (int b = 0; b < 6; b++) buf0[b] = load(dir + "/" + names[b] + ".bin");
    const auto cam0 = load(dir + "/cam.bin");
    if (cam0.size() != 28 * 4) return 2;
    std::mt19937 rng(std::atoi(argv[2]));
    int ok = 0, err = 0;
    std::vector<int> tiles(48);
    std::vector<uint8_t> links(16 << 20), args(1 << 16);
    static const int opts[][2] = {{RT_OPTION_COMPACT_BOXES, 0}, {RT_OPTION_BOX_PRETEST, 0}, {RT_OPTION_COLLAPSE, 0},
                                  {RT_OPTION_REBUILD, 0}, {RT_OPTION_REBUILD, 1}, {RT_OPTION_SPINE, 0},
                                  {RT_OPTION_FIRST_LEAF, 0}, {RT_OPTION_BOX_VNODES, 0}, {RT_OPTION_LDS_NODE_CAP, 4096},
                                  {RT_OPTION_SPHERE_PAIRS, 2}, {RT_OPTION_BIG_WG, 0}, {RT_OPTION_KERNEL_VARIANT, 37}};
    for (int it = 0; it < std::atoi(argv[3]); it++) {
        std::vector<uint8_t> buf[6];
        for (int b = 0; b < 6; b++) buf[b] = buf0[b];
        auto cam = cam0;
        const int which = rng() % 8;
        if (which < 6) mutate(buf[which], rng, rec[which]);
        if (which == 6) mutate(cam, rng, 4);
        rt_debug_scene_in in;
        std::memset(&in, 0, sizeof in);
        for (int b = 0; b < 6; b++) {
            in.buf[b] = buf[b].empty() ? nullptr : buf[b].data();
            in.buf_bytes[b] = buf[b].size();
        }
        in.camera = (const float*)cam.data();
        in.max_depth = 5;
        in.sqrt_spp = in.recip_sqrt_spp = 1.0f;
        in.width = 64; in.height = 48; in.world = 1 + rng() % 2; in.rank = rng() % in.world; in.stripe_rows = 16;
        const int* o = opts[rng() % (sizeof(opts) / sizeof(opts[0]))];
        in.options = o; in.n_options = rng() % 2; in.ab = rng() % 2;
        in.bvh_mode = rng() % 4 == 0; in.moments = rng() % 2;
        const int mask[3] = {(int)(rng() % 8), 8 + (int)(rng() % 8), 16 + (int)(rng() % 40)};   // (may pass the stripe's tiles)
        in.mask = mask; in.n_mask = (int)(rng() % 5) - 1;
        if (in.n_mask > 3) in.n_mask = 3;
        in.prev_frames = rng() % 4;
        in.first_frame = 1 + rng() % 5; in.n_frames = rng() % 4;
        in.waves = rng() % 3 ? 4096 : rng() % 64; in.free_bytes = rng() % 3 ? (size_t)1 << 38 : rng() % (1 << 20);
        rt_debug_scene_out out;
        std::memset(&out, 0, sizeof out);
        out.tile_frames = tiles.data(); out.tile_cap = (int)tiles.size();
        out.links = links.data(); out.links_cap = links.size();
        out.args = args.data(); out.args_cap = args.size();
        int r = rt_debug_plan_scene(&in, &out);
        if (!r && out.launched) {   // chain into the launch decision, as the tests do
            int pko[RT_PKO_N], info[21];
            r = rt_debug_plan_kernel(out.pk, RT_PK_N, in.ab, pko, RT_PKO_N, info, nullptr, 0, nullptr);
        }
        (r ? err : ok)++;
    }
    std::printf("ok %d err %d\n", ok, err);
}
