// refine_host_sanitize.cpp — rt_tile_reach_host and rt_refine_select (rt.h) under the address and
// undefined-behaviour sanitizers: a stand-alone program over csrc/rt_refine_host.cpp alone, CPU only.
// `make -C raytracing-book_amd sanitize-refine` builds it with -fsanitize=address,undefined and runs it.
//
// The inputs are heap arrays of exactly the sizes rt.h states, so a read or a write one element too far is
// caught: 13x9 (partial tiles in both directions), 70x11 (9 tile columns, a partial last row) and 8x8 (one whole
// tile), with counts that are whole numbers, NaN, +-inf, negative and 0, at three thresholds.  Each record is
// checked against a plain count of the tile's pixels restated here (the sums of whole numbers below 2^24 are exact
// in any order), and the selection against its definition for every min_pixels and a range of caps.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt/rt.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

void run_size(int w, int h, uint32_t seed) {
    const size_t n = (size_t)w * h;
    const int tx = (w + 7) / 8, ty = (h + 7) / 8, nt = tx * ty;
    std::vector<float> rgbn(n * 4);
    const float odd[6] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                          -std::numeric_limits<float>::infinity(), -3.0f, 0.0f, -0.0f};
    for (size_t p = 0; p < n; p++) {
        for (int c = 0; c < 3; c++) rgbn[p * 4 + c] = (float)(lcg(seed) >> 8) / 16777216.0f;
        const uint32_t r = lcg(seed) >> 16;
        rgbn[p * 4 + 3] = (r % 7 == 0) ? odd[(r / 7) % 6] : (float)(1 + r % 70);
    }
    const float thresholds[3] = {1.5f, 4.0f, 1e9f};
    for (float mc : thresholds) {
        std::vector<rt_tile_reach> out((size_t)nt);
        expect(rt_tile_reach_host(rgbn.data(), w, h, mc, out.data(), nt) == RT_OK, "rt_tile_reach_host returns RT_OK");
        for (int t = 0; t < nt; t++) {
            double sum = 0.0;
            float mn = std::numeric_limits<float>::infinity();
            uint32_t shrt = 0, px = 0;
            for (int ly = 0; ly < 8; ly++)
                for (int lx = 0; lx < 8; lx++) {
                    const int x = (t % tx) * 8 + lx, y = (t / tx) * 8 + ly;
                    if (x >= w || y >= h) continue;
                    const float v = rgbn[((size_t)y * w + x) * 4 + 3];
                    px++;
                    if (!(v >= mc)) shrt++;
                    if (v > 0.0f && std::fabs(v) <= std::numeric_limits<float>::max()) {
                        sum += v;
                        if (v < mn) mn = v;
                    }
                }
            expect(out[(size_t)t].pixels == px && out[(size_t)t].short_px == shrt, "the counts are the tile's");
            expect(out[(size_t)t].n_min == mn && (double)out[(size_t)t].n_sum == sum, "the minimum and the sum are the tile's");
        }
        // the selection, by its definition
        std::vector<uint8_t> act((size_t)nt, 9);
        for (int min_pixels = 1; min_pixels <= 64; min_pixels += 9)
            for (int cap = 0; cap <= nt + 1; cap++) {
                int n_active = -1;
                expect(rt_refine_select(out.data(), nt, min_pixels, cap, act.data(), &n_active) == RT_OK, "rt_refine_select returns RT_OK");
                int th = min_pixels;
                if (cap > 0)
                    for (;; th++) {
                        int c = 0;
                        for (int t = 0; t < nt; t++) c += out[(size_t)t].short_px >= (uint32_t)th;
                        if (c <= cap) break;
                    }
                int c = 0;
                bool same = true;
                for (int t = 0; t < nt; t++) {
                    const int want = out[(size_t)t].short_px >= (uint32_t)th;
                    same = same && act[(size_t)t] == want;
                    c += want;
                }
                expect(same && c == n_active && (cap == 0 || c <= cap) && th <= 65, "the active tiles are the definition's");
            }
    }
    std::vector<rt_tile_reach> out((size_t)nt);
    expect(rt_tile_reach_host(rgbn.data(), w, h, 4.0f, out.data(), nt - 1) == RT_ERR_INVALID_ARG, "a wrong n_tiles is refused");
    expect(rt_tile_reach_host(rgbn.data(), w, h, 0.0f, out.data(), nt) == RT_ERR_INVALID_ARG, "min_count 0 is refused");
    expect(rt_tile_reach_host(rgbn.data(), w, h, std::numeric_limits<float>::quiet_NaN(), out.data(), nt) == RT_ERR_INVALID_ARG,
           "a NaN min_count is refused");
}

}  // namespace

int main() {
    run_size(13, 9, 1u);
    run_size(70, 11, 2u);
    run_size(8, 8, 3u);
    rt_tile_reach bad = {1.0f, 1.0f, 65u, 64u};
    uint8_t a = 0;
    expect(rt_refine_select(&bad, 1, 1, 0, &a, nullptr) == RT_ERR_INVALID_ARG, "a short_px over 64 is refused");
    expect(rt_refine_select(nullptr, 0, 1, 0, nullptr, nullptr) == RT_OK, "no tiles is fine");
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("refine_host_sanitize: ok\n");
    return 0;
}
