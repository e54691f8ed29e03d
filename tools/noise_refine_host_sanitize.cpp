// noise_refine_host_sanitize.cpp — rt_tile_noise_host and rt_refine_noise_select (rt.h) under the address and
// undefined-behaviour sanitizers: a stand-alone program over csrc/rt_refine_host.cpp alone, CPU only.
// `make -C raytracing-book_amd sanitize-noise-refine` builds it with -fsanitize=address,undefined and runs it.
//
// The inputs are heap arrays of exactly the sizes rt.h states, so a read or a write one element too far is
// caught: 1x1, 8x8 (one whole tile), 9x9 and 13x9 (partial tiles in both directions) and 70x11 (9 tile columns, a
// partial last row), with counts and variances that are plain, NaN, +-inf, negative and 0, and colours that are
// not finite, at three thresholds.  Each record's counts are checked against a plain count of the tile's pixels
// restated here, its sums against a double sum (the terms are not exact in f32, so within a relative 1e-5), and
// the selection against its definition, with and without a mask, and in each of its refusals.
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

bool finite_f(float v) { return std::fabs(v) <= std::numeric_limits<float>::max(); }

bool close_to(double got, double want) { return std::fabs(got - want) <= 1e-5 * std::fabs(want) + 1e-30; }

void run_size(int w, int h, uint32_t seed) {
    const size_t n = (size_t)w * h;
    const int tx = (w + 7) / 8, ty = (h + 7) / 8, nt = tx * ty;
    std::vector<float> rgbn(n * 4), s2(n);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float odd_n[6] = {nan, inf, -inf, -3.0f, 0.0f, -0.0f};
    const float odd_s[6] = {nan, inf, -inf, -1.0f, 0.0f, -0.0f};
    for (size_t p = 0; p < n; p++) {
        for (int c = 0; c < 3; c++) rgbn[p * 4 + c] = (float)(lcg(seed) >> 8) / 16777216.0f;
        const uint32_t r = lcg(seed) >> 16;
        rgbn[p * 4 + 3] = (r % 7 == 0) ? odd_n[(r / 7) % 6] : (float)(1 + r % 70);
        const uint32_t q = lcg(seed) >> 16;
        s2[p] = (q % 5 == 0) ? odd_s[(q / 5) % 6] : (float)(q % 1000) / 250.0f;
        if (q % 11 == 3) rgbn[p * 4 + (q % 3)] = (q & 64) ? nan : inf;
    }
    const float thresholds[3] = {2.0f, 4.0f, 1e9f};
    for (float mc : thresholds) {
        std::vector<rt_tile_noise> out((size_t)nt);
        expect(rt_tile_noise_host(rgbn.data(), s2.data(), w, h, mc, out.data(), nt) == RT_OK, "rt_tile_noise_host returns RT_OK");
        for (int t = 0; t < nt; t++) {
            double sum_v = 0.0, sum_y = 0.0;
            uint32_t known = 0, thin = 0, bad = 0, px = 0;
            for (int ly = 0; ly < 8; ly++)
                for (int lx = 0; lx < 8; lx++) {
                    const int x = (t % tx) * 8 + lx, y = (t / tx) * 8 + ly;
                    if (x >= w || y >= h) continue;
                    const size_t p = (size_t)y * w + x;
                    const float yy = (rgbn[p * 4] + rgbn[p * 4 + 1]) + rgbn[p * 4 + 2], cnt = rgbn[p * 4 + 3], v = s2[p];
                    px++;
                    const bool good = finite_f(yy) && cnt > 0.0f && finite_f(cnt);
                    const bool kn = good && v >= 0.0f && finite_f(v);
                    if (!good) bad++;
                    if (kn) known++;
                    if (good && (!kn || !(cnt >= mc))) thin++;
                    if (kn) sum_v += (double)v / cnt;
                    if (good) sum_y += yy;
                }
            const rt_tile_noise& o = out[(size_t)t];
            expect(o.pixels == px && o.bad_px == bad && o.known_px == known && o.thin_px == thin, "the counts are the tile's");
            expect(close_to(o.v_sum, sum_v) && close_to(o.y_sum, sum_y), "the sums are the tile's");
        }
        // the selection, by its definition, with every tile allowed and with every third one masked out
        std::vector<uint8_t> act((size_t)nt, 9), mask((size_t)nt);
        for (int t = 0; t < nt; t++) mask[(size_t)t] = t % 3 != 1;
        const float targets[4] = {0.0f, 0.05f, 1.0f, std::numeric_limits<float>::max()};
        for (float target : targets)
            for (int masked = 0; masked < 2; masked++) {
                int n_active = -1;
                rt_moved_noise_stats st;
                std::memset(&st, 0xff, sizeof(st));
                expect(rt_refine_noise_select(out.data(), masked ? mask.data() : nullptr, nt, target, act.data(), &n_active, &st) == RT_OK,
                       "rt_refine_noise_select returns RT_OK");
                double sy = 0.0, sv = 0.0;
                uint64_t G = 0, K = 0;
                for (int t = 0; t < nt; t++) {
                    sy += out[(size_t)t].y_sum;
                    sv += out[(size_t)t].v_sum;
                    G += out[(size_t)t].pixels - out[(size_t)t].bad_px;
                    K += out[(size_t)t].known_px;
                }
                const double ybar = G ? sy / (double)G : 0.0, lim = (double)target * ybar;
                int c = 0;
                bool same = true;
                for (int t = 0; t < nt; t++) {
                    const rt_tile_noise& o = out[(size_t)t];
                    const bool want = (!masked || mask[(size_t)t]) && o.pixels > o.bad_px &&
                                      (o.thin_px >= 1 || (o.known_px > 0 && (double)o.v_sum / o.known_px > lim * lim));
                    same = same && act[(size_t)t] == (want ? 1 : 0);
                    c += want;
                }
                expect(same && c == n_active, "the active tiles are the definition's");
                expect(st.sum_v == sv && st.sum_y == sy && st.known == K && st.rounds == 0 && st.converged == 0, "the stats are the sums");
                expect(K == 0 ? std::isinf(st.noise) : (sv == 0.0 ? st.noise == 0.0 : st.noise == std::sqrt(sv / (double)K) / ybar),
                       "the noise figure is the formula's");
            }
    }
    std::vector<rt_tile_noise> out((size_t)nt);
    expect(rt_tile_noise_host(rgbn.data(), s2.data(), w, h, 4.0f, out.data(), nt - 1) == RT_ERR_INVALID_ARG, "a wrong n_tiles is refused");
    expect(rt_tile_noise_host(rgbn.data(), s2.data(), w, h, 0.0f, out.data(), nt) == RT_ERR_INVALID_ARG, "min_count 0 is refused");
    expect(rt_tile_noise_host(rgbn.data(), s2.data(), w, h, std::numeric_limits<float>::quiet_NaN(), out.data(), nt) == RT_ERR_INVALID_ARG,
           "a NaN min_count is refused");
    expect(rt_tile_noise_host(rgbn.data(), nullptr, w, h, 2.0f, out.data(), nt) == RT_ERR_INVALID_ARG, "a NULL s2 is refused");
}

}  // namespace

int main() {
    run_size(1, 1, 5u);
    run_size(8, 8, 3u);
    run_size(9, 9, 4u);
    run_size(13, 9, 1u);
    run_size(70, 11, 2u);
    // the selection's refusals
    const rt_tile_noise fine = {1.0f, 8.0f, 60, 0, 4, 64};
    uint8_t a = 0;
    int n = -1;
    expect(rt_refine_noise_select(&fine, nullptr, 1, 0.1f, &a, &n, nullptr) == RT_OK && n == 1, "a plain record is fine");
    expect(rt_refine_noise_select(&fine, nullptr, 1, 0.1f, &a, nullptr, nullptr) == RT_OK, "n_active and stats may be NULL");
    expect(rt_refine_noise_select(nullptr, nullptr, 0, 0.1f, nullptr, nullptr, nullptr) == RT_OK, "no tiles is fine");
    expect(rt_refine_noise_select(nullptr, nullptr, 1, 0.1f, &a, nullptr, nullptr) == RT_ERR_INVALID_ARG, "NULL tiles are refused");
    expect(rt_refine_noise_select(&fine, nullptr, 1, 0.1f, nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARG, "a NULL active_out is refused");
    expect(rt_refine_noise_select(&fine, nullptr, -1, 0.1f, &a, nullptr, nullptr) == RT_ERR_INVALID_ARG, "a negative n_tiles is refused");
    const float bad_targets[3] = {-1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    for (float t : bad_targets)
        expect(rt_refine_noise_select(&fine, nullptr, 1, t, &a, nullptr, nullptr) == RT_ERR_INVALID_ARG, "a bad target is refused");
    const rt_tile_noise bad[5] = {{0.0f, 1.0f, 65, 0, 0, 65}, {0.0f, 1.0f, 0, 65, 0, 64}, {0.0f, 1.0f, 0, 0, 65, 65},
                                  {0.0f, 1.0f, 1, 0, 0, 65}, {0.0f, 1.0f, 33, 0, 32, 64}};
    for (const rt_tile_noise& b : bad)
        expect(rt_refine_noise_select(&b, nullptr, 1, 0.1f, &a, nullptr, nullptr) == RT_ERR_INVALID_ARG, "counts that cannot be are refused");
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("noise_refine_host_sanitize: ok\n");
    return 0;
}
