// fz_denoise SEED N: random shapes, params and inputs (NaN, inf, negative and huge values; bad
// counts, levels, k and reserved words) through rt_denoise_host (rt_denoise_host.cpp), each buffer
// allocated at its exact size so that a read or write past it is an ASan report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "rt/rt.h"

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 200;
    std::mt19937_64 rng(seed);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    auto flt = [&]() -> float {
        switch (uni(0, 19)) {
            case 0: return std::numeric_limits<float>::quiet_NaN();
            case 1: return std::numeric_limits<float>::infinity();
            case 2: return -std::numeric_limits<float>::infinity();
            case 3: return 3.0e38f;
            case 4: return -1.0f;
            case 5: return 1.0e-42f;
            default: return (float)(rng() % 100000) / 25000.0f;
        }
    };
    int ok = 0, err = 0;
    for (int r = 0; r < rounds; r++) {
        const int W = uni(0, 9) == 0 ? uni(1, 3) : uni(1, 70), H = uni(0, 9) == 0 ? uni(1, 3) : uni(1, 50);
        const int nt = ((W + 7) / 8) * ((H + 7) / 8);
        std::vector<float> img((size_t)W * H * 4), m2(img.size()), out(img.size());
        for (float& v : img) v = flt();
        for (float& v : m2) v = flt();
        std::vector<int32_t> tf((size_t)nt);
        for (int32_t& v : tf) v = uni(0, 29) == 0 ? uni(-2, 1) : uni(2, 4096);
        rt_denoise_params p{};
        p.levels = uni(0, 11) == 0 ? uni(-1, 7) : uni(1, RT_DENOISE_MAX_LEVELS);
        p.k = uni(0, 11) == 0 ? flt() - 1.0f : 0.01f + (float)(rng() % 1000) / 100.0f;
        if (uni(0, 19) == 0) p.reserved[uni(0, 5)] = 1;
        const int n_tiles = uni(0, 19) == 0 ? nt + uni(-1, 1) : nt;
        const int rc = rt_denoise_host(img.data(), m2.data(), tf.data(), n_tiles, W, H, uni(0, 7) == 0 ? nullptr : &p,
                                       out.data());
        if (rc == RT_OK) {
            ok++;
            for (size_t i = 3; i < out.size(); i += 4)
                if (out[i] != 1.0f) {
                    std::printf("round %d: w != 1\n", r);
                    return 1;
                }
        } else if (rc == RT_ERR_INVALID_ARG) {
            err++;
        } else {
            std::printf("round %d: unexpected status %d\n", r, rc);
            return 1;
        }
    }
    std::printf("ok %d err %d\n", ok, err);
    return 0;
}
