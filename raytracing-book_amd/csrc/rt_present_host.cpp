// rt_present_host.cpp — the host half of the presented frame (rt.h rt_present): the parameter resolve that
// rt_present shares with the host function, and rt_present_host, rt_present_math.h's functions over caller
// arrays with rt_gamma_lut.h's table.  Plain C++, no device.
#include <cstring>

#include "rt/rt.h"
#include "rt_gamma_lut.h"
#include "rt_present.h"
#include "rt_present_math.h"

namespace rt_impl {

int present_resolve(const rt_present_params* p, rt_pr_resolved* out) {
    out->source = RT_PRESENT_IMAGE;
    out->exposure = 1.0f;
    out->keep_float = false;
    if (!p) return RT_OK;
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    if (p->source != RT_PRESENT_IMAGE && p->source != RT_PRESENT_DENOISED && p->source != RT_PRESENT_REPROJECTED &&
        p->source != RT_PRESENT_MOVED)
        return RT_ERR_INVALID_ARG;
    if (!(p->exposure > 0.0f) || !dn_finite(p->exposure)) return RT_ERR_INVALID_ARG;
    out->source = p->source;
    out->exposure = p->exposure;
    out->keep_float = p->keep_float != 0;
    return RT_OK;
}

}  // namespace rt_impl

extern "C" int rt_present_host(const float* image, const float* denoised, const float* reprojected, const int32_t* tile_frames,
                               int n_tiles, int width, int height, const rt_present_params* params, uint8_t* rgba8_out,
                               float* rgbw_out) {
    rt_pr_resolved prm;
    if (rt_impl::present_resolve(params, &prm)) return RT_ERR_INVALID_ARG;
    if (!rgba8_out || (prm.keep_float && !rgbw_out)) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const bool moved = prm.source == RT_PRESENT_MOVED;
    const float* src = prm.source == RT_PRESENT_IMAGE ? image : prm.source == RT_PRESENT_DENOISED ? denoised : reprojected;
    if (!src || (moved && (!denoised || !tile_frames))) return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (moved) {
        if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
        for (int t = 0; t < n_tiles; t++)
            if (tile_frames[t] < 0) return RT_ERR_INVALID_ARG;
    }
    const uint8_t* lut = rt_gamma_table().v;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            rt_dn4 c;
            std::memcpy(&c, src + p * 4, sizeof(c));
            if (moved) {
                rt_dn4 D;
                std::memcpy(&D, denoised + p * 4, sizeof(D));
                c = pr_moved(c, D, tile_frames[(size_t)(y >> 3) * tiles_x + (x >> 3)]);
            } else {
                c.w = 1.0f;
            }
            const rt_dn4 e = pr_expose(c, prm.exposure);
            const uint32_t word = pr_pack(e, lut);
            rgba8_out[p * 4 + 0] = (uint8_t)word;
            rgba8_out[p * 4 + 1] = (uint8_t)(word >> 8);
            rgba8_out[p * 4 + 2] = (uint8_t)(word >> 16);
            rgba8_out[p * 4 + 3] = (uint8_t)(word >> 24);
            if (prm.keep_float) std::memcpy(rgbw_out + p * 4, &e, sizeof(e));
        }
    return RT_OK;
}
