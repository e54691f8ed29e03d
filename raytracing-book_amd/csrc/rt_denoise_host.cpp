// rt_denoise_host.cpp — the host reference of the preview filter (rt.h rt_denoise_host) and the
// parameter checks it shares with rt_denoise.  Plain C++, no device: rt_denoise_math.h's functions
// over caller arrays, level by level, the way rt_denoise.hip's kernels run them.
#include <cstring>
#include <new>
#include <vector>

#include "rt/rt.h"
#include "rt_denoise.h"
#include "rt_denoise_math.h"

namespace rt_impl {

int denoise_resolve(const rt_denoise_params* p, rt_dn_resolved* out) {
    out->levels = 3;
    out->k = 3.0f;
    if (!p) return RT_OK;
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    if (p->levels < 1 || p->levels > RT_DENOISE_MAX_LEVELS) return RT_ERR_INVALID_ARG;
    if (!(p->k > 0.0f) || !dn_finite(p->k)) return RT_ERR_INVALID_ARG;
    out->levels = p->levels;
    out->k = p->k;
    return RT_OK;
}

int guide_resolve(const rt_guide_params* p, rt_guide_resolved* out) {
    out->kn = RT_GUIDE_DEFAULT_KN;
    out->kz = RT_GUIDE_DEFAULT_KZ;
    out->ka = RT_GUIDE_DEFAULT_KA;
    if (!p) return RT_OK;
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    const float k[3] = {p->kn, p->kz, p->ka};
    for (float v : k)
        if (!(v >= 0.0f) || !dn_finite(v)) return RT_ERR_INVALID_ARG;
    out->kn = p->kn;
    out->kz = p->kz;
    out->ka = p->ka;
    return RT_OK;
}

}  // namespace rt_impl

namespace {

// The levels over level 0 in `a` (b: the other ping-pong buffer), the way run_levels queues them; the
// result as {r, g, b, 1}.  gnd / gai: the guides' aligned copies when guided.
void levels_host(std::vector<rt_dn4>& a, std::vector<rt_dn4>& b, int width, int height, const rt_dn_resolved& prm, bool guided,
                 const rt_dn_guides& G, float* rgba_out) {
    const size_t n = (size_t)width * height;
    std::vector<float> vb(n);
    rt_dn4 *src = a.data(), *dst = b.data();
    for (int lv = 0; lv < prm.levels; lv++) {
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) vb[(size_t)y * width + x] = dn_vb(src, width, height, x, y);
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++)
                dst[(size_t)y * width + x] =
                    guided ? dn_filter_guided(src, vb.data(), width, height, x, y, 1 << lv, prm.k, G)
                           : dn_filter(src, vb.data(), width, height, x, y, 1 << lv, prm.k);
        rt_dn4* t = src;
        src = dst;
        dst = t;
    }
    for (size_t p = 0; p < n; p++) {
        const rt_dn4 o = src[p];
        const float px[4] = {o.x, o.y, o.z, 1.0f};
        std::memcpy(rgba_out + p * 4, px, sizeof(px));
    }
}

// The filter over caller arrays; nd / ai NULL: unguided (rt_denoise_host).
int denoise_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles, const float* nd,
                 const float* ai, int width, int height, const rt_denoise_params* params, const rt_guide_params* guides,
                 float* rgba_out) {
    if (!image || !m2 || !tile_frames || !rgba_out) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
    for (int t = 0; t < n_tiles; t++)
        if (tile_frames[t] < 2) return RT_ERR_INVALID_ARG;
    rt_dn_resolved prm;
    if (rt_impl::denoise_resolve(params, &prm)) return RT_ERR_INVALID_ARG;
    rt_guide_resolved gp = {0.0f, 0.0f, 0.0f};
    if (nd && rt_impl::guide_resolve(guides, &gp)) return RT_ERR_INVALID_ARG;
    const bool guided = nd && dn_guides_on(gp);
    const size_t n = (size_t)width * height;
    try {
        std::vector<rt_dn4> a(n), b(n), gnd, gai;
        if (guided) {
            gnd.resize(n);
            gai.resize(n);
            std::memcpy(gnd.data(), nd, n * sizeof(rt_dn4));
            std::memcpy(gai.data(), ai, n * sizeof(rt_dn4));
        }
        const rt_dn_guides G = {gnd.data(), gai.data(), gp.kn, gp.kz, gp.ka};
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t p = (size_t)y * width + x;
                rt_dn4 img;
                std::memcpy(&img, image + p * 4, sizeof(img));
                a[p] = dn_level0(img, m2[p * 4 + 3], tile_frames[(size_t)(y >> 3) * tiles_x + (x >> 3)]);
            }
        levels_host(a, b, width, height, prm, guided, G, rgba_out);
    } catch (const std::bad_alloc&) {
        return RT_ERR_NOMEM;
    }
    return RT_OK;
}

}  // namespace

extern "C" int rt_denoise_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles, int width,
                               int height, const rt_denoise_params* params, float* rgba_out) {
    return denoise_host(image, m2, tile_frames, n_tiles, nullptr, nullptr, width, height, params, nullptr, rgba_out);
}

extern "C" int rt_denoise_guided_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles,
                                      const float* normal_depth, const float* albedo_id, int width, int height,
                                      const rt_denoise_params* params, const rt_guide_params* guides, float* rgba_out) {
    if (!normal_depth || !albedo_id) return RT_ERR_INVALID_ARG;
    return denoise_host(image, m2, tile_frames, n_tiles, normal_depth, albedo_id, width, height, params, guides,
                        rgba_out);
}

extern "C" int rt_denoise_reprojected_host(const float* rgbn, const float* s2, const float* normal_depth, const float* albedo_id,
                                           int width, int height, const rt_denoise_params* params,
                                           const rt_guide_params* guides, float* rgba_out) {
    if (!rgbn || !s2 || !normal_depth || !albedo_id || !rgba_out) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    rt_dn_resolved prm;
    if (rt_impl::denoise_resolve(params, &prm)) return RT_ERR_INVALID_ARG;
    rt_guide_resolved gp;
    if (rt_impl::guide_resolve(guides, &gp)) return RT_ERR_INVALID_ARG;
    const bool guided = dn_guides_on(gp);
    const size_t n = (size_t)width * height;
    try {
        std::vector<rt_dn4> a(n), b(n), view(n), gnd, gai(n);
        std::memcpy(view.data(), rgbn, n * sizeof(rt_dn4));
        std::memcpy(gai.data(), albedo_id, n * sizeof(rt_dn4));   // level 0 compares the ids, guided or not
        if (guided) {
            gnd.resize(n);
            std::memcpy(gnd.data(), normal_depth, n * sizeof(rt_dn4));
        }
        const rt_dn_guides G = {gnd.data(), gai.data(), gp.kn, gp.kz, gp.ka};
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++)
                a[(size_t)y * width + x] = dn_level0_reprojected(view.data(), s2, gai.data(), width, height, x, y);
        levels_host(a, b, width, height, prm, guided, G, rgba_out);
    } catch (const std::bad_alloc&) {
        return RT_ERR_NOMEM;
    }
    return RT_OK;
}
