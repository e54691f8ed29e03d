// rt_reproject_host.cpp — the host half of temporal reprojection (rt.h rt_reproject): the parameter
// resolve and the history view's matrix that rt_history_capture and rt_reproject share with the host
// reference, and rt_reproject_host, rt_reproject_variance_host, rt_reproject_misses_host and
// rt_history_variance_host, rt_reproject_math.h's functions over caller arrays.  Plain C++, no device.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "rt/rt.h"
#include "rt_reproject.h"
#include "rt_reproject_math.h"

namespace rt_impl {

int reproject_resolve(const rt_reproject_params* p, rt_rp_resolved* out) {
    out->cos_min = RT_REPROJECT_DEFAULT_COS_MIN;
    out->kz = RT_REPROJECT_DEFAULT_KZ;
    out->max_history = RT_REPROJECT_DEFAULT_MAX_HISTORY;
    if (!p) return RT_OK;
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    if (!(p->cos_min >= -1.0f && p->cos_min <= 1.0f)) return RT_ERR_INVALID_ARG;
    if (!(p->kz >= 0.0f) || !dn_finite(p->kz)) return RT_ERR_INVALID_ARG;
    if (!(p->max_history > 0.0f) || !dn_finite(p->max_history)) return RT_ERR_INVALID_ARG;
    out->cos_min = p->cos_min;
    out->kz = p->kz;
    out->max_history = p->max_history;
    return RT_OK;
}

// M of rt.h, in double: the inverse of the matrix with columns pixel_delta_u, pixel_delta_v,
// up_left - camera_pos, each entry rounded to f32 once.
int reproject_matrix(const rt_camera_ubo& cam, float M[9]) {
    struct d3 { double x, y, z; };
    const auto cross = [](d3 a, d3 b) { return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
    const d3 c0 = {cam.pixel_delta_u[0], cam.pixel_delta_u[1], cam.pixel_delta_u[2]};
    const d3 c1 = {cam.pixel_delta_v[0], cam.pixel_delta_v[1], cam.pixel_delta_v[2]};
    const d3 c2 = {(double)cam.up_left[0] - (double)cam.camera_pos[0], (double)cam.up_left[1] - (double)cam.camera_pos[1],
                   (double)cam.up_left[2] - (double)cam.camera_pos[2]};
    const d3 r0 = cross(c1, c2), r1 = cross(c2, c0), r2 = cross(c0, c1);
    const double det = (c0.x * r0.x + c0.y * r0.y) + c0.z * r0.z;
    if (det == 0.0 || !std::isfinite(det)) return RT_ERR_INVALID_ARG;
    const d3 rows[3] = {r0, r1, r2};
    for (int k = 0; k < 3; k++) {
        M[3 * k + 0] = (float)(rows[k].x / det);
        M[3 * k + 1] = (float)(rows[k].y / det);
        M[3 * k + 2] = (float)(rows[k].z / det);
    }
    return RT_OK;
}

}  // namespace rt_impl

namespace {

// rt_reproject_host (history_s2, m2, s2_out NULL) and rt_reproject_variance_host over caller arrays;
// MISS: rt_reproject_misses_host, the same loop over rp_pixel_t<VAR, true>
template <bool MISS>
int reproject_host(const float* history_rgbn, const float* history_nd, const float* history_ai, const float* history_s2,
                   const float history_camera[28], const float* image, const float* m2, const int32_t* tile_frames, int n_tiles,
                   const float* normal_depth, const float* albedo_id, const float camera[28], int width, int height,
                   const rt_reproject_params* params, float* rgbn_out, float* s2_out) {
    if (!history_rgbn || !history_nd || !history_ai || !history_camera || !image || !tile_frames || !normal_depth ||
        !albedo_id || !camera || !rgbn_out)
        return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
    for (int t = 0; t < n_tiles; t++)
        if (tile_frames[t] < 0) return RT_ERR_INVALID_ARG;
    rt_rp_resolved prm;
    if (rt_impl::reproject_resolve(params, &prm)) return RT_ERR_INVALID_ARG;
    rt_rp_view V;
    std::memcpy(&V.cam, camera, sizeof(V.cam));
    std::memcpy(&V.cam_h, history_camera, sizeof(V.cam_h));
    if (rt_impl::reproject_matrix(V.cam_h, V.M)) return RT_ERR_INVALID_ARG;
    V.cos_min = prm.cos_min;
    V.kz = prm.kz;
    V.max_history = prm.max_history;
    V.W = width;
    V.H = height;
    const size_t n = (size_t)width * height;
    try {
        // aligned copies of the history (rgbn_out may not alias it: the taps read whole neighbourhoods)
        std::vector<rt_dn4> hc(n), hnd(n), hai(n);
        std::memcpy(hc.data(), history_rgbn, n * sizeof(rt_dn4));
        std::memcpy(hnd.data(), history_nd, n * sizeof(rt_dn4));
        std::memcpy(hai.data(), history_ai, n * sizeof(rt_dn4));
        std::vector<float> hs2;
        if (s2_out) hs2.assign(history_s2, history_s2 + n);
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t p = (size_t)y * width + x;
                rt_dn4 img, nd, ai;
                std::memcpy(&img, image + p * 4, sizeof(img));
                std::memcpy(&nd, normal_depth + p * 4, sizeof(nd));
                std::memcpy(&ai, albedo_id + p * 4, sizeof(ai));
                const int count = tile_frames[(size_t)(y >> 3) * tiles_x + (x >> 3)];
                rt_dn4 o;
                if (s2_out) {
                    float s2;
                    o = rp_pixel_t<true, MISS>(img, count, nd, ai, hc.data(), hnd.data(), hai.data(), V, x, y, m2[p * 4 + 3],
                                               hs2.data(), &s2);
                    s2_out[p] = s2;
                } else {
                    o = rp_pixel_t<false, MISS>(img, count, nd, ai, hc.data(), hnd.data(), hai.data(), V, x, y, 0.0f, nullptr,
                                                nullptr);
                }
                std::memcpy(rgbn_out + p * 4, &o, sizeof(o));
            }
    } catch (const std::bad_alloc&) {
        return RT_ERR_NOMEM;
    }
    return RT_OK;
}

}  // namespace

extern "C" int rt_reproject_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                                 const float history_camera[28], const float* image, const int32_t* tile_frames, int n_tiles,
                                 const float* normal_depth, const float* albedo_id, const float camera[28], int width,
                                 int height, const rt_reproject_params* params, float* rgbn_out) {
    return reproject_host<false>(history_rgbn, history_nd, history_ai, nullptr, history_camera, image, nullptr, tile_frames, n_tiles,
                          normal_depth, albedo_id, camera, width, height, params, rgbn_out, nullptr);
}

extern "C" int rt_reproject_variance_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                                          const float* history_s2, const float history_camera[28], const float* image,
                                          const float* m2, const int32_t* tile_frames, int n_tiles, const float* normal_depth,
                                          const float* albedo_id, const float camera[28], int width, int height,
                                          const rt_reproject_params* params, float* rgbn_out, float* s2_out) {
    if (!history_s2 || !m2 || !s2_out) return RT_ERR_INVALID_ARG;
    return reproject_host<false>(history_rgbn, history_nd, history_ai, history_s2, history_camera, image, m2, tile_frames, n_tiles,
                          normal_depth, albedo_id, camera, width, height, params, rgbn_out, s2_out);
}

extern "C" int rt_reproject_misses_host(const float* history_rgbn, const float* history_nd, const float* history_ai,
                                        const float* history_s2, const float history_camera[28], const float* image,
                                        const float* m2, const int32_t* tile_frames, int n_tiles, const float* normal_depth,
                                        const float* albedo_id, const float camera[28], int width, int height,
                                        const rt_reproject_params* params, float* rgbn_out, float* s2_out) {
    const int given = (history_s2 != nullptr) + (m2 != nullptr) + (s2_out != nullptr);
    if (given != 0 && given != 3) return RT_ERR_INVALID_ARG;
    return reproject_host<true>(history_rgbn, history_nd, history_ai, history_s2, history_camera, image, m2, tile_frames, n_tiles,
                                normal_depth, albedo_id, camera, width, height, params, rgbn_out, s2_out);
}

extern "C" int rt_history_variance_host(const float* image, const float* m2, const int32_t* tile_frames, int n_tiles, int width,
                                        int height, float* s2_out) {
    if (!image || !m2 || !tile_frames || !s2_out) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
    for (int t = 0; t < n_tiles; t++)
        if (tile_frames[t] < 0) return RT_ERR_INVALID_ARG;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            rt_dn4 img;
            std::memcpy(&img, image + p * 4, sizeof(img));
            s2_out[p] = rp_history_s2(img, m2[p * 4 + 3], tile_frames[(size_t)(y >> 3) * tiles_x + (x >> 3)]);
        }
    return RT_OK;
}
