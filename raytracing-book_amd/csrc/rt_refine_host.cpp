// rt_refine_host.cpp — the host half of the reach records (rt.h rt_reach_tiles): the parameter resolve that
// rt_render_moved_refined uses, rt_tile_reach_host, rt_refine_math.h's functions over a caller array with the
// kernel's butterfly run over a 64-entry array, and rt_refine_select, the pure selection rule.  Plain C++, no
// device.  The noise records' host half likewise: noise_refine_resolve, rt_tile_noise_host and rt_refine_noise_select.
#include <cmath>
#include <cstring>

#include "rt/rt.h"
#include "rt_refine.h"
#include "rt_refine_math.h"

namespace rt_impl {

int refine_resolve(const rt_refine_params* p, rt_rf_resolved* out) {
    out->min_count = 0.0f;
    out->extra_frames = 0;
    out->min_pixels = 1;
    out->max_tiles = 0;
    if (!p) return RT_OK;
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    if (p->extra_frames < 0 || p->min_pixels < 0 || p->min_pixels > 64 || p->max_tiles < 0) return RT_ERR_INVALID_ARG;
    if (!(p->min_count >= 0.0f) || !dn_finite(p->min_count)) return RT_ERR_INVALID_ARG;
    out->min_count = p->min_count;
    out->extra_frames = p->extra_frames;
    out->min_pixels = p->min_pixels ? p->min_pixels : 1;
    out->max_tiles = p->max_tiles;
    return RT_OK;
}

int noise_refine_resolve(const rt_noise_refine_params* p, rt_nz_resolved* out) {
    for (int r : p->reserved)
        if (r != 0) return RT_ERR_INVALID_ARG;
    if (!(p->target_noise >= 0.0f) || !dn_finite(p->target_noise)) return RT_ERR_INVALID_ARG;
    if (!(p->min_count >= 0.0f) || !dn_finite(p->min_count)) return RT_ERR_INVALID_ARG;
    if (p->batch_frames < 1 || p->max_rounds < 0) return RT_ERR_INVALID_ARG;
    out->target_noise = p->target_noise;
    // the fewest frames from which the moments give an estimate, unless the caller names a count
    out->min_count = p->min_count > 0.0f ? p->min_count : 2.0f;
    out->batch_frames = p->batch_frames;
    out->max_rounds = p->max_rounds;
    return RT_OK;
}

}  // namespace rt_impl

extern "C" {

int rt_tile_reach_host(const float* rgbn, int width, int height, float min_count, rt_tile_reach* out, int n_tiles) {
    if (!rgbn || !out || !rf_min_count_ok(min_count)) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
    for (int tile = 0; tile < n_tiles; tile++) {
        float v_min[64], v_sum[64], t_min[64], t_sum[64];
        uint32_t short_px = 0, pixels = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
            const int in = x < width && y < height;
            const float n = in ? rgbn[((size_t)y * width + x) * 4 + 3] : 0.0f;
            const rf_lane l = rf_lane_of(in, n, min_count);
            v_min[lane] = l.v_min;
            v_sum[lane] = l.v_sum;
            short_px += (uint32_t)l.is_short;
            pixels += (uint32_t)in;
        }
        for (int off = 32; off >= 1; off >>= 1) {   // every lane with its partner, as the wave's shuffles do
            for (int lane = 0; lane < 64; lane++) {
                t_sum[lane] = rf_sum_step(v_sum[lane], v_sum[lane ^ off]);
                t_min[lane] = rf_min_step(v_min[lane], v_min[lane ^ off]);
            }
            std::memcpy(v_sum, t_sum, sizeof(v_sum));
            std::memcpy(v_min, t_min, sizeof(v_min));
        }
        out[tile].n_min = v_min[0];
        out[tile].n_sum = v_sum[0];
        out[tile].short_px = short_px;
        out[tile].pixels = pixels;
    }
    return RT_OK;
}

int rt_refine_select(const rt_tile_reach* tiles, int n_tiles, int min_pixels, int max_tiles, uint8_t* active_out,
                     int* n_active) {
    if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !active_out)) || min_pixels < 1 || min_pixels > 64 || max_tiles < 0)
        return RT_ERR_INVALID_ARG;
    int at_least[66] = {0};   // at_least[t]: the tiles with short_px >= t, t in 0 .. 65
    for (int i = 0; i < n_tiles; i++) {
        if (tiles[i].short_px > 64u) return RT_ERR_INVALID_ARG;   // a tile has 64 pixels
        at_least[tiles[i].short_px]++;
    }
    for (int t = 64; t >= 0; t--) at_least[t] += at_least[t + 1];
    int t = min_pixels;
    // a cap: the threshold rises until the tiles at or over it fit; equal counts stay or go together, so no
    // tile's index decides, and at 65 none is left
    if (max_tiles > 0)
        while (at_least[t] > max_tiles) t++;
    for (int i = 0; i < n_tiles; i++) active_out[i] = tiles[i].short_px >= (uint32_t)t ? 1 : 0;
    if (n_active) *n_active = at_least[t];
    return RT_OK;
}

int rt_tile_noise_host(const float* rgbn, const float* s2, int width, int height, float min_count, rt_tile_noise* out,
                       int n_tiles) {
    if (!rgbn || !s2 || !out || !rf_min_count_ok(min_count)) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || width > RT_MAX_IMAGE_DIM || height > RT_MAX_IMAGE_DIM ||
        (size_t)width * height > ((size_t)1 << 30))
        return RT_ERR_INVALID_ARG;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (n_tiles != tiles_x * tiles_y) return RT_ERR_INVALID_ARG;
    for (int tile = 0; tile < n_tiles; tile++) {
        float v[64], yv[64], t_v[64], t_yv[64];
        uint32_t known = 0, thin = 0, bad = 0, pixels = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
            const int in = x < width && y < height;
            const size_t p = in ? (size_t)y * width + x : 0;
            const rf_noise_lane l = in ? rf_noise_lane_of(1, rgbn[p * 4], rgbn[p * 4 + 1], rgbn[p * 4 + 2], rgbn[p * 4 + 3], s2[p], min_count)
                                       : rf_noise_lane_of(0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, min_count);
            v[lane] = l.v;
            yv[lane] = l.yv;
            known += (uint32_t)l.known;
            thin += (uint32_t)l.thin;
            bad += (uint32_t)l.bad;
            pixels += (uint32_t)in;
        }
        for (int off = 32; off >= 1; off >>= 1) {   // every lane with its partner, as the wave's shuffles do
            for (int lane = 0; lane < 64; lane++) {
                t_v[lane] = rf_sum_step(v[lane], v[lane ^ off]);
                t_yv[lane] = rf_sum_step(yv[lane], yv[lane ^ off]);
            }
            std::memcpy(v, t_v, sizeof(v));
            std::memcpy(yv, t_yv, sizeof(yv));
        }
        out[tile].v_sum = v[0];
        out[tile].y_sum = yv[0];
        out[tile].known_px = (uint16_t)known;
        out[tile].thin_px = (uint16_t)thin;
        out[tile].bad_px = (uint16_t)bad;
        out[tile].pixels = (uint16_t)pixels;
    }
    return RT_OK;
}

int rt_refine_noise_select(const rt_tile_noise* tiles, const uint8_t* active_in, int n_tiles, float target,
                           uint8_t* active_out, int* n_active, rt_moved_noise_stats* stats) {
    if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !active_out)) || !(target >= 0.0f) || !dn_finite(target))
        return RT_ERR_INVALID_ARG;
    double sum_v = 0.0, sum_y = 0.0;
    uint64_t known = 0, thin = 0, bad = 0, pixels = 0;
    for (int i = 0; i < n_tiles; i++) {
        const rt_tile_noise& t = tiles[i];
        if (t.known_px > 64 || t.thin_px > 64 || t.bad_px > 64 || t.pixels > 64 || t.known_px + t.bad_px > t.pixels)
            return RT_ERR_INVALID_ARG;   // a tile has 64 pixels, and a known pixel is good
        sum_v += (double)t.v_sum;
        sum_y += (double)t.y_sum;
        known += t.known_px;
        thin += t.thin_px;
        bad += t.bad_px;
        pixels += t.pixels;
    }
    const uint64_t good = pixels - bad;
    const double ybar = good > 0 ? sum_y / (double)good : 0.0;
    const double lim = (double)target * ybar;
    int n = 0;
    for (int i = 0; i < n_tiles; i++) {
        const rt_tile_noise& t = tiles[i];
        const int G = (int)t.pixels - (int)t.bad_px, K = (int)t.known_px;
        int on = (!active_in || active_in[i]) && G > 0;
        // a thin pixel has no estimate, or one from too few samples to trust: it may not stop its tile
        if (on && t.thin_px < 1) on = K > 0 && (double)t.v_sum / (double)K > lim * lim;
        active_out[i] = on ? 1 : 0;
        n += on;
    }
    if (n_active) *n_active = n;
    if (stats) {
        stats->sum_v = sum_v;
        stats->sum_y = sum_y;
        stats->known = known;
        stats->thin = thin;
        stats->bad = bad;
        stats->pixels = pixels;
        stats->rounds = 0;
        stats->converged = 0;
        if (known == 0) stats->noise = INFINITY;
        else if (sum_v == 0.0) stats->noise = 0.0;
        else if (ybar == 0.0) stats->noise = INFINITY;
        else stats->noise = std::sqrt(sum_v / (double)known) / ybar;
    }
    return RT_OK;
}

}  // extern "C"
