// rt_gamma_lut.h — step 2 of Texture.saveAsPNG (Texture.java:89-120), the per-byte gamma table, stated
// once for its two users: image_io.cpp (rts_tonemap_rgb8) and the presented frame (rt.h rt_present: the
// table rt_present_host indexes and rt_present copies to the device).  Host only: the device never
// recomputes it.
//   per byte b: (byte)((float)Math.pow(b / 255.0, 1 / 2.2) * 255.0f)  — double pow, f32 product, truncation.
#pragma once

#include <cmath>
#include <cstdint>

struct rt_gamma_lut {
    uint8_t v[256];
    rt_gamma_lut() {
        for (int b = 0; b < 256; b++) {
            float corrected = (float)std::pow(b / 255.0, 1.0 / 2.2) * 255.0f;
            v[b] = (uint8_t)(int8_t)(int)corrected;
        }
    }
};

// the one table of the library that includes this header (built at its first use)
inline const rt_gamma_lut& rt_gamma_table() {
    static const rt_gamma_lut k;
    return k;
}
