// nfl_pixel.h -- one uint8 pixel of an image bank as fp32 colour: THE conversion of nfl_gather_batch (training batches)
// and nfl_image_metrics (evaluation), so that a colour scored is bit for bit the colour trained on.
//   c / 255.0f by true division (torchvision's ToTensor); RGBA then rgb * a + (1 - a), every operation rounded on its own
//   (datasets/blender.py:89) -- the translation units that include this are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_macros.h"

// colour of pixel `local` (row-major) of image `im`; returns its alpha code value (255 for an RGB image)
NFL_DEV uint32_t nfl_pixel_rgb(const uint8_t* d_pixels, const nfl_image_rec& im, long long local, float c[3]) {
    if (im.channels == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(d_pixels + im.byte0 + local * 4);
        const float al = (float)(w >> 24) / 255.0f, rest = 1.f - al;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (float)((w >> (8 * k)) & 255u) / 255.0f * al + rest;
        return w >> 24;
    }
    const uint8_t* s = d_pixels + im.byte0 + local * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (float)s[k] / 255.0f;
    return 255u;
}
