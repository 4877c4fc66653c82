// internal interface between rectify_engine.cpp (host) and rectify_kernels.hip (device)
#ifndef SVH_RECTIFY_INTERNAL_H
#define SVH_RECTIFY_INTERNAL_H
#include <stddef.h>
#include <stdint.h>

#include "rectify_core.h"

namespace svh {

// One remap launch over `images` images: image z belongs to pair z / ncam and camera slot z % ncam; its source starts at
// src[slot] + pair * src_image_stride, its destination at dst[slot] + pair * dst_image_stride, and it reads the
// fixed-point table tab[slot] (dh * dw entries of sx, sy).
struct RectRemap {
    const uint8_t* src[2];
    uint8_t* dst[2];
    const int32_t* tab[2];
    size_t src_image_stride, dst_image_stride;
    int32_t src_row_stride, dst_row_stride;
    int32_t sw, sh, dw, dh;
    int32_t ncam, images, border;
};

// k_rect_maps: float maps mx, my (dh * dw each) and the table (dh * dw pairs) of one camera
void rectlaunch_maps(void* stream, const rect::Cam& cam, int32_t sw, int32_t sh, int32_t dw, int32_t dh, int32_t border,
                     float* mx, float* my, int32_t* tab);
// k_rect_remap
void rectlaunch_remap(void* stream, const RectRemap& a);

}  // namespace svh
#endif
