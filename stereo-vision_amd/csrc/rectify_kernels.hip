// Rectification on the device (stereomapper/framecapturethread.cpp:100-131, 328-349).  The arithmetic is
// rectify_core.h's, no FMA contraction (-ffp-contract=off).
//
// k_rect_maps   once per object and camera: one lane per output pixel evaluates the map entry in fp64, writes the two
//               float maps (kept for the parity tap) and the resident fixed-point table (sx, sy as two int32, 8 bytes
//               per pixel), in which the border mode's reduction of the first tap is already done.
// k_rect_remap  per call, all images of the call in one launch (blockIdx.z = image, .y = rows, .x = columns): a lane
//               produces the four output bytes of one 4-byte-ALIGNED destination word.  Rows of a tightly packed image of
//               odd width start at any address, so the lane's first column is 4 t - (row address & 3): the first and
//               the last word of a row are partial and written byte by byte, every other as one dword.  Per byte: one
//               8-byte table entry, four source taps as plain global loads (neighbouring outputs read neighbouring
//               sources, which the vector L1 and the L2 serve), integer weights.  No float work, no division, no LDS.
//               Byte model per output pixel: 8 B of table in, 1 B out, 1-2 B of source.
// Bounds: every destination store is inside [0, dw) of its row; every source tap is checked against [0, sw) x [0, sh)
// (sample_fixed), whatever the table holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rectify_internal.h"

namespace svh {

namespace {

constexpr int MAPS_T = 256;    // lanes of k_rect_maps
constexpr int RM_LANES = 64;   // k_rect_remap: one wave along a row, 4 bytes per lane = 256 columns ...
constexpr int RM_ROWS = 4;     // ... by four rows per workgroup

__global__ __launch_bounds__(MAPS_T) void k_rect_maps(rect::Cam cam, int32_t sw, int32_t sh, int32_t dw, int32_t dh,
                                                      int32_t border, float* __restrict__ mx, float* __restrict__ my,
                                                      int2* __restrict__ tab) {
    const size_t idx = (size_t)blockIdx.x * MAPS_T + threadIdx.x;
    if (idx >= (size_t)dw * (size_t)dh) return;
    const int32_t i = (int32_t)(idx / (size_t)dw), j = (int32_t)(idx - (size_t)i * (size_t)dw);
    float x, y;
    rect::map_entry(cam, i, j, &x, &y);
    int32_t sx, sy;
    rect::fixed_entry(x, y, sw, sh, border, &sx, &sy);
    mx[idx] = x;
    my[idx] = y;
    tab[idx] = make_int2(sx, sy);
}

__global__ __launch_bounds__(RM_LANES* RM_ROWS) void k_rect_remap(RectRemap a) {
    const int32_t z = (int32_t)blockIdx.z;
    const int32_t pair = z / a.ncam, slot = z - pair * a.ncam;
    const int32_t row = (int32_t)blockIdx.y * RM_ROWS + (int32_t)threadIdx.y;
    if (z >= a.images || row >= a.dh) return;
    const uint8_t* __restrict__ S = a.src[slot] + (size_t)pair * a.src_image_stride;
    uint8_t* __restrict__ drow = a.dst[slot] + (size_t)pair * a.dst_image_stride + (size_t)row * (size_t)a.dst_row_stride;
    const int2* __restrict__ T = reinterpret_cast<const int2*>(a.tab[slot]) + (size_t)row * (size_t)a.dw;
    const int32_t mis = (int32_t)(reinterpret_cast<uintptr_t>(drow) & 3);
    const int32_t c0 = 4 * ((int32_t)blockIdx.x * RM_LANES + (int32_t)threadIdx.x) - mis;   // column of the word's byte 0
    if (c0 >= a.dw) return;
    int2 e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {   // (columns outside the row are computed from the nearest one and not stored)
        const int32_t c = c0 + k;
        e[k] = T[c < 0 ? 0 : (c < a.dw ? c : a.dw - 1)];
    }
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        word |= (uint32_t)rect::sample_fixed(S, a.sw, a.sh, (size_t)a.src_row_stride, a.border, e[k].x, e[k].y) << (8 * k);
    if (c0 >= 0 && c0 + 4 <= a.dw) {
        *reinterpret_cast<uint32_t*>(drow + c0) = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k >= 0 && c0 + k < a.dw) drow[c0 + k] = (uint8_t)(word >> (8 * k));
    }
}

}  // namespace

void rectlaunch_maps(void* stream, const rect::Cam& cam, int32_t sw, int32_t sh, int32_t dw, int32_t dh, int32_t border,
                     float* mx, float* my, int32_t* tab) {
    const size_t n = (size_t)dw * (size_t)dh;
    hipLaunchKernelGGL(k_rect_maps, dim3((unsigned)((n + MAPS_T - 1) / MAPS_T)), dim3(MAPS_T), 0, (hipStream_t)stream,
                       cam, sw, sh, dw, dh, border, mx, my, reinterpret_cast<int2*>(tab));
}

void rectlaunch_remap(void* stream, const RectRemap& a) {
    const int32_t words = (a.dw + 6) / 4;   // 4 t - 3 < dw: the words a row of any alignment touches
    const dim3 grid((unsigned)((words + RM_LANES - 1) / RM_LANES), (unsigned)((a.dh + RM_ROWS - 1) / RM_ROWS),
                    (unsigned)a.images);
    hipLaunchKernelGGL(k_rect_remap, grid, dim3(RM_LANES, RM_ROWS), 0, (hipStream_t)stream, a);
}

}  // namespace svh
