// Between csrc/view2d_engine.cpp (host) and csrc/view2d_kernels.hip: a texel conversion's and a render's launches.
#ifndef SVH_VIEW2D_INTERNAL_H
#define SVH_VIEW2D_INTERNAL_H

#include <hip/hip_runtime_api.h>

#include "view2d_core.h"

namespace svh {
namespace view2d {

enum { SRC_GREY = 0, SRC_RGB_F32 = 1, SRC_DISPARITY = 2 };

// one source (device memory, any byte alignment) into the object's texel store:
//   SRC_GREY       h rows of w bytes, src_pitch apart  ->  h rows of dst_pitch bytes (a multiple of 16, >= w)
//   SRC_RGB_F32    w * h * 3 floats                    ->  w * h RGB8 texels, byte_of of each float
//   SRC_DISPARITY  w * h floats                        ->  w * h RGB8 texels, byte_of of disparity_colour
// The RGB8 store has room for 12 bytes per started group of four texels.
struct TexelJob {
    int32_t kind;
    const void* src;
    int32_t w, h;
    uint32_t src_pitch, dst_pitch;
    uint8_t* dst;
};

struct RenderJob {
    Pane pane;
    const uint8_t* tex;
    const Match* matches;      // n records and n inlier flags; n = 0: the overlay is not touched
    const uint8_t* inlier;
    int32_t n, left;
    uint32_t* ovl;             // W * H words, zero (n > 0)
    uint8_t* rgb;              // W * H * 3 bytes, row 0 = top, any byte alignment
};

// on stream `s`; the caller checks hipGetLastError() afterwards
void launch_texels(hipStream_t s, const TexelJob& j);
void launch_render(hipStream_t s, const RenderJob& j);

}  // namespace view2d
}  // namespace svh
#endif
