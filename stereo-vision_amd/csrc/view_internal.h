// Between csrc/view_engine.cpp (host) and csrc/view_kernels.hip: one render's launches.
#ifndef SVH_VIEW_INTERNAL_H
#define SVH_VIEW_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "view_core.h"

namespace svh {
namespace view {

struct RenderJob {
    Frame frame;
    const float4* pts;          // the point store: (x, y, z, val), draw index GRID_SEGS + position
    uint32_t npts;
    const Seg* segs;
    uint32_t nseg;
    uint32_t anchor_index;      // NO_ANCHOR: no rotation anchor
    float anchor[3];
    int32_t white;
    unsigned long long* key;    // W * H words, all ones
    uint32_t* ovl;              // W * H words, zero
    uint8_t* rgb;               // W * H * 3 bytes, row 0 = top
};

// points, lines + anchor, resolve on stream `s`; the caller has cleared key and ovl on that stream and checks
// hipGetLastError() afterwards
void launch_render(hipStream_t s, const RenderJob& j);

}  // namespace view
}  // namespace svh
#endif
