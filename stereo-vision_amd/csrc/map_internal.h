// The map-fusion object of csrc/map_kernels.hip, for the one other engine that reads it: the map view takes the two
// point lists of the last frame where they lie (svh_view_add_map, csrc/view_engine.cpp).  Host code only.
#ifndef SVH_MAP_INTERNAL_H
#define SVH_MAP_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "../../include/svh_map.h"
#include "hip_guard.h"

struct svh_map {
    svh_map_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t w = 0, h = 0;            // geometry the buffers are sized for
    int cur = 0;                     // planes [cur], [1 - cur] = previous, swapped every frame
    bool have_prev = false;
    bool last_fused = false;         // the last frame had a previous map to fuse with (else it started a reconstruction)
    int32_t pw = 0, ph = 0;
    struct Bufs {                    // everything sized by the geometry
        svh::HipBuf<float> pl[2][5];         // I, D, X, Y, Z
        svh::HipBuf<float4> pts[2];
        svh::HipBuf<float> dD1;              // staged disparity map when the caller's is on the host
        svh::HipBuf<uint8_t> dI1;
        svh::HipBuf<int32_t> head, next;
        svh::HipBuf<uint8_t> state;
        svh::HipBuf<int32_t> blockcnt;
        svh::PinnedBuf<uint8_t> h_stage;     // packed I1 rows, then D1
    } b;
    svh::PinnedBuf<int64_t> h_total; // point counts of the two lists
    int64_t npts[2] = {0, 0};
};

#endif
