// Between csrc/view_engine.cpp (host) and csrc/view_kernels.hip: one render's launches.
#ifndef SVH_VIEW_INTERNAL_H
#define SVH_VIEW_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "view_core.h"

struct svh_view;

namespace svh {
namespace view {

// The point store of a view as it lies on the device, for a consumer inside the library (csrc/grid_engine.cpp): `n` points
// (x, y, z, val), the lists back to back.  Every entry of the view returns when it is complete; a reader on another
// stream waits on `stream` first.  Valid until the next call that changes the view.
struct StoreRef {
    const float4* pts;
    int64_t n;
    int device;
    hipStream_t stream;
};
StoreRef store_of(const svh_view* v);
// the lists first .. first + n_lists - 1 of the sequence as a range of the store: *at points before it, *n points in it;
// false, nothing written: first < 0, n_lists < 0, or the range ends past the view's last list
bool list_range(const svh_view* v, int32_t first, int32_t n_lists, int64_t* at, int64_t* n);

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

// One voxel-grid thinning (csrc/view_thin_kernels.hip; the arithmetic is csrc/view_thin_core.h).  The compaction works
// in blocks of THIN_BLOCK points.
constexpr uint32_t THIN_BLOCK = 1024;
struct ThinJob {
    const float4* pts;          // the store, n points
    uint32_t n;
    float voxel;
    unsigned long long* keys;   // `capacity` slots, all ones
    uint32_t* win;              // `capacity` slots, all ones: the lowest store index that entered the slot's key
    uint64_t capacity;          // thin::capacity_for(n)
    uint32_t* slot;             // n: where a placeable point found its key
    uint8_t* keep;              // n: 1 survivor, 0 removed (2 between the first two kernels: kept without a voxel)
    int32_t* blockcnt;          // ceil(n / THIN_BLOCK): survivors per block, then survivors before the block
    const int64_t* bounds;      // nbounds store positions, ascending, each in [0, n]: the list boundaries
    int32_t nbounds;
    int64_t* out;               // [0] survivors, [1] unplaceable points (zero on entry), [2 + k] survivors before bounds[k]
    float4* dst;                // the second store: the survivors in store order
};
// insert, flag + count, scan, scatter, boundaries on stream `s`; the caller has set keys, win and out[1] on that stream
// and checks hipGetLastError() afterwards
void launch_thin(hipStream_t s, const ThinJob& j);

}  // namespace view
}  // namespace svh
#endif
