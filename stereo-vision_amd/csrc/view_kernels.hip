// The map view on the device (include/svh_view.h; the arithmetic is csrc/view_core.h): a software renderer for the
// accumulated point lists of stereomapper's View3D (view3d.cpp:271-384).
//
// Two layers per render, cleared on the stream before the kernels run:
//   key  one 64-bit word per pixel, depth bits << 32 | draw index, all ones = empty.  GL_LESS with "first drawn wins a
//        tie" is atomicMin on that word, so the winner does not depend on scheduling and a render is reproducible bit
//        for bit.  Every writer reads the word first and skips the atomic when it cannot win: the word only ever
//        decreases, so a stale read can only be too large, never hide a win.
//   ovl  one 32-bit word per pixel for what paintGL draws with the depth test off (cameras, track, axes): the later
//        primitive wins, atomicMax on (order + 1) << 3 | colour code.
// k_view_points streams the point store, one thread and one 16-byte load per point, at most four key updates each;
// k_view_lines takes one lane per segment (a few thousand short ones) plus one for the rotation anchor; k_view_resolve
// turns the two layers into RGB8, gathering a point's grey by its draw index.
#include <hip/hip_runtime.h>

#include "view_core.h"
#include "view_internal.h"

namespace svh {
namespace view {
namespace {

__device__ __forceinline__ void key_min(unsigned long long* key, size_t at, unsigned long long k) {
    if (k < key[at]) atomicMin(&key[at], k);
}

__global__ __launch_bounds__(256) void k_view_points(const float4* __restrict__ pts, uint32_t n, Frame f,
                                                     unsigned long long* __restrict__ key) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    int32_t ix, iy;
    uint32_t zb;
    if (!point_window(f, p.x, p.y, p.z, true, &ix, &iy, &zb)) return;
    const unsigned long long k = ((unsigned long long)zb << 32) | (unsigned long long)(GRID_SEGS + i);
#pragma unroll
    for (int32_t dy = -1; dy <= 0; dy++)
#pragma unroll
        for (int32_t dx = -1; dx <= 0; dx++)
            if (in_image(f, ix + dx, iy + dy)) key_min(key, pixel_index(f, ix + dx, iy + dy), k);
}

struct PlotDepth {
    const Frame& f;
    unsigned long long* key;
    uint32_t index;
    __device__ void operator()(int32_t x, int32_t y, uint32_t zb) {
        key_min(key, pixel_index(f, x, y), ((unsigned long long)zb << 32) | index);
    }
};

struct PlotOverlay {
    const Frame& f;
    uint32_t* ovl;
    uint32_t value;
    __device__ void operator()(int32_t x, int32_t y, uint32_t) {
        const size_t at = pixel_index(f, x, y);
        if (value > ovl[at]) atomicMax(&ovl[at], value);
    }
};

// lanes 0 .. nseg-1: one segment each; lane nseg: the rotation anchor (anchor_index != NO_ANCHOR), a 3 x 3 point at
// (ax, ay, az) that is depth-tested like the points and drawn last
__global__ __launch_bounds__(64) void k_view_lines(const Seg* __restrict__ segs, uint32_t nseg, Frame f,
                                                   unsigned long long* __restrict__ key, uint32_t* __restrict__ ovl,
                                                   uint32_t anchor_index, float ax, float ay, float az) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < nseg) {
        const Seg s = segs[i];
        if (s.flags & SEG_OVERLAY) {
            PlotOverlay plot{f, ovl, s.value};
            raster_segment(f, s, plot);
        } else {
            PlotDepth plot{f, key, s.value};
            raster_segment(f, s, plot);
        }
    } else if (i == nseg && anchor_index != NO_ANCHOR) {
        int32_t ix, iy;
        uint32_t zb;
        if (!point_window(f, ax, ay, az, false, &ix, &iy, &zb)) return;
        const unsigned long long k = ((unsigned long long)zb << 32) | anchor_index;
        for (int32_t dy = -1; dy <= 1; dy++)
            for (int32_t dx = -1; dx <= 1; dx++)
                if (in_image(f, ix + dx, iy + dy)) key_min(key, pixel_index(f, ix + dx, iy + dy), k);
    }
}

__global__ __launch_bounds__(256) void k_view_resolve(const unsigned long long* __restrict__ key,
                                                      const uint32_t* __restrict__ ovl, const float4* __restrict__ pts,
                                                      size_t npix, uint32_t anchor_index, int32_t white,
                                                      uint8_t* __restrict__ rgb) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    resolve_pixel(key[i], ovl[i], anchor_index, (const float*)pts, white != 0, rgb + 3 * i);
}

}  // namespace

void launch_render(hipStream_t s, const RenderJob& j) {
    const size_t npix = (size_t)j.frame.W * (size_t)j.frame.H;
    if (j.npts > 0)
        hipLaunchKernelGGL(k_view_points, dim3((unsigned)((j.npts + 255) / 256)), dim3(256), 0, s, j.pts, j.npts, j.frame, j.key);
    const uint32_t lanes = j.nseg + (j.anchor_index != NO_ANCHOR ? 1u : 0u);
    if (lanes > 0)
        hipLaunchKernelGGL(k_view_lines, dim3((lanes + 63) / 64), dim3(64), 0, s, j.segs, j.nseg, j.frame, j.key, j.ovl,
                           j.anchor_index, j.anchor[0], j.anchor[1], j.anchor[2]);
    hipLaunchKernelGGL(k_view_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, j.key, j.ovl, j.pts, npix,
                       j.anchor_index, j.white, j.rgb);
}

}  // namespace view
}  // namespace svh
