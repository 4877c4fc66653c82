// The 2-D panes on the device (include/svh_view2d.h; the arithmetic is csrc/view2d_core.h): a software renderer for
// stereomapper's View2D (view2d.cpp:69-154) -- the image as a nearest-sampled quad, the matches over it.
//
//   k_view2d_texels   takes the copy a glTexImage2D takes: a grey frame at any pitch, a float RGB image or a disparity
//                     map (coloured on the way, stereothread.cpp:117-147) into the object's byte texels.  A source may
//                     start at any byte: only ALIGNED words that hold bytes of the source itself are loaded.
//   k_view2d_matches  one lane per match: its 2-pixel line, then its 5 x 5 point, into the overlay -- one 32-bit word per
//                     pixel, the later primitive the larger word, atomicMax after a plain read that skips the atomic when
//                     it cannot win (the word only ever grows, so a stale read can only be too small, never hide a win).
//                     The winner of a pixel does not depend on scheduling: a render is reproducible bit for bit.
//   k_view2d_resolve  four consecutive pixels of the linear RGB8 image per thread, three 32-bit stores; a match's colour
//                     is gathered from its record.
#include <hip/hip_runtime.h>

#include "view2d_core.h"
#include "view2d_internal.h"

namespace svh {
namespace view2d {
namespace {

__device__ __forceinline__ uint32_t keep_bytes(uint32_t v, int k) {   // the low k bytes of v (k <= 0: none, >= 4: all)
    return k >= 4 ? v : (k <= 0 ? 0u : v & ((1u << (8 * k)) - 1u));
}

// float e of an array that starts at any byte: the aligned word, or the two aligned words, that hold its four bytes
__device__ __forceinline__ float load_f32(const uint8_t* base, size_t e) {
    const uint8_t* p = base + 4 * e;
    const unsigned lead = (unsigned)((uintptr_t)p & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - lead);
    uint32_t v = q[0];
    if (lead) v = __builtin_amdgcn_alignbyte(q[1], v, lead);
    return __uint_as_float(v);
}

__device__ __forceinline__ uint32_t pack4(const uint8_t* b) {
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

__global__ __launch_bounds__(256) void k_view2d_texels(TexelJob a) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (a.kind == SRC_GREY) {
        // one 16-byte chunk of a texel row per thread: the one to five aligned words that hold its source bytes,
        // shifted into place, the bytes beyond w zero
        const uint32_t c16 = a.dst_pitch / 16u;
        if (i >= (size_t)c16 * (size_t)a.h) return;
        const int row = (int)(i / c16), x0 = (int)(i - (size_t)row * c16) * 16;
        const int nv = min(a.w - x0, 16);
        uint4 o = {0u, 0u, 0u, 0u};
        if (nv > 0) {
            const uint8_t* p = (const uint8_t*)a.src + (size_t)row * (size_t)a.src_pitch + x0;
            const unsigned lead = (unsigned)((uintptr_t)p & 3u);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p - lead);
            const int nw = (int)(lead + (unsigned)nv + 3u) >> 2;   // 1..5 words hold bytes p[0 .. nv-1]
            const uint32_t w0 = q[0];
            const uint32_t w1 = nw > 1 ? q[1] : 0u, w2 = nw > 2 ? q[2] : 0u, w3 = nw > 3 ? q[3] : 0u, w4 = nw > 4 ? q[4] : 0u;
            o.x = keep_bytes(__builtin_amdgcn_alignbyte(w1, w0, lead), nv);
            o.y = keep_bytes(__builtin_amdgcn_alignbyte(w2, w1, lead), nv - 4);
            o.z = keep_bytes(__builtin_amdgcn_alignbyte(w3, w2, lead), nv - 8);
            o.w = keep_bytes(__builtin_amdgcn_alignbyte(w4, w3, lead), nv - 12);
        }
        reinterpret_cast<uint4*>(a.dst)[i] = o;
        return;
    }
    // four texels per thread: 12 bytes, three 32-bit stores; the texels a last group does not have are zero
    const size_t n = (size_t)a.w * (size_t)a.h, e0 = 4 * i;
    if (e0 >= n) return;
    const uint8_t* src = (const uint8_t*)a.src;
    const bool wide = e0 + 4 <= n && ((uintptr_t)src & 15u) == 0;
    uint8_t b[12];
    if (a.kind == SRC_DISPARITY) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (wide) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e0 + k < n) d[k] = load_f32(src, e0 + k);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float c[3];
            disparity_colour(d[k], c);
            const bool have = e0 + k < n;
            b[3 * k + 0] = have ? byte_of(c[0]) : 0, b[3 * k + 1] = have ? byte_of(c[1]) : 0, b[3 * k + 2] = have ? byte_of(c[2]) : 0;
        }
    } else {
        float c[12];
        if (wide) {
            const float4* s4 = reinterpret_cast<const float4*>(src) + 3 * i;
            const float4 v0 = s4[0], v1 = s4[1], v2 = s4[2];
            c[0] = v0.x, c[1] = v0.y, c[2] = v0.z, c[3] = v0.w, c[4] = v1.x, c[5] = v1.y, c[6] = v1.z, c[7] = v1.w;
            c[8] = v2.x, c[9] = v2.y, c[10] = v2.z, c[11] = v2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) c[k] = e0 + k / 3 < n ? load_f32(src, 3 * e0 + k) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 12; k++) b[k] = byte_of(c[k]);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(a.dst) + 3 * i;
    out[0] = pack4(b), out[1] = pack4(b + 4), out[2] = pack4(b + 8);
}

struct PlotOverlay {
    const Pane& f;
    uint32_t* ovl;
    __device__ void operator()(int32_t x, int32_t y, uint32_t word) {
        const size_t at = pixel_index(f, x, y);
        if (word > ovl[at]) atomicMax(&ovl[at], word);
    }
};

__global__ __launch_bounds__(64) void k_view2d_matches(Pane f, const Match* __restrict__ m, int32_t n, int32_t left,
                                                       uint32_t* __restrict__ ovl) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= (uint32_t)n) return;
    const Match r = m[i];
    PlotOverlay plot{f, ovl};
    raster_match(f, r, left != 0, i, plot);
}

// ovl == nullptr: no matches, nothing was drawn
__global__ __launch_bounds__(256) void k_view2d_resolve(Pane f, const uint8_t* __restrict__ tex,
                                                        const uint32_t* __restrict__ ovl, const Match* __restrict__ m,
                                                        const uint8_t* __restrict__ inlier, size_t npix,
                                                        uint8_t* __restrict__ rgb) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x, i0 = 4 * g;
    if (i0 >= npix) return;
    const bool full = i0 + 4 <= npix;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    if (ovl) {
        if (full) {
            const uint4 v = reinterpret_cast<const uint4*>(ovl)[g];
            o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i0 + k < npix) o[k] = ovl[i0 + k];
        }
    }
    int32_t py = (int32_t)(i0 / (size_t)f.W), px = (int32_t)(i0 - (size_t)py * (size_t)f.W);
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0;
        if (i0 + k < npix) resolve_pixel(f, tex, o[k], m, inlier, px, py, b + 3 * k);
        if (++px == f.W) px = 0, py++;
    }
    uint8_t* out = rgb + 3 * i0;
    if (full && ((uintptr_t)rgb & 3u) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(out);
        o4[0] = pack4(b), o4[1] = pack4(b + 4), o4[2] = pack4(b + 8);
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (i0 + k / 3 < npix) out[k] = b[k];
    }
}

}  // namespace

void launch_texels(hipStream_t s, const TexelJob& j) {
    const size_t threads = j.kind == SRC_GREY ? (size_t)(j.dst_pitch / 16u) * (size_t)j.h
                                              : ((size_t)j.w * (size_t)j.h + 3) / 4;
    hipLaunchKernelGGL(k_view2d_texels, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, j);
}

void launch_render(hipStream_t s, const RenderJob& j) {
    const size_t npix = (size_t)j.pane.W * (size_t)j.pane.H;
    if (j.n > 0)
        hipLaunchKernelGGL(k_view2d_matches, dim3(((uint32_t)j.n + 63u) / 64u), dim3(64), 0, s, j.pane, j.matches, j.n,
                           j.left, j.ovl);
    hipLaunchKernelGGL(k_view2d_resolve, dim3((unsigned)(((npix + 3) / 4 + 255) / 256)), dim3(256), 0, s, j.pane, j.tex,
                       j.n > 0 ? j.ovl : (const uint32_t*)nullptr, j.matches, j.inlier, npix, j.rgb);
}

}  // namespace view2d
}  // namespace svh
