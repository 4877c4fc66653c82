// Finished disparity maps in their 16-bit form (csrc/disp_core.h): k_disp_pack_u16, its launcher for the ELAS engine
// (a host caller that asks for SVH_DISP_U16 gets 2 bytes per pixel over PCIe instead of 4) and the stand-alone entries
// svh_disparity_pack_u16 / svh_disparity_unpack_u16 of include/svh.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "disp_core.h"
#include "hip_guard.h"
#include "svh_internal.h"

namespace svh {
namespace {

struct PackTable {
    PackMap m[kPackMaps];
};

__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)disp::u16(a) | (uint32_t)disp::u16(b) << 16; }

// A pure streaming kernel: blockIdx.y = map, eight pixels per lane (two 16-byte loads, one 16-byte store) from the
// destination's first 16-byte boundary on.  The up to 7 elements in front of that boundary and the up to 7 behind the
// last whole vector go one by one (block 0 of the map).  A source that is not 16-byte aligned where the vectors start
// (the two offsets are independent) is read with eight 4-byte loads per lane instead; the choice is uniform per map.
__global__ __launch_bounds__(256) void k_disp_pack_u16(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                       PackTable t) {
    const PackMap m = t.m[blockIdx.y];
    const float* __restrict__ s = src + m.src;
    uint16_t* __restrict__ d = dst + m.dst;
    const long long to_boundary = (long long)(((16 - ((uintptr_t)d & 15)) & 15) / 2);
    const long long head = to_boundary < m.n ? to_boundary : m.n;
    const long long nv = (m.n - head) / 8;
    if (blockIdx.x == 0) {
        if ((long long)threadIdx.x < head) d[threadIdx.x] = disp::u16(s[threadIdx.x]);
        const long long i = head + 8 * nv + ((long long)threadIdx.x - 64);   // lanes 64..70: the tail
        if (threadIdx.x >= 64 && i < m.n) d[i] = disp::u16(s[i]);
    }
    s += head;
    d += head;
    const bool src_vec = ((uintptr_t)s & 15) == 0;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const float* p = s + 8 * v;
        float4 a, b;
        if (src_vec) {
            a = *reinterpret_cast<const float4*>(p);
            b = *reinterpret_cast<const float4*>(p + 4);
        } else {
            a = make_float4(p[0], p[1], p[2], p[3]);
            b = make_float4(p[4], p[5], p[6], p[7]);
        }
        *reinterpret_cast<uint4*>(d + 8 * v) = make_uint4(pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w));
    }
}

}  // namespace

void launch_disp_pack(const LaunchCtx& cx, const float* src, uint16_t* dst, const PackMap* maps, int32_t count) {
    for (int32_t at = 0; at < count; at += kPackMaps) {
        const int32_t c = std::min<int32_t>(kPackMaps, count - at);
        PackTable t{};
        int64_t longest = 0;
        for (int32_t i = 0; i < c; i++) {
            t.m[i] = maps[at + i];
            longest = std::max(longest, t.m[i].n);
        }
        if (longest <= 0) continue;
        // 2048 pixels per block and trip; enough blocks to fill the device, the rest by the stride loop
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((longest + 2047) / 2048, 4096));
        if (cx.prof) cx.prof->begin("k_disp_pack_u16");
        hipLaunchKernelGGL(k_disp_pack_u16, dim3(gx, (unsigned)c), dim3(256), 0, (hipStream_t)cx.stream, src, dst, t);
        if (cx.prof) cx.prof->end();
    }
}

}  // namespace svh

#define DISP_TRY(kind, expr) SVH_HIP_TRY("disparity_pack_u16", kind, expr)
#define DISP_GROW(buf, bytes) SVH_HIP_GROW("disparity_pack_u16", buf, bytes)

extern "C" {

int32_t svh_disparity_pack_u16(const float* D, int32_t d_on_device, int64_t n, uint16_t* out, int32_t out_on_device) {
    if (!D || !out || n < 0) return svh::fail(SVH_ERR_BAD_ARG, "null argument");
    if (n == 0) return SVH_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
    svh::HipBuf<float> dD;
    svh::HipBuf<uint16_t> dU;
    const float* src = D;
    uint16_t* dst = out;
    if (!d_on_device) {
        DISP_GROW(dD, (size_t)n * 4);
        DISP_TRY(copy, hipMemcpy(dD, D, (size_t)n * 4, hipMemcpyHostToDevice));
        src = dD;
    }
    if (!out_on_device) {
        DISP_GROW(dU, (size_t)n * 2);
        dst = dU;
    }
    const svh::PackMap one = {0, 0, n};
    svh::launch_disp_pack(svh::LaunchCtx{nullptr, nullptr}, src, dst, &one, 1);
    DISP_TRY(launch, hipGetLastError());
    if (!out_on_device) DISP_TRY(copy, hipMemcpy(out, dU, (size_t)n * 2, hipMemcpyDeviceToHost));
    else DISP_TRY(wait, hipStreamSynchronize(nullptr));
    return SVH_OK;
}

int32_t svh_disparity_unpack_u16(const uint16_t* v, int64_t n, float* out) {
    if (!v || !out || n < 0) return svh::fail(SVH_ERR_BAD_ARG, "null argument");
    for (int64_t i = 0; i < n; i++) out[i] = svh::disp::f32(v[i]);
    return SVH_OK;
}

}  // extern "C"
