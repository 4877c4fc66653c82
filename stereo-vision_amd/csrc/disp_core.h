// The 16-bit form of a disparity map (SVH_DISP_U16 of include/svh.h): value x 256 in a uint16, 0 = invalid.  This is the
// encoding of the disparity images of KITTI's stereo benchmark as its development kit documents it; THE CONTRACT IS THE
// RULE BELOW, unverified against the kit's own code (the kit is not part of this project).  Compiled from this one
// header by
//   * hipcc into k_disp_pack_u16 of csrc/disp_kernels.hip,
//   * the host compiler into svh_disparity_unpack_u16 (same file),
//   * g++ into tests/cxx/disp_core_check.cpp, which pins it against the numpy restatement of tests/disp_u16_ref.py.
//
//   u16(d) = 0                                            when !(d >= 0): every negative value, -inf and NaN
//          = max(1, (uint32)min(d * 256.0f, 65535.0f))    otherwise
//   f32(v) = v ? v / 256.0f : -1.0f
//
// d * 256.0f is exact (a power of two; an overflow gives +inf, which the min takes), the conversion truncates, and the
// clamp happens in float BEFORE the conversion: no out-of-range float-to-integer conversion occurs.  -0.0f and 0.0f
// give 1 (a valid disparity of zero must not read as invalid); +inf and every d >= 255.99609375f give 65535.  disp_max
// may exceed 255 (up to 4095): such maps SATURATE at 65535 / 256 in this form.  f32(u16(d)) lies in [d - 1/256, d] for
// 1/256 <= d < 255.99609375f.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DISP_FN __host__ __device__ __forceinline__
#else
#define DISP_FN inline
#endif

namespace svh {
namespace disp {

DISP_FN uint16_t u16(float d) {
    if (!(d >= 0.0f)) return 0;
    const float s = d * 256.0f;
    const float c = s < 65535.0f ? s : 65535.0f;
    const uint32_t v = (uint32_t)c;
    return (uint16_t)(v < 1u ? 1u : v);
}

DISP_FN float f32(uint16_t v) { return v ? (float)v / 256.0f : -1.0f; }

}  // namespace disp
}  // namespace svh
