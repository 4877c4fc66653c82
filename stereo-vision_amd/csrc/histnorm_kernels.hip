// StereoImage::histogramNormalization on the device (stereomapper/stereoimage.cpp:94-134).  The arithmetic is
// histnorm_core.h's, no FMA contraction (-ffp-contract=off).  Three kernels per call, each ONE launch over all images
// of the call (blockIdx.y = image), in the job form of job_kernel.h:
//
// k_hist_count  exact integer counts.  An image is cut into the 16-byte-ALIGNED windows its rows touch (rows start at
//               any address: a row of w bytes touches at most (w + 30) / 16 windows).  A lane takes one window: a window
//               that lies inside its row is one 16-byte load, the head and the tail of a row are read byte by byte, and
//               nothing outside the rows is read.  Equal neighbours among the 16 bytes are counted in a register first
//               (one LDS add per run, not per byte), and when every lane of the wave ends on the same grey level -- a
//               flat image, where 64 lanes would otherwise queue on one LDS word -- the wave adds its lanes' runs with
//               shuffles and one lane issues one add.  Each wave owns a 256-bin histogram in LDS; the four of a
//               workgroup are summed and the non-empty bins go to the image's 256 global counters with integer
//               atomics.  Integer sums do not depend on the order of arrival.
// k_hist_table  one workgroup per image: 256 lanes evaluate f(count[g]) from the segment table, lane 0 runs the 255
//               dependent additions of the cdf (not associative: serial), 256 lanes write cdf and map.
// k_hist_apply  the same windows; the image's 256-byte table in LDS; 16 bytes per lane read, mapped and written in
//               place, heads and tails byte by byte.  A byte is read and written by one lane only, and no byte
//               between the rows is written.
// Byte model per image of N pixels: 2 N read, N written (+ 2.25 KiB of tables).
// Bounds: every access to an image is inside [0, w) of a row < h; windows past a row's end are skipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "histnorm_internal.h"
#include "job_kernel.h"

namespace svh {

namespace {

constexpr int HN_T = 256;           // lanes of every kernel here
constexpr int HN_PER_LANE = 4;      // windows a lane takes when the image is large enough ...
constexpr unsigned HN_MAX_BLOCKS = 256;   // ... up to this many workgroups per image, which then stride

__device__ __forceinline__ HistJob globalise(HistJob a) {
    all_global(a.img0, a.img1, a.counts, a.cdf, a.map, a.seg);
    return a;
}

__host__ __device__ __forceinline__ unsigned hist_cpr(const HistJob& a) { return (unsigned)(a.w + 30) / 16u; }
__host__ __device__ __forceinline__ unsigned hist_items(const HistJob& a) { return hist_cpr(a) * (unsigned)a.h; }
__host__ __device__ __forceinline__ unsigned hist_blocks(const HistJob& a) {
    const unsigned b = (hist_items(a) + HN_T * HN_PER_LANE - 1) / (HN_T * HN_PER_LANE);
    return b < HN_MAX_BLOCKS ? b : HN_MAX_BLOCKS;
}

__device__ __forceinline__ uint8_t* image_of(const HistJob& a, unsigned z) {
    const unsigned pair = z / (unsigned)a.slots, slot = z - pair * (unsigned)a.slots;
    return (slot ? a.img1 : a.img0) + (size_t)pair * a.image_stride;
}

// window `item` of the image at `base`: its 16 bytes start at p (16-byte aligned); bytes [lo, hi) of it belong to
// the row (hi <= lo: none)
struct Window {
    uint8_t* p;
    int lo, hi;
};
__device__ __forceinline__ Window window_of(const HistJob& a, uint8_t* base, unsigned item, unsigned cpr) {
    const unsigned row = item / cpr, c = item - row * cpr;
    uint8_t* rowp = base + (size_t)row * (size_t)a.row_stride;
    const int start = 16 * (int)c - (int)(reinterpret_cast<uintptr_t>(rowp) & 15);   // column of the window's byte 0
    Window wd;
    wd.p = rowp + start;
    wd.lo = start < 0 ? -start : 0;
    wd.hi = a.w - start < 16 ? a.w - start : 16;
    return wd;
}

__device__ __forceinline__ void d_hist_count(const HistJob& a, unsigned bx, unsigned z) {
    __shared__ int32_t s_h[HN_T / 64][256];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    int32_t* H = s_h[tid >> 6];
#pragma unroll
    for (int w = 0; w < HN_T / 64; w++) s_h[w][tid] = 0;
    __syncthreads();
    uint8_t* base = image_of(a, z);
    const unsigned cpr = hist_cpr(a), items = cpr * (unsigned)a.h, stride = hist_blocks(a) * HN_T;
    for (unsigned first = bx * HN_T; first < items; first += stride) {   // (workgroup-uniform: the waves stay whole)
        const unsigned item = first + tid;
        uint32_t cur = 0, run = 0;   // the lane's last run of equal bytes, added below
        if (item < items) {
            const Window wd = window_of(a, base, item, cpr);
            if (wd.lo == 0 && wd.hi == 16) {
                const uint4 v = *reinterpret_cast<const uint4*>(wd.p);
                const uint32_t q[4] = {v.x, v.y, v.z, v.w};
                cur = q[0] & 255u, run = 1;
#pragma unroll
                for (int k = 1; k < 16; k++) {
                    const uint32_t b = (q[k >> 2] >> (8 * (k & 3))) & 255u;
                    if (b == cur) {
                        run++;
                    } else {
                        atomicAdd(&H[cur], (int32_t)run);
                        cur = b, run = 1;
                    }
                }
            } else {
                for (int k = wd.lo; k < wd.hi; k++) atomicAdd(&H[wd.p[k]], 1);
            }
        }
        const bool has = run > 0;
        const unsigned long long who = __ballot(has);
        if (who) {
            const int src = __ffsll(who) - 1;
            const uint32_t v0 = (uint32_t)__shfl((int)cur, src, 64);
            if (__all(!has || cur == v0)) {   // one grey level ends every lane: one add for the wave
                int total = (int)run;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
                if ((int)lane == src) atomicAdd(&H[v0], total);
            } else if (has) {
                atomicAdd(&H[cur], (int32_t)run);
            }
        }
    }
    __syncthreads();
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < HN_T / 64; w++) sum += s_h[w][tid];
    if (sum) atomicAdd(&a.counts[(size_t)z * 256 + tid], sum);
}
SVH_JOB_KERNEL(kd_hist_count, , k_hist_count, k_hist_count_b, HistJob, HN_T, 1, d_hist_count,
               blockIdx.y < (unsigned)a.images && blockIdx.x < hist_blocks(a))

__device__ __forceinline__ void d_hist_table(const HistJob& a, unsigned, unsigned z) {
    __shared__ float s_p[256], s_cdf[256];
    const unsigned g = threadIdx.x;
    s_p[g] = hn::eval(a.seg, a.nseg, a.counts[(size_t)z * 256 + g]);
    __syncthreads();
    if (g == 0) hn::cdf_chain(s_p, s_cdf);
    __syncthreads();
    const float c = s_cdf[g];
    a.cdf[(size_t)z * 256 + g] = c;
    a.map[(size_t)z * 256 + g] = hn::map_entry(c);
}
SVH_JOB_KERNEL(kd_hist_table, , k_hist_table, k_hist_table_b, HistJob, HN_T, 1, d_hist_table,
               blockIdx.y < (unsigned)a.images && blockIdx.x == 0)

__device__ __forceinline__ uint32_t map4(const uint8_t* M, uint32_t v) {
    return (uint32_t)M[v & 255u] | ((uint32_t)M[(v >> 8) & 255u] << 8) | ((uint32_t)M[(v >> 16) & 255u] << 16) |
           ((uint32_t)M[v >> 24] << 24);
}
__device__ __forceinline__ void d_hist_apply(const HistJob& a, unsigned bx, unsigned z) {
    __shared__ uint32_t s_map[64];
    const unsigned tid = threadIdx.x;
    if (tid < 64) s_map[tid] = reinterpret_cast<const uint32_t*>(a.map + (size_t)z * 256)[tid];
    __syncthreads();
    const uint8_t* M = reinterpret_cast<const uint8_t*>(s_map);
    uint8_t* base = image_of(a, z);
    const unsigned cpr = hist_cpr(a), items = cpr * (unsigned)a.h, stride = hist_blocks(a) * HN_T;
    for (unsigned item = bx * HN_T + tid; item < items; item += stride) {
        const Window wd = window_of(a, base, item, cpr);
        if (wd.lo == 0 && wd.hi == 16) {
            uint4 v = *reinterpret_cast<const uint4*>(wd.p);
            v.x = map4(M, v.x), v.y = map4(M, v.y), v.z = map4(M, v.z), v.w = map4(M, v.w);
            *reinterpret_cast<uint4*>(wd.p) = v;
        } else {
            for (int k = wd.lo; k < wd.hi; k++) wd.p[k] = M[wd.p[k]];
        }
    }
}
SVH_JOB_KERNEL(kd_hist_apply, , k_hist_apply, k_hist_apply_b, HistJob, HN_T, 1, d_hist_apply,
               blockIdx.y < (unsigned)a.images && blockIdx.x < hist_blocks(a))

}  // namespace

void histlaunch_count(void* stream, const HistJob& a) {
    launch_or_record(stream, kd_hist_count, a, dim3(hist_blocks(a), (unsigned)a.images));
}
void histlaunch_table(void* stream, const HistJob& a) {
    launch_or_record(stream, kd_hist_table, a, dim3(1, (unsigned)a.images));
}
void histlaunch_apply(void* stream, const HistJob& a) {
    launch_or_record(stream, kd_hist_apply, a, dim3(hist_blocks(a), (unsigned)a.images));
}

}  // namespace svh
