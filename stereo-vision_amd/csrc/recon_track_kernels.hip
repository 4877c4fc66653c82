// Reconstruction::update with the track table in device memory (libviso2/src/reconstruction.cpp:72-145): the kernels
// listed in recon_internal.h, each over K objects (blockIdx.y = object, its ReconJob read from a table in device
// memory).  Everything here is integer work and pixel copies except k_rt_tracks, which is recon::track_outcome of
// recon_core.h, fp64 in the reference's order without FMA contraction, exactly as k_recon_tracks runs it.
//
// Bounds: every index that comes out of memory (a feature index of a match or a track, a position out of a scan) is
// tested against the job's sizes before it is used; B holds cap_tracks tracks and cap_px pixels, which the host sizes
// for n_old + n tracks and old_px + 2 n pixels, the most an update can produce.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "dev_common.h"
#include "recon_internal.h"

namespace svh {

namespace {

using mono::Mat;
using mono::Vec;

constexpr int RT_LANES = 64;   // k_rt_tracks: lanes (tracks) per workgroup, the SVD state of k_recon_tracks
constexpr int RT_SLAB = 40;    // J 16 | V 16 | w 4 | rv1 4
constexpr int RT_NONE = INT_MAX;

// a pointer out of the job table is device (or device-mapped pinned host) memory: as_global (dev_common.h) says so

__global__ __launch_bounds__(256) void k_rt_stage(const ReconJob* __restrict__ J) {
    const ReconJob& a = J[blockIdx.y];
    const int32_t at = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int seg = 0; seg < 2; seg++) {
        const uint4* src = reinterpret_cast<const uint4*>(as_global(a.up_src[seg]));
        uint4* dst = reinterpret_cast<uint4*>(as_global(a.up_dst[seg]));
        const int32_t n16 = (int32_t)(a.up_bytes[seg] / 16);
        for (int32_t k = at; k < n16; k += step) dst[k] = src[k];
    }
    int32_t* tidx = as_global(a.track_idx);
    for (int32_t k = at; k < a.tbl; k += step) tidx[k] = -1;
    int32_t* claim = as_global(a.claim);
    for (int32_t k = at; k < a.n_old; k += step) claim[k] = RT_NONE;
    if (at < RT_HDR) as_global(a.hdr)[at] = 0;
}

__global__ __launch_bounds__(256) void k_rt_scatter(const ReconJob* __restrict__ J) {
    const ReconJob& a = J[blockIdx.y];
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_old) return;
    const int32_t li = as_global(a.a_last)[t];
    if (li >= 0 && li < a.tbl) atomicMax(as_global(a.track_idx) + li, t);
}

__global__ __launch_bounds__(256) void k_rt_associate(const ReconJob* __restrict__ J) {
    const ReconJob& a = J[blockIdx.y];
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const svh_p_match* m = as_global(a.m);
    const int32_t ip = m[i].i1p, ic = m[i].i1c;
    int32_t idx = -1;
    if (ip < 0 || ip >= a.max_index || ic < 0 || ic >= a.max_index) {
        atomicOr(as_global(a.hdr) + RT_ERROR, RT_BAD_INDEX);
    } else {
        idx = as_global(a.track_idx)[ip];   // (max_index <= tbl)
        if (idx >= a.n_old) idx = -1;
        if (idx >= 0) atomicMin(as_global(a.claim) + idx, i);
    }
    as_global(a.midx)[i] = idx;
}

// One workgroup per object; thread t owns a contiguous run of old tracks and a contiguous run of matches, so thread
// order is track / match order.
__global__ __launch_bounds__(1024) void k_rt_scan(const ReconJob* __restrict__ J) {
    const ReconJob& a = J[blockIdx.y];
    __shared__ int32_t s_wave[16];
    const int t = threadIdx.x;
    int32_t* hdr = as_global(a.hdr);
    if ((int64_t)a.n_old + a.n > a.cap_tracks) {   // (uniform over the workgroup)
        if (t == 0) atomicOr(hdr + RT_ERROR, RT_NO_ROOM);
        return;
    }
    const int32_t* claim = as_global(a.claim);
    const int32_t* a_offs = as_global(a.a_offs);
    int32_t *src = as_global(a.src), *b_offs = as_global(a.b_offs), *lost = as_global(a.lost);
    // ---- old tracks: extended ones keep their order at the front of B, lost ones are listed in order
    const int32_t ct = (a.n_old + 1023) / 1024;
    const int32_t lo = min(t * ct, a.n_old), hi = min(lo + ct, a.n_old);
    int32_t ext = 0, px = 0;
    for (int32_t k = lo; k < hi; k++)
        if (claim[k] != RT_NONE) {
            ext++;
            px += a_offs[k + 1] - a_offs[k] + 1;
        }
    int32_t n_ext, ext_px;
    int32_t at = block_exclusive_scan<1024>(ext, s_wave, &n_ext);
    int32_t at_px = block_exclusive_scan<1024>(px, s_wave, &ext_px);
    int32_t at_lost = lo - at;
    for (int32_t k = lo; k < hi; k++) {
        if (claim[k] != RT_NONE) {
            src[at] = k;
            b_offs[at] = at_px;
            at++;
            at_px += a_offs[k + 1] - a_offs[k] + 1;
        } else {
            lost[at_lost++] = k;
        }
    }
    // ---- matches: one that did not win its track (or reached none) creates a track, in match order
    const int32_t* midx = as_global(a.midx);
    const int32_t cm = (a.n + 1023) / 1024;
    const int32_t mlo = min(t * cm, a.n), mhi = min(mlo + cm, a.n);
    int32_t cr = 0;
    for (int32_t i = mlo; i < mhi; i++) {
        const int32_t idx = midx[i];
        cr += !(idx >= 0 && claim[idx] == i);
    }
    int32_t n_cr;
    int32_t at_cr = block_exclusive_scan<1024>(cr, s_wave, &n_cr);
    for (int32_t i = mlo; i < mhi; i++) {
        const int32_t idx = midx[i];
        if (!(idx >= 0 && claim[idx] == i)) {
            src[n_ext + at_cr] = ~i;
            b_offs[n_ext + at_cr] = ext_px + 2 * at_cr;
            at_cr++;
        }
    }
    if (t == 0) {
        const int32_t total = ext_px + 2 * n_cr;
        b_offs[n_ext + n_cr] = total;
        hdr[RT_EXTENDED] = n_ext;
        hdr[RT_CREATED] = n_cr;
        hdr[RT_LOST] = a.n_old - n_ext;
        hdr[RT_PIXELS] = total;
        if (total > a.cap_px) atomicOr(hdr + RT_ERROR, RT_NO_ROOM);
    }
}

__global__ __launch_bounds__(256) void k_rt_gather(const ReconJob* __restrict__ J) {
    const ReconJob& a = J[blockIdx.y];
    const int32_t d = blockIdx.x * 256 + threadIdx.x;
    const int32_t* hdr = as_global(a.hdr);
    if (hdr[RT_ERROR] || d >= hdr[RT_EXTENDED] + hdr[RT_CREATED]) return;
    const svh_p_match* m = as_global(a.m);
    const int32_t s = as_global(a.src)[d], o = as_global(a.b_offs)[d];
    float2* out = reinterpret_cast<float2*>(as_global(a.b_px));
    if (s >= 0) {   // old track s, extended by match claim[s]
        if (s >= a.n_old) return;
        const int32_t ao = as_global(a.a_offs)[s], len = as_global(a.a_offs)[s + 1] - ao, i = as_global(a.claim)[s];
        if (i < 0 || i >= a.n || ao < 0 || len < 0 || ao + len > a.old_px || o < 0 || o + len + 1 > a.cap_px) return;
        const float2* in = reinterpret_cast<const float2*>(as_global(a.a_px));
        for (int32_t k = 0; k < len; k++) out[o + k] = in[ao + k];
        out[o + len] = make_float2(m[i].u1c, m[i].v1c);
        as_global(a.b_first)[d] = as_global(a.a_first)[s];
        as_global(a.b_last)[d] = m[i].i1c;
    } else {        // created by match ~s
        const int32_t i = ~s;
        if (i >= a.n || o < 0 || o + 2 > a.cap_px) return;
        out[o] = make_float2(m[i].u1p, m[i].v1p);
        out[o + 1] = make_float2(m[i].u1c, m[i].v1c);
        as_global(a.b_first)[d] = a.frame_prev;
        as_global(a.b_last)[d] = m[i].i1c;
    }
}

// k_recon_tracks over the lost tracks where they lie in A: lane g evaluates track lost[g]
__global__ __launch_bounds__(RT_LANES) void k_rt_tracks(const ReconJob* __restrict__ J) {
    __shared__ double slab[RT_SLAB * RT_LANES];
    const ReconJob& a = J[blockIdx.y];
    const int lane = threadIdx.x;
    const int32_t g = blockIdx.x * RT_LANES + lane;
    const int32_t* hdr = as_global(a.hdr);
    if (hdr[RT_ERROR] || g >= hdr[RT_LOST]) return;
    const int32_t t = as_global(a.lost)[g];
    double* base = slab + lane;
    const Mat Jm{base, 4, RT_LANES}, V{base + 16 * RT_LANES, 4, RT_LANES};
    const Vec w{base + 32 * RT_LANES, RT_LANES}, rv1{base + 36 * RT_LANES, RT_LANES};
    float p[3] = {0.f, 0.f, 0.f};
    int32_t c = recon::INIT_FAILED;
    if (t >= 0 && t < a.n_old) {
        const int32_t o = as_global(a.a_offs)[t], nf = as_global(a.a_offs)[t + 1] - o, f0 = as_global(a.a_first)[t];
        // a track that would read outside the pixel or frame arrays is not evaluated
        if (nf >= 2 && o >= 0 && o + nf <= a.old_px && f0 >= 0 && f0 + nf <= a.n_frames)
            c = recon::track_outcome(as_global(a.frames), f0, as_global(a.a_px) + 2 * (size_t)o, nf, a.s, Jm, V, w, rv1, p);
    }
    as_global(a.code)[g] = c;
    float* xyz = as_global(a.xyz);
    xyz[3 * (size_t)g + 0] = p[0];
    xyz[3 * (size_t)g + 1] = p[1];
    xyz[3 * (size_t)g + 2] = p[2];
}

// k_recon_compact with the count taken from the device header; the header goes to pinned host memory as well
__global__ __launch_bounds__(256) void k_rt_compact(const ReconJob* __restrict__ J) {
    __shared__ int32_t s_wave[4];
    const ReconJob& a = J[blockIdx.y];
    const int32_t* hdr = as_global(a.hdr);
    int32_t* out_hdr = as_global(a.out_hdr);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t err = hdr[RT_ERROR];
    const int32_t n_lost = err ? 0 : min(hdr[RT_LOST], a.n_old);
    const int32_t* code = as_global(a.code);
    const float* xyz = as_global(a.xyz);
    float* points = as_global(a.points);
    int32_t* out_code = as_global(a.out_code);
    float* out_xyz = as_global(a.out_xyz);
    int32_t running = a.n_points;
    for (int32_t b = 0; b < n_lost; b += 256) {
        const int32_t i = b + (int32_t)threadIdx.x;
        const int32_t c = i < n_lost ? code[i] : -1;
        float p[3] = {0.f, 0.f, 0.f};
        if (i < n_lost) {
            for (int k = 0; k < 3; k++) p[k] = xyz[3 * (size_t)i + k];
            out_code[i] = c;
            for (int k = 0; k < 3; k++) out_xyz[3 * (size_t)i + k] = p[k];
        }
        const bool take = c == recon::ACCEPTED;
        const unsigned long long mask = __ballot(take);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int k = 0; k < 4; k++) {
            before += k < wave ? s_wave[k] : 0;
            total += s_wave[k];
        }
        if (take) {
            const size_t at = (size_t)running + before + __popcll(mask & ((1ull << lane) - 1ull));
            for (int k = 0; k < 3; k++) points[3 * at + k] = p[k];
        }
        running += total;
        __syncthreads();
    }
    if (threadIdx.x < RT_HDR) {
        const int k = threadIdx.x;
        out_hdr[k] = k == RT_POINTS ? running : hdr[k];
    }
}

unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

}  // namespace

void rlaunch_resident(void* stream, const ReconJob* d_jobs, int32_t K, int32_t max_n, int32_t max_old, int32_t max_tbl,
                      uint32_t max_up) {
    hipStream_t st = (hipStream_t)stream;
    if (K <= 0) return;
    const int64_t stage = std::max<int64_t>(std::max<int64_t>(max_tbl, max_old), max_up / 16);
    k_rt_stage<<<dim3(std::min(blocks(stage, 256), 128u), K), 256, 0, st>>>(d_jobs);
    if (max_old > 0) k_rt_scatter<<<dim3(blocks(max_old, 256), K), 256, 0, st>>>(d_jobs);
    if (max_n > 0) k_rt_associate<<<dim3(blocks(max_n, 256), K), 256, 0, st>>>(d_jobs);
    k_rt_scan<<<dim3(1, K), 1024, 0, st>>>(d_jobs);
    if ((int64_t)max_old + max_n > 0) k_rt_gather<<<dim3(blocks((int64_t)max_old + max_n, 256), K), 256, 0, st>>>(d_jobs);
    if (max_old > 0) k_rt_tracks<<<dim3(blocks(max_old, RT_LANES), K), RT_LANES, 0, st>>>(d_jobs);
    k_rt_compact<<<dim3(1, K), 256, 0, st>>>(d_jobs);
}

}  // namespace svh
