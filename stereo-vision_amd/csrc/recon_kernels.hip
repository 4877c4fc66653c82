// Reconstruction::update on the device (libviso2/src/reconstruction.cpp:118-349): what happens to the tracks that
// were lost in this update.
//
// k_recon_tracks   one lane per lost track: initPoint (4x4 SVD, its state in LDS interleaved across the lanes of the
//                  workgroup as in k_mono_chiral), pointType, up to 22 Gauss-Newton updates over the track's frames
//                  (sums in registers, the projection matrices and pixels read from global memory, so a track may
//                  have any length), pointDistance, rayAngle.  Output: the outcome code and the point of the track.
//                  `order` (optional) maps a lane to its track, so the host can hand tracks of similar length to the
//                  lanes of one wave; results are stored at the track's own index.
// k_recon_compact  one workgroup: appends the ACCEPTED points, in track order (the reference appends in tracks_copy
//                  order, :119-145), to the resident point array, and hands the codes, the points and the new count
//                  to pinned host memory.
// All arithmetic is fp64 in the reference's operation order (recon_core.h), no FMA contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_core.h"
#include "vo_internal.h"

namespace svh {

namespace {

using mono::Mat;
using mono::Vec;

constexpr int TRK_LANES = 64;   // lanes (tracks) per workgroup: 40 x 8 B x 64 = 20 KB LDS
constexpr int TRK_SLAB = 40;    // J 16 | V 16 | w 4 | rv1 4

__global__ __launch_bounds__(TRK_LANES) void k_recon_tracks(const int32_t* __restrict__ offs,
                                                            const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ order,
                                                            const float* __restrict__ px, int32_t n_lost,
                                                            int32_t n_px, const double* __restrict__ frames,
                                                            int32_t n_frames, recon::Settings s,
                                                            int32_t* __restrict__ code, float* __restrict__ xyz) {
    __shared__ double slab[TRK_SLAB * TRK_LANES];
    const int lane = threadIdx.x;
    const int32_t g = blockIdx.x * TRK_LANES + lane;
    if (g >= n_lost) return;
    int32_t t = order ? order[g] : g;
    t = t < 0 ? 0 : (t >= n_lost ? n_lost - 1 : t);   // (a permutation made on the host; clamped all the same)
    double* base = slab + lane;
    const Mat J{base, 4, TRK_LANES}, V{base + 16 * TRK_LANES, 4, TRK_LANES};
    const Vec w{base + 32 * TRK_LANES, TRK_LANES}, rv1{base + 36 * TRK_LANES, TRK_LANES};
    const int32_t o = offs[t], nf = offs[t + 1] - o, f0 = first[t];
    float p[3] = {0.f, 0.f, 0.f};
    int32_t c = recon::INIT_FAILED;
    // the host gathers consistent tracks; one that would read outside the pixel or frame arrays is not evaluated
    if (nf >= 2 && o >= 0 && o + nf <= n_px && f0 >= 0 && f0 + nf <= n_frames)
        c = recon::track_outcome(frames, f0, px + 2 * (size_t)o, nf, s, J, V, w, rv1, p);
    code[t] = c;
    xyz[3 * (size_t)t + 0] = p[0];
    xyz[3 * (size_t)t + 1] = p[1];
    xyz[3 * (size_t)t + 2] = p[2];
}

__global__ __launch_bounds__(256) void k_recon_compact(const int32_t* __restrict__ code,
                                                       const float* __restrict__ xyz, int32_t n_lost,
                                                       float* __restrict__ points, int32_t n_points,
                                                       int32_t* __restrict__ out_code, float* __restrict__ out_xyz,
                                                       int32_t* __restrict__ out_count) {
    __shared__ int32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t running = n_points;
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
        const unsigned long long m = __ballot(take);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int k = 0; k < 4; k++) {
            before += k < wave ? s_wave[k] : 0;
            total += s_wave[k];
        }
        if (take) {
            const size_t at = (size_t)running + before + __popcll(m & ((1ull << lane) - 1ull));
            for (int k = 0; k < 3; k++) points[3 * at + k] = p[k];
        }
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) out_count[0] = running;
}

}  // namespace

void rlaunch_tracks(void* stream, const int32_t* offs, const int32_t* first, const int32_t* order, const float* px,
                    int32_t n_lost, int32_t n_px, const double* frames, int32_t n_frames, const recon::Settings& s,
                    int32_t* code, float* xyz, float* points, int32_t n_points, int32_t* out_code, float* out_xyz,
                    int32_t* out_count) {
    hipStream_t st = (hipStream_t)stream;
    if (n_lost > 0)
        k_recon_tracks<<<(n_lost + TRK_LANES - 1) / TRK_LANES, TRK_LANES, 0, st>>>(offs, first, order, px, n_lost,
                                                                                  n_px, frames, n_frames, s, code,
                                                                                  xyz);
    k_recon_compact<<<1, 256, 0, st>>>(code, xyz, n_lost, points, n_points, out_code, out_xyz, out_count);
}

}  // namespace svh
